// Implicit-GEMM 3x3 / 1x1 convolution on the gfx950 fp32 matrix cores
// (v_mfma_f32_32x32x2_f32: exact f32, 157.3 TFLOP/s chip peak).
//
// One kernel serves every contraction on the E4S hot path:
//   * generator StyledConv, masked   : REGION-SELECT AT FRAGMENT LEVEL (spatial mode + label map):
//     every output pixel is one GEMM row whose A fragment is scaled, on its way into the MFMA, by
//     the style s[region(pixel)][ci] of that pixel's own region, and whose accumulator is
//     demodulated with d[region(pixel)][co] -- every pixel is computed once instead of the
//     reference's 12 full passes + one-hot mask multiply (model.py:386-400), with no padding and
//     no dependence on the mask geometry.  (A region-gathered row plan, `plan` mode, is kept as a
//     second, independently tested formulation.)
//   * generator up-conv              : conv_transpose2d(stride 2) (*) 4x4 blur (model.py:287-300)
//     folded into 4 phase-specific 3x3 kernels over the input grid (ncls = 4)
//   * generator StyledConv, unmasked : natural order, halo-tiled loader (SPATIAL)
//   * encoder Conv2d 3x3 (stride 1/2) and the 1x1 stride-2 shortcut (helpers.py:122-144)
//
// GEMM view: M = rows (pixels), N = Cout, K = taps x Cin.  A = activations (NHWC, so one tap of
// one pixel is a contiguous Cin vector), B = weights [cls][tap][Cout][Cin].
// Block = 256 threads = 4 waves; block tile BM x BN, K step 32; each wave owns TM x TN
// 32x32 MFMA blocks (16 accumulator VGPRs each).  Both operands are staged global -> VGPR ->
// LDS (double buffered, one barrier per K step; next step's global loads are in flight during
// the MFMAs).  LDS rows are 36 floats (144 B) so ds_read_b128 fragment reads are conflict free.
// Style modulation s[g][ci] is applied to the B tile while it is staged (input-scaling form,
// model.py:245-274); demodulation, noise, bias and leaky-ReLU live in the epilogue.
#include "conv_launch.h"
#include <stdlib.h>

namespace {

constexpr int KC = 32;    // K step (input channels per stage)
constexpr int LDA = 36;   // padded LDS row, floats
constexpr int NTHR = 256;

template <int BM, int BN, bool SPATIAL>
struct SmemLayout {
    static constexpr int TH = 8, TW = BM / 8, HALO_W = TW + 2, HALO = (TH + 2) * HALO_W;
    static constexpr int META_WORDS = 4 * BM;
    static constexpr int A_WORDS = SPATIAL ? HALO * LDA : 2 * BM * LDA;
    static constexpr int B_WORDS = 2 * BN * LDA;
    static constexpr int MAXR = 16;                                   // regions per sample (spatial mode)
    static constexpr int S_WORDS = SPATIAL ? MAXR * LDA : 0;          // style chunk s[r][32] of the current K step
    static constexpr int BYTES = (META_WORDS + A_WORDS + B_WORDS + S_WORDS) * 4;
};

template <int BM, int BN, int WM, int WN, bool SPATIAL, int PF>
__global__ __launch_bounds__(NTHR, 2) void conv_mfma_kernel(const e4s_conv_params p, const int ntn,
                                                            const int tiles_per_cls, const int ksplit, const int cper) {
    using L = SmemLayout<BM, BN, SPATIAL>;
    constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
    constexpr int TH = L::TH, TW = L::TW, HALO_W = L::HALO_W, HALO = L::HALO;
    constexpr int AR = BM / 32, BR = BN / 32, HR = (HALO + 31) / 32;
    constexpr int PA = SPATIAL ? HR : AR;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    int* s_out = reinterpret_cast<int*>(smem_raw);
    float* s_nz = reinterpret_cast<float*>(s_out + BM);
    int* s_base = reinterpret_cast<int*>(s_nz + BM);
    int* s_yx = s_base + BM;
    float* sA = reinterpret_cast<float*>(s_yx + BM);
    float* sB = sA + L::A_WORDS;
    float* sS = sB + L::B_WORDS;
    int* s_grp = s_base;                 // spatial mode: region index of each row (s_base is gather-only)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;

    // ---- which tile ------------------------------------------------------------------
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = logical / ntn, nt = logical - mt * ntn;
    const int n0 = nt * BN;
    const bool plan = (p.tiles != nullptr);
    int row_start = 0, g = 0, cls = 0, tt = mt, tb = 0, tyb = 0, txb = 0, plan_rows = 0;
    if (plan) {
        if (mt >= p.meta[0] || mt >= p.tiles_cap) return;
        row_start = p.tiles[mt * 4 + 0];
        g = p.tiles[mt * 4 + 1];
        cls = p.tiles[mt * 4 + 2];
        plan_rows = p.tiles[mt * 4 + 3];               // real rows of this tile; the rest of its BM slots are padding
        // a plan that does not describe THIS launch (stale or clobbered tables) must not become an address
        if (row_start < 0 || plan_rows < 0 || plan_rows > BM || (unsigned)g >= (unsigned)(p.B * p.groups_per_batch) ||
            (unsigned)cls >= (unsigned)p.ncls)
            return;
    } else {
        cls = mt / tiles_per_cls;
        tt = mt - cls * tiles_per_cls;
        if (SPATIAL) {
            const int tx_n = (p.Wa + TW - 1) / TW, per_img = ((p.Ha + TH - 1) / TH) * tx_n;
            tb = tt / per_img;
            const int rem = tt - tb * per_img;
            tyb = rem / tx_n;
            txb = rem - tyb * tx_n;
            g = tb;
        } else {
            g = (tt * BM) / (p.Ha * p.Wa);
        }
    }
    const int py = (p.ncls == 4) ? (cls >> 1) : 0, px = (p.ncls == 4) ? (cls & 1) : 0;

    // ---- per-row metadata ------------------------------------------------------------
    if (tid < BM) {
        int b, ay, ax;
        bool valid = true;
        if (SPATIAL) {
            b = tb;
            ay = tyb * TH + tid / TW;
            ax = txb * TW + tid % TW;
            valid = ay < p.Ha && ax < p.Wa;
        } else {
            const int anchor = plan ? (tid < plan_rows ? p.rows[row_start + tid] : -1) : tt * BM + tid;
            valid = anchor >= 0 && anchor < p.B * p.Ha * p.Wa;             // natural order: the last tile may be ragged
            const int a = valid ? anchor : 0;
            const int hw = p.Ha * p.Wa;
            b = a / hw;
            const int rem = a - b * hw;
            ay = rem / p.Wa;
            ax = rem - ay * p.Wa;
        }
        if (valid) {
            const int oy = ay * p.ostride + py, ox = ax * p.ostride + px;
            s_out[tid] = (b * p.Ho + oy) * p.Wo + ox;
            const int64_t npix = (int64_t)b * p.noise_bstride + (int64_t)oy * p.Wo + ox;
            if (!p.noise) s_nz[tid] = 0.f;
            else if (p.noise_per_channel) s_nz[tid] = __int_as_float((int)npix);
            else s_nz[tid] = p.noise_w[0] * p.noise[npix];
            const int by = ay * p.istride, bx = ax * p.istride;
            if (SPATIAL) {
                int r = 0;
                if (p.labels) {   // legacy-nearest lookup of the OUTPUT pixel (F.interpolate 'nearest', model.py:391)
                    const int sy = min((int)floorf((float)oy * ((float)p.Hm / (float)p.Ho)), p.Hm - 1);
                    const int sx = min((int)floorf((float)ox * ((float)p.Wm / (float)p.Wo)), p.Wm - 1);
                    r = p.labels[((size_t)b * p.Hm + sy) * p.Wm + sx];
                }
                s_grp[tid] = r;
            } else {
                s_base[tid] = (b * p.Hi + by) * p.Wi + bx;
            }
            s_yx[tid] = (by << 16) | bx;
        } else {
            s_out[tid] = -1;
            s_nz[tid] = 0.f;
            s_base[tid] = 0;
            s_yx[tid] = 0x7fff7fff;
        }
    }
    __syncthreads();

    // ---- staging roles: thread -> (row r0 + 32 j, 16-byte chunk c of the 32-float K step) ----
    const int c4 = (tid & 7) * 4, r0 = tid >> 3;
    int a_base[AR], a_yx[AR];
    if (!SPATIAL) {
#pragma unroll
        for (int j = 0; j < AR; ++j) {
            a_base[j] = s_base[r0 + 32 * j];
            a_yx[j] = s_yx[r0 + 32 * j];
        }
    }
    const int R = SPATIAL ? (p.labels ? p.groups_per_batch : 1) : 1;
    const bool scaled = p.in_scale != nullptr;
    // gather: tile-uniform group, style folded into the B tile while staging.
    // spatial: per-row region, style applied to the A fragment; the K-step slice of the table lives in LDS.
    const float* sscale = (!SPATIAL && scaled) ? p.in_scale + (size_t)g * p.Cin : nullptr;
    const float* stable = (SPATIAL && scaled) ? p.in_scale + (size_t)tb * R * p.Cin : nullptr;
    // prefetch registers of one pipeline stage (global -> VGPR, later VGPR -> LDS)
    struct Pref {
        f32x4 a[PA];
        f32x4 b[BR];
        f32x4 s;
        unsigned ok;      // bit j: a[j] is a real (in-image) sample; applied when the registers are written to LDS, so
                          // that nothing consumes a load result before the stage that needs it
    };
    // split-K (ksplit > 1: launches whose tiles alone leave most CUs idle -- 14x14 / 7x7 maps, batch-1 low resolutions):
    // blockIdx.y owns the input-channel chunks [c_lo, c_hi), stores its raw partial sums (x demodulation) into slab
    // blockIdx.y of p.splitk_ws, and a second kernel adds the slabs in order and applies the epilogue
    const int ntaps = p.ntaps, nchunk = p.Cin / KC;
    const int ks = blockIdx.y;
    const int c_lo = ks * cper, c_hi = (c_lo + cper < nchunk) ? c_lo + cper : nchunk;
    const int nstage = (c_hi - c_lo) * ntaps, cbeg = c_lo * KC;

    auto fetch = [&](Pref& P, int tap, int c0) {
        const bool new_chunk = (tap == 0);
        const float* wp = p.w + ((size_t)(cls * ntaps + tap) * p.Cout + n0) * p.Cin + c0 + c4;
#pragma unroll
        for (int j = 0; j < BR; ++j) P.b[j] = *reinterpret_cast<const f32x4*>(wp + (size_t)(r0 + 32 * j) * p.Cin);
        if (sscale) {
            const f32x4 sv = *reinterpret_cast<const f32x4*>(sscale + c0 + c4);
#pragma unroll
            for (int j = 0; j < BR; ++j) P.b[j] *= sv;
        }
        if (SPATIAL) {
            if (new_chunk) {
                unsigned okm = 0;
#pragma unroll
                for (int j = 0; j < HR; ++j) {
                    const int h = r0 + 32 * j;
                    const int hy = h / HALO_W, hx = h - hy * HALO_W;
                    const int iy = tyb * TH + hy - 1, ix = txb * TW + hx - 1;
                    // branch-free: out-of-image halo pixels load a valid dummy address and are zeroed by a select, so
                    // the loads stay in one basic block and the compiler can use counted s_waitcnt vmcnt(N)
                    const bool ok = h < HALO && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
                    const size_t off = ok ? ((size_t)(tb * p.Hi + iy) * p.Wi + ix) * p.Cin : 0;
                    P.a[j] = *reinterpret_cast<const f32x4*>(p.x + off + c0 + c4);
                    okm |= (ok ? 1u : 0u) << j;
                }
                P.ok = okm;
                if (stable) {
                    const int sr = min(tid >> 3, R - 1);
                    P.s = *reinterpret_cast<const f32x4*>(stable + (size_t)sr * p.Cin + c0 + c4);
                }
            }
        } else {
            const int kw = ntaps == 25 ? 5 : ntaps == 9 ? 3 : 1;      // square k x k taps, 'same' padding k/2
            const int oy = tap / kw - kw / 2 + p.tap_shift, ox = tap % kw - kw / 2 + p.tap_shift;
            const int doff = oy * p.Wi + ox;
            unsigned okm = 0;
#pragma unroll
            for (int j = 0; j < AR; ++j) {
                const int iy = (a_yx[j] >> 16) + oy, ix = (a_yx[j] & 0xffff) + ox;
                const bool ok = (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
                const size_t off = ok ? (size_t)(a_base[j] + doff) * p.Cin : 0;
                P.a[j] = *reinterpret_cast<const f32x4*>(p.x + off + c0 + c4);
                okm |= (ok ? 1u : 0u) << j;
            }
            P.ok = okm;
        }
    };
    // VGPR -> LDS for the stage whose first tap flag is `new_chunk`; B (and gather A) go to buffer `buf`
    auto store = [&](const Pref& P, int buf, bool new_chunk) {
        float* d = sB + buf * (BN * LDA) + r0 * LDA + c4;
#pragma unroll
        for (int j = 0; j < BR; ++j) *reinterpret_cast<f32x4*>(d + 32 * j * LDA) = P.b[j];
        if (SPATIAL) {
            if (new_chunk) {
#pragma unroll
                for (int j = 0; j < HR; ++j) {
                    const int h = r0 + 32 * j;
                    if (h < HALO)
                        *reinterpret_cast<f32x4*>(sA + h * LDA + c4) = ((P.ok >> j) & 1u) ? P.a[j] : f32x4{0.f, 0.f, 0.f, 0.f};
                }
                if (stable && tid < R * 8) *reinterpret_cast<f32x4*>(sS + (tid >> 3) * LDA + c4) = P.s;
            }
        } else {
            float* da = sA + buf * (BM * LDA) + r0 * LDA + c4;
#pragma unroll
            for (int j = 0; j < AR; ++j)
                *reinterpret_cast<f32x4*>(da + 32 * j * LDA) = ((P.ok >> j) & 1u) ? P.a[j] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };

    // ---- fragment addressing ---------------------------------------------------------
    int arow[TM], brow[TN], srow[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int m = (wm * TM + tm) * 32 + li;
        arow[tm] = SPATIAL ? ((m / TW) * HALO_W + (m % TW)) * LDA : m * LDA;
        srow[tm] = SPATIAL ? s_grp[m] * LDA : 0;
    }
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) brow[tn] = ((wn * TN + tn) * 32 + li) * LDA;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    auto compute = [&](int s, int tap) {
        const int buf = s & 1;
        const float* Ab = SPATIAL ? sA + ((tap / 3) * HALO_W + (tap % 3)) * LDA : sA + buf * (BM * LDA);
        const float* Bb = sB + buf * (BN * LDA);
#pragma unroll
        for (int kk = 0; kk < KC / 8; ++kk) {
            f32x4 a[TM], b[TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) a[tm] = *reinterpret_cast<const f32x4*>(Ab + arow[tm] + kk * 8 + kh * 4);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) b[tn] = *reinterpret_cast<const f32x4*>(Bb + brow[tn] + kk * 8 + kh * 4);
            if (SPATIAL && scaled) {
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) a[tm] *= *reinterpret_cast<const f32x4*>(sS + srow[tm] + kk * 8 + kh * 4);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][e], b[tn][e], acc[tm][tn], 0, 0, 0);
        }
    };
    auto advance = [&](int& tap, int& c0) {
        if (++tap == ntaps) { tap = 0; c0 += KC; }
    };

    // ---- software pipeline: LDS holds stage s, registers hold stage s+1 (PF == 1) or s+1 and s+2 (PF == 2:
    // the small column tiles have only ~1000 MFMA cycles per stage, not enough to cover an L2 round trip) ----
    Pref P0, P1;
    P0.s = P1.s = f32x4{1.f, 1.f, 1.f, 1.f};
    P0.ok = P1.ok = 0u;
    int tap = 0, c0 = cbeg, t1 = 0, c1 = cbeg;
    advance(t1, c1);
    fetch(P0, 0, cbeg);
    store(P0, 0, true);
    if (PF == 2 && nstage > 1) fetch(P1, t1, c1);
    __syncthreads();

    if (PF == 1) {
        for (int s = 0; s < nstage; ++s) {
            const bool more = (s + 1 < nstage);
            const bool new_chunk = (t1 == 0);
            if (more) fetch(P0, t1, c1);
            compute(s, tap);
            if (more) {
                if (SPATIAL && new_chunk) __syncthreads();   // single A halo buffer: everyone done reading it
                store(P0, (s + 1) & 1, new_chunk);
            }
            __syncthreads();
            tap = t1; c0 = c1;
            advance(t1, c1);
        }
    } else {
        int t2 = t1, c2 = c1;
        advance(t2, c2);
        // steady state: the prefetch is unconditional (a conditional load would force s_waitcnt vmcnt(0) on the
        // older register set); the last stages run the guarded form
        auto step = [&](Pref& Pf, const Pref& Ps, int s, bool guarded) {
            if (!guarded || s + 2 < nstage) fetch(Pf, t2, c2);
            compute(s, tap);
            if (!guarded || s + 1 < nstage) {
                const bool new_chunk = (t1 == 0);
                if (SPATIAL && new_chunk) __syncthreads();
                store(Ps, (s + 1) & 1, new_chunk);
            }
            __syncthreads();
            tap = t1; c0 = c1;
            t1 = t2; c1 = c2;
            advance(t2, c2);
        };
        int s = 0;
        for (; s + 3 < nstage; s += 2) {
            step(P0, P1, s, false);
            step(P1, P0, s + 1, false);
        }
        for (; s < nstage; s += 2) {
            step(P0, P1, s, true);
            if (s + 1 < nstage) step(P1, P0, s + 1, true);
        }
    }
    (void)c0;

    // ---- epilogue: demod * acc + noise + bias, activation, scatter to NHWC ------------
    // spatial mode: the demodulation coefficient depends on the row's region -> table d[r][n] in LDS
    // (the A region is free: the loop's last barrier has passed)
    float* sD = sA;
    if (SPATIAL && p.out_scale) {
        for (int t = tid; t < R * BN; t += NTHR) {
            const int r = t / BN, n = t - r * BN;
            sD[t] = p.out_scale[((size_t)tb * R + r) * p.Cout + n0 + n];
        }
        __syncthreads();
    }
    float osc[TN], bsv[TN], slp[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int col = n0 + (wn * TN + tn) * 32 + li;
        osc[tn] = (!SPATIAL && p.out_scale) ? p.out_scale[(size_t)g * p.Cout + col] : 1.f;
        bsv[tn] = p.bias ? p.bias[col] : 0.f;
        slp[tn] = (p.act == 2) ? p.slope[col] : p.alpha;
    }
    const float gain = (p.act == 1) ? p.gain : 1.f;
    const bool do_act = p.act != 0;
    const bool nz_pc = p.noise && p.noise_per_channel;
    const float nzw = nz_pc ? p.noise_w[0] : 0.f;
    const bool row_scale = SPATIAL && p.out_scale;
    const int ycs = p.y_cstride ? p.y_cstride : p.Cout;
    const bool raw = ksplit > 1;
    float* yo = raw ? p.splitk_ws + (size_t)ks * ((size_t)p.B * p.Ho * p.Wo * ycs) : p.y;
    // epilogue math per element, then 4x4 quad transposes: 16-byte NHWC stores instead of four times as many 4-byte ones (common.h)
    const bool wide = (ycs & 3) == 0;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            float v[TN][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * g4 + i;
                const int row = (wm * TM + tm) * 32 + i + 8 * g4 + 4 * kh;
                const float nz = s_nz[row];
                const float* drow = sD + (row_scale ? s_grp[row] * BN : 0);
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    const int ncol = (wn * TN + tn) * 32 + li;
                    const float sc = row_scale ? drow[ncol] : osc[tn];
                    float t = acc[tm][tn][r] * sc;
                    if (!raw) {
                        const float nzv = nz_pc ? nzw * p.noise[(size_t)__float_as_int(nz) * p.Cout + n0 + ncol] : nz;
                        t += nzv + bsv[tn];
                        if (do_act) t = (t > 0.f ? t : t * slp[tn]) * gain;
                    }
                    v[tn][i] = t;
                }
            }
            if (wide) {
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) quad_transpose4(v[tn][0], v[tn][1], v[tn][2], v[tn][3], li);
                const int off = s_out[(wm * TM + tm) * 32 + (li & 3) + 8 * g4 + 4 * kh];
                if (off >= 0) {
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        *reinterpret_cast<f32x4*>(yo + (size_t)off * ycs + n0 + (wn * TN + tn) * 32 + (li & ~3)) =
                            f32x4{v[tn][0], v[tn][1], v[tn][2], v[tn][3]};
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int off = s_out[(wm * TM + tm) * 32 + i + 8 * g4 + 4 * kh];
                    if (off < 0) continue;
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) yo[(size_t)off * ycs + n0 + (wn * TN + tn) * 32 + li] = v[tn][i];
                }
            }
        }
    }
}

// Split-K policy of the fp32 kernel.  It depends on ONE sample's pixel tiles and the channel count only -- never on the batch
// or on the column tile the dispatch picks (which follows the batch) -- so a sample's result does not depend on what it is
// batched with: maps of <= 2 pixel tiles (<= 16x16: IR-SE50's 14x14 / 7x7 layers, the generator's 4^2-16^2 layers) split
// their input-channel chunks up to 8 ways (round 6: down to ONE 32-channel chunk per split -- these launches are a chain of exposed stage
// latencies, 16.6 us each and 69 of them per config-3 step; five alternations on one box: 13.12 -> 12.80 ms per step); larger maps with < 256 blocks per sample split just enough to get there.
inline void f32_split(const e4s_conv_params& p, int64_t tiles_per_sample, int& ksplit, int& cper) {
    const int nchunk = p.Cin / KC;
    ksplit = 1;
    cper = nchunk;
    if (tiles_per_sample < 1 || nchunk < 4 || p.noise_per_channel || !p.splitk_ws) return;
#ifdef E4S_ABLATIONS      // profiling builds only: the three switches of this rule
    static const int max_split = [] { const char* e = getenv("E4S_F32_MAX_SPLIT"); return e && atoi(e) > 0 ? atoi(e) : 8; }();
    static const int min_chunks = [] { const char* e = getenv("E4S_F32_MIN_CHUNKS"); return e && atoi(e) > 0 ? atoi(e) : 1; }();
    static const int forced = [] { const char* e = getenv("E4S_F32_PLAIN_SPLIT"); return e ? atoi(e) : -1; }();
#else
    constexpr int max_split = 8, min_chunks = 1, forced = -1;
#endif
    int want = nchunk / min_chunks;
    if (want > max_split) want = max_split;
    if (tiles_per_sample > 2) {
        // (plain contractions only: the styled / masked / tiled forms were never split above 2 tiles and their epilogues are not built for it)
        // OPT-IN (p.split_hint, set by the frozen loss networks; profiling builds: E4S_F32_PLAIN_SPLIT=1 forces it everywhere, =0 forbids it): the re-ordered sums
        // are as accurate as the unsplit ones (7e-7 of scale vs fp64), but through the TRAINED encoder's PReLU gates a re-ordering alone moved the
        // worst weight-gradient tensor of the fp64 gradient test from 1.7e-3 to 3.1e-3 relative L2 (gate flips on 512-pixel maps)
        const bool on = forced >= 0 ? forced != 0 : p.split_hint != 0;
        if (!on || p.labels || p.in_scale || p.out_scale || p.noise || p.tiles || p.in_stats || p.ncls != 1) return;
        // Round 6: maps of a few dozen tiles too (the batch-1 encoder's stride-2 convs: 32 tiles x 4 column tiles = 128 blocks per sample, one
        // block per CU, every stage an exposed gather round trip -- 125-150 us for 2.4 GFLOP): split until a SAMPLE has >= 256 blocks
        const int64_t per_sample = tiles_per_sample * (p.Cout / 32);
        if (per_sample >= 256) return;
        const int need = (int)((256 + per_sample - 1) / per_sample);
        if (want > need) want = need;
        if (want < 2) return;
    }
    cper = (nchunk + want - 1) / want;
    ksplit = (nchunk + cper - 1) / cper;
}

template <int BM, bool SPATIAL>
int64_t tiles_per_sample(const e4s_conv_params& p) {
    if (SPATIAL) return (int64_t)((p.Ha + 7) / 8) * ((p.Wa + BM / 8 - 1) / (BM / 8)) * p.ncls;
    return (((int64_t)p.Ha * p.Wa + BM - 1) / BM + (p.tiles ? 1 : 0)) * p.ncls;
}

template <int BM, int BN, int WM, int WN, bool SPATIAL, int PF = 1>
int launch(const e4s_conv_params& p, hipStream_t st) {
    using L = SmemLayout<BM, BN, SPATIAL>;
    auto kern = conv_mfma_kernel<BM, BN, WM, WN, SPATIAL, PF>;
    static std::atomic<uint64_t> smem_set{0};
    if (int e = e4s_ensure_dyn_smem(reinterpret_cast<const void*>(kern), L::BYTES, smem_set)) return e;
    const int ntn = p.Cout / BN;
    int mtiles, tiles_per_cls = 0;
    if (p.tiles) {
        mtiles = p.tiles_cap;
    } else if (SPATIAL) {
        tiles_per_cls = p.B * ((p.Ha + L::TH - 1) / L::TH) * ((p.Wa + L::TW - 1) / L::TW);
        mtiles = tiles_per_cls * p.ncls;
    } else {
        // the tile-uniform group (style / demodulation row) needs tiles that never straddle two samples; without those
        // operands (plain convs: encoder shortcuts, the loss networks' 7x7 ... 127x127 maps) any grid goes, ragged tail included
        if (((int64_t)p.Ha * p.Wa) % BM && (p.in_scale || p.out_scale)) return (int)hipErrorInvalidValue;
        tiles_per_cls = (int)(((int64_t)p.B * p.Ha * p.Wa + BM - 1) / BM);
        mtiles = tiles_per_cls * p.ncls;
    }
    if (mtiles <= 0) return 0;
    int ksplit, cper;
    f32_split(p, tiles_per_sample<BM, SPATIAL>(p) / p.ncls, ksplit, cper);
    hipLaunchKernelGGL(kern, dim3(mtiles * ntn, ksplit), dim3(NTHR), L::BYTES, st, p, ntn, tiles_per_cls, ksplit, cper);
    E4S_CHECK_LAUNCH();
    if (ksplit > 1) return e4s_splitk_epilogue(p, ksplit, false, st);     // slabs already carry the demodulation
    return 0;
}

// Column-tile width: the widest BN that still yields >= 2 blocks per CU (256 CUs); small problems
// (low resolutions, batch 1) take narrower tiles so the serial K loop of one block is shorter.
int pick_bn(const e4s_conv_params& p, int64_t mtiles) {
    const int cands[3] = {128, 64, 32};
    for (int i = 0; i < 3; ++i) {
        const int bn = cands[i];
        if (p.Cout % bn) continue;
        if (mtiles * (p.Cout / bn) >= 512 || bn == 32) return bn;
    }
    return 32;
}

}  // namespace

// the tile the dispatch below picks for a launch with few blocks per sample (the only launches that split)
extern "C" int64_t e4s_conv_mfma_ws_floats(const e4s_conv_params* pp, int spatial) {
    e4s_conv_params p = *pp;
    if (p.Cin % KC || p.Cout % 32) return 0;
    float dummy;
    p.splitk_ws = &dummy;                                        // "the caller will provide one"
    const int64_t per = (spatial ? tiles_per_sample<128, true>(p) : tiles_per_sample<128, false>(p)) / p.ncls;
    int best, cper;
    f32_split(p, per, best, cper);
    if (best <= 1) return 0;
    return (int64_t)best * p.B * p.Ho * p.Wo * (p.y_cstride ? p.y_cstride : p.Cout);
}

extern "C" int e4s_conv_mfma_f32(const e4s_conv_params* pp, int spatial, void* stream) {
    const e4s_conv_params& p = *pp;
    hipStream_t st = as_stream(stream);
    if (p.Cin % KC || p.Cout % 32 || (p.ntaps != 9 && p.ntaps != 1 && p.ntaps != 25) || (p.ncls != 1 && p.ncls != 4))
        return (int)hipErrorInvalidValue;
    if (p.ntaps == 25 && (spatial || p.ncls != 1)) return (int)hipErrorInvalidValue;   // 5x5: per-tap gather mode only
    if (p.Hi >= 32767 || p.Wi >= 32767) return (int)hipErrorInvalidValue;
    if (p.tap_shift && (spatial || p.tap_shift != 1)) return (int)hipErrorInvalidValue;
    if (spatial) {
        if (p.tiles || p.istride != 1 || p.ntaps != 9) return (int)hipErrorInvalidValue;
        if (p.labels && (p.groups_per_batch < 1 || p.groups_per_batch > 16)) return (int)hipErrorInvalidValue;
        const int64_t mt = (int64_t)p.B * ((p.Ha + 7) / 8) * ((p.Wa + 15) / 16) * p.ncls;
        const int bn = pick_bn(p, mt);
        if (bn == 128) return launch<128, 128, 2, 2, true>(p, st);
        // deeper register prefetch only where few blocks are resident (batch 1 / low resolutions): on big grids its
        // extra VGPRs cost more occupancy than the latency it hides (measured: -6 % at 16k+ blocks, +8 % at 256)
        const bool deep = mt * (p.Cout / bn) < 2048;
        if (bn == 64) return deep ? launch<128, 64, 2, 2, true, 2>(p, st) : launch<128, 64, 2, 2, true, 1>(p, st);
        return deep ? launch<128, 32, 4, 1, true, 2>(p, st) : launch<128, 32, 4, 1, true, 1>(p, st);
    }
    if (p.labels) return (int)hipErrorInvalidValue;     // per-row regions exist only in spatial mode
    const int64_t mt = p.tiles ? p.tiles_cap : ((int64_t)p.B * p.Ha * p.Wa + 127) / 128 * p.ncls;
    const int bn = pick_bn(p, mt);
    if (bn == 128) return launch<128, 128, 2, 2, false>(p, st);
    const bool deep = mt * (p.Cout / bn) < 2048;
    if (bn == 64) return deep ? launch<128, 64, 2, 2, false, 2>(p, st) : launch<128, 64, 2, 2, false, 1>(p, st);
    return deep ? launch<128, 32, 4, 1, false, 2>(p, st) : launch<128, 32, 4, 1, false, 1>(p, st);
}
