// The strided gather conv (conv_bf16x3.hip: conv_bf16x3_gather_kernel -- stride-2 3x3 and 1x1 convs, one stage = one tap x 32 input channels,
// tile 256 pixels x 128 channels in natural pixel order) re-cut for ONE wave per SIMD.
//
// conv_bf16x3_gather_kernel: 8 waves of 64 x 64, two per SIMD: per stage every wave reads 16 ds_read_b128 (8 A, 8 B) for 24 MFMAs -- 128 KB of
// fragment reads per CU and stage beside 48 KB of staging stores, ~1 375 LDS-port cycles under 1 536 matrix-pipe cycles.  Here a 256-thread
// block owns the whole register file: 2 x 2 waves of 128 rows x 64 channels = 8 accumulator tiles (128 registers) per wave, 48 MFMAs per wave
// and stage.
//   * B (weights) does NOT go through the LDS: a wave needs only its own 64 channels, so it loads them straight into its B fragment registers
//     from a fragment-major image (gather_frag_kernel: 1 KB contiguous per instruction, ordered (chunk, tap, 32-column block, k-step, hi | lo)),
//     a whole stage ahead (two register sets).  The two waves of a column pair read the same lines.
//   * A: the same per-tap gather of 256 rows x 32 channels (four 8-channel items per thread now), fetched into registers TWO stages ahead
//     (two register sets: a set is split and stored while the other is in flight), split to hi | lo bf16 and stored into a double-buffered LDS
//     stage of 144-byte rows -- the ds_read_b128 fragment reads (lane -> row, lane half -> +16 B) are conflict free: a 16-lane service group
//     ({0-3, 12-15, 20-27}, ...) covers sixteen different rows mod 16, and 9 r mod 16 is a bijection on the 16-byte slots of a bank row.
//   * ONE barrier per stage, after the seventh of the eight MFMA groups: the last fragment reads of this stage's buffer are issued before it,
//     all staging stores of the next stage's buffer too; the first group of the next stage is read behind it, under the eighth group's MFMAs.
//   * Every MFMA slot carries at most one fragment read or one global load and one PIECE of the staging (two channels' hi or lo split, or a
//     store), sched_barrier(0) per slot: with one wave per SIMD nothing else covers a long gap (conv_wino1w.hip).
// Order of additions per accumulator = the 8-wave kernel's: stages in (chunk, tap) order, k-step 0 then 1, lo x hi, hi x lo, hi x hi -- the conv
// output is the same bits.  The fused statistics add two wave rows where the 8-wave kernel adds four (a slot may differ in the last fp64 bit).
#include "conv_launch.h"
#include "gather1w_rows.h"
#include <stdlib.h>
#include <type_traits>

namespace {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int NTHR = 256, BM = 256, BN = 128, KC = 32;
constexpr int ROWB = e4s_gather1w::kRowBytes, LO = e4s_gather1w::kLo;      // LDS row [32 hi bf16 | 32 lo bf16 | 16 pad]: gather1w_rows.h
constexpr int WM = 2, WN = 2, TM = 4, TN = 2;              // 2 x 2 waves of 128 rows x 64 channels
constexpr int A_BYTES = BM * ROWB;
constexpr int SMEM_1W = 2 * A_BYTES + BM * 4;
constexpr int FRAG = 1024;                                 // one wave instruction of the fragment-major image
static_assert(WM * TM * 32 == BM && WN * TN * 32 == BN && WM * WN * 64 == NTHR, "wave layout");

struct AF { bf16x8 h, l; };                                // one 32-row group, one k-step
struct BS { bf16x8 h[2][TN], l[2][TN]; };                  // a stage: [k-step][32-column block]
struct PS { f32x4 v[4][2]; unsigned ok; };                 // the four 8-channel items of a stage, and which of them are not padding

// VAR: profiling variants (builds with -DE4S_ABLATIONS select them with env E4S_GATHER_1W_VAR; results are WRONG for VAR >= 1; product builds
// only instantiate VAR = 0): 1 no A staging (no fetch, split or store), 2 no weight loads, 3 MFMAs only (no fragment reads, no barrier)
template <int VAR = 0>
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(1, 1)))
void conv_gather1w_kernel(const e4s_conv_params p, const int ntn, const int npix, const int ntile, const int ksplit, const int cper) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sA = smem;                              // [2][BM][ROWB]
    int* s_out = reinterpret_cast<int*>(smem + 2 * A_BYTES);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int ks = logical / ntile, tile = logical - ks * ntile;          // K split major, as the 8-wave kernel
    const int mt = tile / ntn, nt = tile - mt * ntn;
    const int n0 = nt * BN;
    const int hw = p.Ha * p.Wa;
    const int c_lo = ks * cper, c_hi = min(p.Cin / KC, c_lo + cper);

    {
        const int a = mt * BM + tid;
        s_out[tid] = a < npix ? a : -1;                    // ostride == 1: the output pixel index IS the anchor index
    }
    // A staging role: rows ar0 + 64 j (j < 4), 8-channel group aq.  Offsets are unsigned BYTES from p.x (the launcher keeps x under 4 GB)
    // (the rows are dealt against ds_write_b128 bank conflicts: gather1w_rows.h)
    const int aq = tid & 3, ar0 = e4s_gather1w::stage_row(tid >> 2);
    unsigned a_off[4];
    int a_y[4], a_x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int a = mt * BM + ar0 + 64 * j;
        const bool valid = a < npix;
        const int aa = valid ? a : 0;
        const int b = aa / hw, rem = aa - b * hw;
        const int ay = rem / p.Wa, ax = rem - ay * p.Wa;
        const int by = ay * p.istride, bx = ax * p.istride;
        a_off[j] = ((unsigned)((b * p.Hi + by) * p.Wi + bx) * (unsigned)p.Cin + (unsigned)aq * 8u) * 4u;
        a_y[j] = valid ? by : 0x7fff;                      // rows past the launch: every tap is "padding"
        a_x[j] = valid ? bx : 0x7fff;
    }
    const int ntaps = p.ntaps, nstage = ntaps * (c_hi - c_lo);
    const unsigned char* xb = reinterpret_cast<const unsigned char*>(p.x);
    const unsigned char* wf = reinterpret_cast<const unsigned char*>(p.w_frag) + (size_t)lane * 16;
    const int nb32 = p.Cout / 32, cb0 = n0 / 32 + wn * TN;

    // stages run in the 8-wave kernel's order, tap fastest.  (tap, chunk) of a stage advance by one stage without a division or a branch; past the
    // last stage the chunk wraps to the first one: harmless loads of a valid stage, never used
    struct Stg { int tap, chunk; };
    auto next_stage = [&](Stg t) -> Stg {
        const bool wrap = t.tap + 1 == ntaps;
        const int c = t.chunk + (wrap ? 1 : 0);
        return Stg{wrap ? 0 : t.tap + 1, c == c_hi ? c_lo : c};
    };
    auto b_src = [&](Stg t) -> const unsigned char* { return wf + ((size_t)(t.chunk * ntaps + t.tap) * nb32 + cb0) * (4 * FRAG); };
    auto ldB = [&](BS& B, const unsigned char* src, int i) {          // i < 8, in the order of use: k-step, hi | lo, column block
        const int kk = i >> 2, hl = (i >> 1) & 1, tn = i & 1;
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + tn * (4 * FRAG) + kk * (2 * FRAG) + hl * FRAG);
        if (hl) B.l[kk][tn] = v; else B.h[kk][tn] = v;
    };
    // where item j of a stage comes from: the tap's offset from the anchor pixel, or (padding) the chunk's first channels of pixel 0
    struct Tap { int oy, ox, toff; unsigned fb; };
    const int m9 = ntaps == 9 ? 1 : 0;
    auto tap_of = [&](Stg t) -> Tap {
        const int ty = (t.tap * 11) >> 5, tx = t.tap - 3 * ty;            // tap / 3, tap % 3 for tap < 9
        Tap T;
        T.oy = m9 * (ty - 1) + p.tap_shift;
        T.ox = m9 * (tx - 1) + p.tap_shift;
        T.toff = ((T.oy * p.Wi + T.ox) * p.Cin + t.chunk * KC) * 4;
        T.fb = (unsigned)(t.chunk * KC + aq * 8) * 4u;
        return T;
    };
    auto item_addr = [&](const Tap& T, int j, unsigned& off, bool& ok) {
        const int iy = a_y[j] + T.oy, ix = a_x[j] + T.ox;
        ok = (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
        off = ok ? a_off[j] + (unsigned)T.toff : T.fb;
    };
    auto item_load = [&](PS& P, int j, unsigned off) {
        P.v[j][0] = *reinterpret_cast<const f32x4*>(xb + off);
        P.v[j][1] = *reinterpret_cast<const f32x4*>(xb + off + 16);
    };
    auto fetch_all = [&](PS& P, Stg t) {
        const Tap T = tap_of(t);
        P.ok = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned off;
            bool ok;
            item_addr(T, j, off, ok);
            item_load(P, j, off);
            P.ok |= (ok ? 1u : 0u) << j;
        }
    };
    // channels 2 pr, 2 pr + 1 of an item split to hi / lo bf16 in two steps (a slot each in the K loop): v = hi + lo, hi = rne_bf16(v),
    // lo = rne_bf16(v - hi) -- split_store's arithmetic (conv_bf16x3.hip)
    auto split_hi = [&](float v0, float v1, unsigned& hi, float& h0, float& h1) {
        hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v0, v1}, bf16x2));
        h0 = __builtin_bit_cast(float, hi << 16);
        h1 = __builtin_bit_cast(float, hi & 0xffff0000u);
    };
    auto split_lo = [&](float v0, float v1, float h0, float h1, unsigned& lo) {
        lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v0 - h0, v1 - h1}, bf16x2));
    };
    const int a_dst = e4s_gather1w::stage_dst(ar0, aq);

    int arow[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) arow[tm] = e4s_gather1w::frag_src(wm * TM + tm, lane, 0);
    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;
    // the accumulators live in AGPRs: without an "a" operand in the function hipcc selects the MFMAs' VGPR form, and the 128 accumulators + two
    // weight sets + two item sets do not fit 256 VGPRs -- it then copied all 128 between the files on every trip of the K loop
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) asm volatile("" : "+a"(acc[tm][tn]));

    // ---- prologue: items of stages 0 and 1, B fragments of stage 0; stage 0 split and stored; the fragments of its first group ----
    PS P[2];
    BS B[2];
    AF Af[2];
    const Stg st0 = {0, c_lo};
    Stg st1 = next_stage(st0);               // stage s + 1, s + 2 of the K loop
    Stg st2 = next_stage(st1);
    fetch_all(P[0], st0);
    {
        const unsigned char* b0 = b_src(st0);
#pragma unroll
        for (int i = 0; i < 8; ++i) ldB(B[0], b0, i);
    }
    fetch_all(P[1], st1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        u32x4 h, l;
#pragma unroll
        for (int pr = 0; pr < 4; ++pr) {
            const bool ok = (P[0].ok >> j) & 1u;
            const float v0 = ok ? P[0].v[j][pr >> 1][(pr & 1) * 2] : 0.f, v1 = ok ? P[0].v[j][pr >> 1][(pr & 1) * 2 + 1] : 0.f;
            unsigned hh, ll;
            float h0, h1;
            split_hi(v0, v1, hh, h0, h1);
            split_lo(v0, v1, h0, h1, ll);
            h[pr] = hh;
            l[pr] = ll;
        }
        *reinterpret_cast<u32x4*>(sA + a_dst + 64 * j * ROWB) = h;
        *reinterpret_cast<u32x4*>(sA + a_dst + 64 * j * ROWB + LO) = l;
    }
    __syncthreads();
    Af[0].l = *reinterpret_cast<const bf16x8*>(sA + arow[0] + LO);
    Af[0].h = *reinterpret_cast<const bf16x8*>(sA + arow[0]);

    // ---- one stage: 8 groups (k-step, 32-row group) of 6 MFMAs = 48 slots.  Per slot, behind its MFMA:
    //   j 0, 1 of every group      the lo / hi A fragment of the NEXT group (group 7: of the next stage's first group, behind the barrier)
    //   j 2, 3 of groups 0..3      one B fragment of stage s + 1 (a stage of flight)
    //   j 4, 5 of groups 0..3      item g of stage s + 2: its address, then its two loads (more than a stage of flight)
    //   slots 0..39                the items of stage s + 1, ten slots each: four x (hi step, lo step) of a channel pair, then the two stores
    // barrier after slot 41.  Q = s & 1: the LDS buffer and the B set of this stage; the item set being fetched (the other one is being stored) ----
    unsigned hw4[4], lw4[4];
    float v0 = 0.f, v1 = 0.f, h0 = 0.f, h1 = 0.f;
    bool okj = false;
    auto stage = [&](auto q_c) {
        constexpr int Q = decltype(q_c)::value;
        const unsigned char* Ab = sA + Q * A_BYTES;
        unsigned char* An = sA + (Q ^ 1) * A_BYTES;
        const BS& Bc = B[Q];
        BS& Bn = B[Q ^ 1];
        PS& Pf = P[Q];                     // fetched now: stage s + 2
        const PS& Pc = P[Q ^ 1];           // split and stored now: stage s + 1
        const unsigned char* bn = b_src(st1);
        const Tap T2 = tap_of(st2);
        st1 = st2;
        st2 = next_stage(st2);
        unsigned foff = 0, okn = 0;
#pragma unroll
        for (int k = 0; k < 48; ++k) {
            const int g = k / 6, j = k % 6, kk = g >> 2, tm = g & 3, tn = j & 1, prod = j >> 1;
            const AF& Ac = Af[g & 1];
            AF& Ax = Af[(g + 1) & 1];
            acc[tm][tn] = prod == 0 ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ac.l, Bc.h[kk][tn], acc[tm][tn], 0, 0, 0)
                        : prod == 1 ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ac.h, Bc.l[kk][tn], acc[tm][tn], 0, 0, 0)
                                    : __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ac.h, Bc.h[kk][tn], acc[tm][tn], 0, 0, 0);
            if (j < 2) {
                if (VAR == 3) {
                    if (j == 0) Ax = Ac;
                } else {
                    const int ng = (g + 1) & 7;
                    const unsigned char* a = (g < 7 ? Ab : An) + arow[ng & 3] + (ng >> 2) * 32;
                    if (j == 0) Ax.l = *reinterpret_cast<const bf16x8*>(a + LO);
                    else Ax.h = *reinterpret_cast<const bf16x8*>(a);
                }
            }
            if (VAR == 0 || VAR == 1) {
                if (g < 4 && (j == 2 || j == 3)) ldB(Bn, bn, g * 2 + j - 2);
            }
            if (VAR == 0 || VAR == 2) {
                if (g < 4 && j == 4) {
                    bool ok;
                    item_addr(T2, g, foff, ok);
                    okn |= (ok ? 1u : 0u) << g;
                    if (g == 3) Pf.ok = okn;
                }
                if (g < 4 && j == 5) item_load(Pf, g, foff);
                if (k < 40) {
                    const int it = k / 10, r = k % 10, pr = r >> 1;
                    if (r == 0) okj = (Pc.ok >> it) & 1u;
                    if (r < 8 && (r & 1) == 0) {
                        v0 = okj ? Pc.v[it][pr >> 1][(pr & 1) * 2] : 0.f;
                        v1 = okj ? Pc.v[it][pr >> 1][(pr & 1) * 2 + 1] : 0.f;
                        split_hi(v0, v1, hw4[pr], h0, h1);
                    }
                    if (r < 8 && (r & 1) == 1) split_lo(v0, v1, h0, h1, lw4[pr]);
                    if (r == 8) *reinterpret_cast<u32x4*>(An + a_dst + 64 * it * ROWB) = u32x4{hw4[0], hw4[1], hw4[2], hw4[3]};
                    if (r == 9) *reinterpret_cast<u32x4*>(An + a_dst + 64 * it * ROWB + LO) = u32x4{lw4[0], lw4[1], lw4[2], lw4[3]};
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (k == 41 && VAR != 3) {
                lds_barrier();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    for (int s = 0; s < nstage; s += 2) {
        stage(std::integral_constant<int, 0>{});
        if (s + 1 < nstage) stage(std::integral_constant<int, 1>{});
    }

    // ---- epilogue: bias, activation, NHWC store (K split: the raw sums to this split's slab, same layout as y) ----
    const bool raw = ksplit > 1;
    float bsv[TN], slp[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int col = n0 + (wn * TN + tn) * 32 + li;
        bsv[tn] = (p.bias && !raw) ? p.bias[col] : 0.f;
        slp[tn] = (p.act == 2 && !raw) ? p.slope[col] : p.alpha;
    }
    const float gain = (p.act == 1) ? p.gain : 1.f;
    const bool do_act = p.act != 0 && !raw;
    const bool stats = p.stats_ws != nullptr;         // the launcher guarantees tiles that do not straddle samples (and no K split)
    double st_s[TN], st_q[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) st_s[tn] = st_q[tn] = 0.0;
    const int gycs = p.y_cstride ? p.y_cstride : p.Cout;        // a multiple of 4 (launcher)
    float* const yout = raw ? p.splitk_ws + (size_t)ks * ((size_t)npix * gycs) : p.y;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float v[TN][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * g + i;
                const bool live = s_out[(wm * TM + tm) * 32 + i + 8 * g + 4 * kh] >= 0;
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    float t = acc[tm][tn][r] + bsv[tn];
                    if (do_act) t = (t > 0.f ? t : t * slp[tn]) * gain;
                    v[tn][i] = t;
                    if (stats && live) { st_s[tn] += (double)t; st_q[tn] += (double)t * (double)t; }
                }
            }
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) quad_transpose4(v[tn][0], v[tn][1], v[tn][2], v[tn][3], li);
            const int off = s_out[(wm * TM + tm) * 32 + (li & 3) + 8 * g + 4 * kh];
            if (off >= 0) {
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    *reinterpret_cast<f32x4*>(yout + (size_t)off * gycs + n0 + (wn * TN + tn) * 32 + (li & ~3)) =
                        f32x4{v[tn][0], v[tn][1], v[tn][2], v[tn][3]};
            }
        }
    }
    if (stats) {
        // per-thread fp64 sums -> the two k-halves of a lane pair -> the two wave rows in fixed order through LDS: one slot per (image, channel, tile)
        double* s_st = reinterpret_cast<double*>(sA);
        __syncthreads();                                     // every wave is past its last fragment read: A is free
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            st_s[tn] += __shfl_xor(st_s[tn], 32, 64);
            st_q[tn] += __shfl_xor(st_q[tn], 32, 64);
            if (kh == 0) {
                const int col = (wn * TN + tn) * 32 + li;
                s_st[(wm * BN + col) * 2] = st_s[tn];
                s_st[(wm * BN + col) * 2 + 1] = st_q[tn];
            }
        }
        __syncthreads();
        if (tid < BN) {
            double a = 0.0, q = 0.0;
#pragma unroll
            for (int j = 0; j < WM; ++j) { a += s_st[(j * BN + tid) * 2]; q += s_st[(j * BN + tid) * 2 + 1]; }
            const int tiles_per_img = hw / BM;
            const int b = mt / tiles_per_img, tile_in_img = mt - b * tiles_per_img;
            double* slot = p.stats_ws + (((size_t)b * p.Cout + n0 + tid) * p.stats_slots + tile_in_img) * 2;
            slot[0] = a;
            slot[1] = q;
        }
    }
}

// tap-packed fp32 weights [ntaps][Cout][Cin] -> the fragment-major split image: per (chunk of 32 channels, tap, 32-column block, k-step of 16
// channels) [hi: lane l -> column l & 31, channels 8 (l >> 5) .. + 7 | lo: the same], 1 KB each; the values of split_bf16x2_kernel
__global__ void gather_frag_kernel(const float* __restrict__ w, unsigned char* __restrict__ out, int64_t n8, int ntaps, int cout, int cin) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // one 8-channel group of one (tap, column)
    if (i >= n8) return;
    const int g8 = cin / 8;
    const int64_t row = i / g8;
    const int c = (int)(i - row * g8) * 8;
    const int tap = (int)(row / cout), co = (int)(row - (int64_t)tap * cout);
    const f32x4 a = *reinterpret_cast<const f32x4*>(w + row * cin + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(w + row * cin + c + 4);
    const f32x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    const bf16x8 h = __builtin_convertvector(v, bf16x8);
    const f32x8 r = v - __builtin_convertvector(h, f32x8);
    const bf16x8 l = __builtin_convertvector(r, bf16x8);
    const int chunk = c / KC, kk = (c % KC) / 16, half = (c % 16) / 8;
    unsigned char* d = out + ((((size_t)chunk * ntaps + tap) * (cout / 32) + co / 32) * 2 + kk) * (size_t)(2 * FRAG) + (half * 32 + co % 32) * 16;
    *reinterpret_cast<bf16x8*>(d) = h;
    *reinterpret_cast<bf16x8*>(d + FRAG) = l;
}

// E4S_GATHER_1W=0: every gather launch on the 8-wave kernel (read per launch: one process can run both)
inline bool gather1w_enabled() {
    const char* e = getenv("E4S_GATHER_1W");
    return e ? atoi(e) != 0 : true;
}

}  // namespace

// launches the one-wave-per-SIMD kernel takes: the fragment-major image is there, whole 128-column tiles, 16-byte stores, and an input small enough
// for the kernel's 32-bit byte offsets
bool e4s_gather1w_ok(const e4s_conv_params& p) {
    const int ycs = p.y_cstride ? p.y_cstride : p.Cout;
    return p.w_frag && p.Cout % BN == 0 && (ycs & 3) == 0 && (int64_t)p.B * p.Hi * p.Wi * p.Cin * 4 < (1ll << 32) && gather1w_enabled();
}

int e4s_launch_gather1w(const e4s_conv_params& p, const e4s_gather_plan& g, hipStream_t st) {
    const dim3 grid((unsigned)(g.ntile * g.ksplit));
#ifdef E4S_ABLATIONS
    {
        const char* ev = getenv("E4S_GATHER_1W_VAR");
        int e;
#define GV(V) case V: if ((e = (int)hipFuncSetAttribute((const void*)conv_gather1w_kernel<V>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_1W))) return e; \
              hipLaunchKernelGGL((conv_gather1w_kernel<V>), grid, dim3(NTHR), SMEM_1W, st, p, g.ntn, (int)g.npix, (int)g.ntile, g.ksplit, g.cper); \
              E4S_CHECK_LAUNCH(); return 0;
        switch (ev ? atoi(ev) : 0) {
            GV(1) GV(2) GV(3)
            default: break;
        }
#undef GV
    }
#endif
    static std::atomic<uint64_t> smem_set{0};
    if (int e = e4s_ensure_dyn_smem(reinterpret_cast<const void*>(conv_gather1w_kernel<0>), SMEM_1W, smem_set)) return e;
    hipLaunchKernelGGL(conv_gather1w_kernel<0>, grid, dim3(NTHR), SMEM_1W, st, p, g.ntn, (int)g.npix, (int)g.ntile, g.ksplit, g.cper);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t e4s_gather_frag_bytes(int ntaps, int cout, int cin) {
    return (cin % KC || cout % 32 || ntaps < 1) ? 0 : (int64_t)ntaps * cout * cin * 4;
}

extern "C" int e4s_gather_frag_bf16x2_f32(const float* w, void* out, int ntaps, int cout, int cin, void* stream) {
    if (cin % KC || cout % 32 || ntaps < 1) return (int)hipErrorInvalidValue;
    const int64_t n8 = (int64_t)ntaps * cout * (cin / 8);
    hipLaunchKernelGGL(gather_frag_kernel, dim3(cdiv(n8, 256)), dim3(256), 0, as_stream(stream), w, reinterpret_cast<unsigned char*>(out), n8, ntaps,
                       cout, cin);
    E4S_CHECK_LAUNCH();
    return 0;
}
