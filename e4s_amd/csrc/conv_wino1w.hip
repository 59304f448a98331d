// Winograd F(2,3)-along-the-rows 3x3 convolution (conv_wino.hip: algebra, V layout, epilogue forms), re-cut for ONE wave per SIMD
// (round 6; the encoder's stride-1 convs are 43 % of a face swap's GPU time).
//
// conv_wino_kernel: 8 waves of 64 rows x 32 channels x 4 positions, two per SIMD inside 256 registers: 24 ds_read_b128 per 24 MFMAs, a
// barrier every 24 MFMAs per wave, the weights by LDS-DMA, the input transform on three "storer" waves per stage.  Here a 256-thread block
// owns the whole 512-entry register file: wave w holds ALL 128 GEMM rows x channels 32 w .. 32 w + 31 x four positions = 16 accumulator
// tiles (256 AGPRs); a stage (one vertical tap x 16 channels) is 48 MFMAs per wave; the output transform still happens in registers and the
// block tile (128 GEMM rows x 128 channels x 4 positions) is unchanged.
//   * U (weights) does NOT go through the LDS: a wave needs only its own 32 channels, so it loads them straight into its B fragment
//     registers from a fragment-major image (1 KB contiguous per instruction), position p of the NEXT stage behind the MFMAs of position p
//     of this one.  History: LDS-DMA into a ring of planes with vmcnt(0) before the barrier: 23 % SLOWER than the 8-wave kernel (a DMA
//     needs ~1.1 us from issue to landed); register-staged ring (load -> ds_write_b128 -> ds_read_b128): -6 % -- the LDS write port, ~79
//     B/clk per CU, was 415 of the 1 070 LDS cycles of a stage; direct: see profiles/r06_wino1w.json.
//   * V (transformed input) in LDS, double buffered by chunk, ONE barrier per stage after position 1; the A fragments of position p + 1 (of
//     the next stage after position 3) are read under the MFMAs of position p; every wave reads the whole V tile (the same LDS read
//     traffic as A + B fragments of a 64 x 64 wave tile).
//   * Input transform: 576 items (V-pixel, 4 channels) per chunk = two per thread (A, B) + 64 left over, which are cut into their four
//     positions so that every thread takes one quarter (Q: wave w computes position w).  Addresses are a per-thread constant + a
//     wave-uniform tile / chunk base, padding is two flag words: no integer multiplies, no branches, no 64-bit vector arithmetic.
//   * The issue order is pinned slot by slot (one MFMA + an A fragment read or a B fragment load + one PIECE of the input transform,
//     sched_barrier(0)).  One wave per SIMD means nothing else covers a long MFMA gap (a gap runs max(32, sum of issue costs) cycles, a VALU
//     instruction costs 4), so the transform is cut into pieces of <= 5 VALU -- one channel of one position, one step of a hi / lo split,
//     half of a padded pixel's fill, one fetch -- and spread over the chunk's 144 slots: the table is in stage() below;
//     tools/mfma_gap_report.py prints what the compiler made of it (profiles/r10_wino1w_gaps.txt: the largest gap went from 32 VALU to 6,
//     the modelled overrun from 17 % to 0.5 %; measured -9 ... -12 % per launch in the step).
// Split-K launches (<= 128 tiles) and short-K layers stay on conv_wino_kernel.
#include "conv_launch.h"
#include "rows64.h"
#include <stdlib.h>
#include <type_traits>

namespace {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int NTHR = 256;
constexpr int TH = 16, TW = 16, NPAIR = TW / 2;
constexpr int VROWS = (TH + 2) * NPAIR;          // 144 V-pixels per position and chunk
constexpr int BN = 128;
using rows64::KC;
using rows64::ROWB;
using rows64::swz;          // 64-byte swizzled rows [16 hi | 16 lo]
constexpr int A_PLANE = VROWS * ROWB, A_BYTES = 4 * A_PLANE;        // 36 864
constexpr int OFF_IN = 2 * A_BYTES;                                 // XF == 2: float [2 tile parities][Cin][{mean, rstd}]
constexpr int SMEM_1W = OFF_IN;
#ifndef E4S_WINO_BPF
#define E4S_WINO_BPF 1
#endif
// B fragments are fetched this many stages ahead.  2 (three register sets) measured SLOWER in the step, same box, two alternations:
// encoder convs 6.95 vs 6.85 ms, step 16.40 vs 16.31 ms (profiles/r06_wino1w.json) -- one stage of flight covers the weight stream
constexpr int BPF = E4S_WINO_BPF;
static_assert(BPF == 1 || BPF == 2, "B prefetch distance");

struct WTile {
    int n0, tb, ty0, tx0, slot;
};

struct AF { bf16x8 h[4], l[4]; };          // the four 32-row groups of a position
struct BF { bf16x8 h, l; };                // one position of this wave's 32 channels

// v = (a - m) + sg (b - m) [m = 0, sg = -1: a - b exactly; m = mean, sg = +1: position 1 of the InstanceNorm form], * rs: one channel of a quarter item
template <int XF>
__device__ __forceinline__ float quarter_v(const float a, const float b, const float m, const float sg, const float r) {
    const float v = __builtin_fmaf(sg, b - m, a - m);
    return XF == 2 ? v * r : v;
}

// XF: 0 plain input, 2 InstanceNorm (x - mean) * rstd folded into the input transform (zero padding applies to the NORMALISED map)
// VAR: profiling variants (builds with -DE4S_ABLATIONS select them with env E4S_WINO_1W_VAR; results are WRONG for VAR >= 1; product builds
// only instantiate VAR = 0): 1 no weight staging, 2 no input-transform staging, 3 neither, 4 MFMAs only (no fragment reads, no barrier)
template <int XF, int VAR = 0>
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(1, 1)))
void conv_wino1w_kernel(const e4s_conv_params p, const int ntn, const int tx_n, const int per_img, const int ntiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sA = smem;                                  // [2][4 pos][144][64]
    float* s_in = reinterpret_cast<float*>(smem + OFF_IN);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kh = lane >> 5;
    const int wn = wave;                                       // this wave: all 128 GEMM rows x channels 32 wn .. 32 wn + 31, four positions
    const int G = gridDim.x;
    const int first = xcd_remap(blockIdx.x, G);
    const int mtiles = ntiles / ntn;
    const int nchunk = p.Cin / KC;
    const unsigned char* ub = reinterpret_cast<const unsigned char*>(p.w);
    // n-major tile order: consecutive ids (one XCD) share a column tile, i.e. one slab of U in their L2
    auto decode = [&](int t) -> WTile {
        WTile w;
        const int nt = t / mtiles, mt = t - nt * mtiles;
        w.n0 = nt * BN;
        w.tb = mt / per_img;
        w.slot = mt - w.tb * per_img;
        const int tyb = w.slot / tx_n;
        w.ty0 = tyb * TH;
        w.tx0 = (w.slot - tyb * tx_n) * TW;
        return w;
    };

    // ---- input-transform items.  Item it = (V-pixel v = it >> 2 [row hy = v >> 3 of 18, pair j = v & 7], channels 4 (it & 3) .. + 3) reads the
    // pixels d_i = x[ty0 + hy - 1][tx0 + 2 j - 1 + i], i < 4.  Per thread and class (A: it = tid, B: tid + 256, Q: 512 + lane) the element
    // offset relative to the tile's (ty0, tx0, chunk) origin and the edge flags {hy == 0, hy == 17, j == 0, j == 7} are constants. ----
    // Offsets are unsigned BYTES from the pixel one row up and one to the left of the tile origin (the smallest address an item reads), so a load
    // is a wave-uniform 64-bit base + a 32-bit per-lane offset: no 64-bit vector arithmetic in the K loop.
    const int cq = tid & 3;
    const unsigned cin4 = (unsigned)p.Cin * 4u, fb_off = (unsigned)((p.Wi + 1) * p.Cin + cq * 4) * 4u;      // fb_off: the tile's first own pixel
    auto rel_of = [&](int v) -> unsigned { return (unsigned)(((v >> 3) * p.Wi + 2 * (v & 7)) * p.Cin + cq * 4) * 4u; };
    auto flg_of = [&](int v) -> unsigned { return ((v >> 3) == 0 ? 1u : 0u) | ((v >> 3) == 17 ? 2u : 0u) | ((v & 7) == 0 ? 4u : 0u) | ((v & 7) == 7 ? 8u : 0u); };
    auto dst_of = [&](int v) -> int { return swz(v, cq >> 1) + (cq & 1) * 8; };
    const int vA = tid >> 2, vB = 64 + (tid >> 2), vQ = 128 + (lane >> 2);
    const unsigned relA = rel_of(vA), relB = rel_of(vB), relQ = rel_of(vQ);
    const unsigned flgA = flg_of(vA), flgB = flg_of(vB), flgQ = flg_of(vQ);
    const int dstA = dst_of(vA), dstB = dst_of(vB), dstQ = dst_of(vQ) + wave * A_PLANE;      // Q: this wave's position plane
    // quarter items: position = wave: V0 = d0 - d2, V1 = d1 + d2, V2 = d2 - d1, V3 = d1 - d3
    const int qa = wave == 0 ? 0 : (wave == 2 ? 2 : 1), qb = wave == 0 ? 2 : (wave == 1 ? 2 : (wave == 2 ? 1 : 3));
    const float qsg = wave == 1 ? 1.f : -1.f;
    // tile edge bits {top, bottom, left, right} and the element offset of a tile's (chunk) origin
    auto edge_of = [&](const WTile& T) -> unsigned {
        return (T.ty0 == 0 ? 1u : 0u) | (T.ty0 + TH == p.Hi ? 2u : 0u) | (T.tx0 == 0 ? 4u : 0u) | (T.tx0 + TW == p.Wi ? 8u : 0u);
    };
    auto xbase_of = [&](const WTile& T, int chunk) -> const unsigned char* {
        return reinterpret_cast<const unsigned char*>(p.x + (size_t)T.tb * p.Hi * p.Wi * p.Cin + ((size_t)T.ty0 * p.Wi + T.tx0) * p.Cin + chunk * KC) -
               (size_t)(p.Wi + 1) * p.Cin * 4;
    };
    // pixel i of an item: valid unless its row is padding (flags 1 | 2) or it is the left-most / right-most pixel of a border pair.  One mask
    // test (a short-circuit would put branches into the K loop); `bad` = the item's flags & the tile's edge bits.  The test is two VALU, so the
    // fill repeats it instead of keeping ten lane masks alive from the fetch to the fill
    auto px_ok = [&](unsigned flg, unsigned edge, int i) -> bool { return (flg & (edge & (3u | (i == 0 ? 4u : 0u) | (i == 3 ? 8u : 0u)))) == 0u; };
    auto load_px = [&](const unsigned char* xb, unsigned rel, unsigned flg, unsigned edge, int i) -> f32x4 {
        return *reinterpret_cast<const f32x4*>(xb + (px_ok(flg, edge, i) ? rel + (unsigned)i * cin4 : fb_off));
    };
    struct Item {
        f32x4 d[4];
    };
    // {mean, rstd} of the thread's four channels (XF == 2); padded pixels -> 0 of the NORMALISED map, i.e. the mean
    auto stats_half = [&](f32x4& mu, f32x4& rs, int chunk, int par, int h) {          // channels 2 h, 2 h + 1 of the thread's four
        if (XF == 2) {
            const f32x4 s = *reinterpret_cast<const f32x4*>(s_in + par * p.Cin * 2 + (chunk * KC + cq * 4) * 2 + 4 * h);
            mu[2 * h] = s[0];
            rs[2 * h] = s[1];
            mu[2 * h + 1] = s[2];
            rs[2 * h + 1] = s[3];
        }
    };
    auto stats_of = [&](f32x4& mu, f32x4& rs, int chunk, int par) {
        stats_half(mu, rs, chunk, par, 0);
        stats_half(mu, rs, chunk, par, 1);
    };
    // channels 2 h, 2 h + 1 of a padded pixel <- 0 of the (normalised) map
    auto fill_half = [&](f32x4& d, const f32x4& mu, unsigned flg, unsigned edge, int i, int h) {
        const bool ok = px_ok(flg, edge, i);
        d[2 * h] = ok ? d[2 * h] : (XF == 2 ? mu[2 * h] : 0.f);
        d[2 * h + 1] = ok ? d[2 * h + 1] : (XF == 2 ? mu[2 * h + 1] : 0.f);
    };
    // position ps (compile time) of an item, channel c: V0 = d0 - d2, V1 = d1 + d2, V2 = d2 - d1, V3 = d1 - d3 (the mean cancels in the
    // differences; V1 of the InstanceNorm form = (d1 - mu) + (d2 - mu)), * rstd
    auto item_v = [&](const Item& I, const f32x4& mu, const f32x4& rs, int ps, int c) -> float {
        float t;
        if (ps == 0) t = I.d[0][c] - I.d[2][c];
        else if (ps == 1) t = XF == 2 ? (I.d[1][c] - mu[c]) + (I.d[2][c] - mu[c]) : I.d[1][c] + I.d[2][c];
        else if (ps == 2) t = I.d[2][c] - I.d[1][c];
        else t = I.d[1][c] - I.d[3][c];
        if (XF == 2) t *= rs[c];
        return t;
    };
    // two channels split to hi / lo bf16, in two steps (a slot each in the K loop): hi and its two values back in fp32; the residuals
    auto split_hi = [&](float v0, float v1, unsigned& hi, float& h0, float& h1) {
        hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v0, v1}, bf16x2));
        h0 = __builtin_bit_cast(float, hi << 16);
        h1 = __builtin_bit_cast(float, hi & 0xffff0000u);
    };
    auto split_lo = [&](float v0, float v1, float h0, float h1, unsigned& lo) {
        lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v0 - h0, v1 - h1}, bf16x2));
    };
    auto item_pair = [&](const Item& I, const f32x4& mu, const f32x4& rs, int ps, int half, unsigned& hi, unsigned& lo) {
        const float v0 = item_v(I, mu, rs, ps, 2 * half), v1 = item_v(I, mu, rs, ps, 2 * half + 1);
        float h0, h1;
        split_hi(v0, v1, hi, h0, h1);
        split_lo(v0, v1, h0, h1, lo);
    };
    auto load_stats = [&](const WTile& T, int par) {
        if (XF == 2) {
            const float* st = p.in_stats + (size_t)T.tb * p.Cin * 2;
            for (int i = tid * 4; i < p.Cin * 2; i += NTHR * 4)
                *reinterpret_cast<f32x4*>(s_in + par * p.Cin * 2 + i) = *reinterpret_cast<const f32x4*>(st + i);
        }
    };

    // ---- weights: straight from global memory into the B fragments of the wave that uses them (no LDS round trip: the LDS write port --
    // ~79 B/clk per CU -- was 415 of the 1 070 LDS cycles of a stage).  The fragment-major image (wino_weights_kernel writes it behind the
    // plane-major one): per (ky, chunk, position, 32-channel block) 2 KB = [hi: lane l -> channel l & 31, k-half l >> 5][lo: the same], so a
    // wave's fragment load is 1 KB contiguous ----
    const unsigned char* uf = ub + (size_t)3 * nchunk * 4 * p.Cout * ROWB;                          // behind the plane-major image
    auto uf_src = [&](int ky, int chunk, int ps, int n0) -> const unsigned char* {
        return uf + ((((size_t)ky * nchunk + chunk) * 4 + ps) * (p.Cout / 32) + (n0 / 32 + wn)) * 2048 + lane * 16;
    };
    if (first >= ntiles) return;
    WTile cur = decode(first);
    int t_next = first + G;
    bool has_next = t_next < ntiles;
    WTile nxt = decode(has_next ? t_next : first);

    // ---- prologue (once per block): V of chunk 0 (three rounds of items, the last one on wave 0 only), items A and Q of chunk 1, the B
    // fragments of stage 0.  EVERY global load is issued before the first wait: the statistics, chunk 0's pixels, the fragments, chunk 1's
    // items, in the order in which they are consumed (vmcnt counts in order) ----
    Item IA, IB;                       // items A and B in flight
    f32x4 Qa, Qb;                      // quarter item in flight: the two pixels of this wave's position
#pragma unroll
    for (int i = 0; i < 4; ++i) IB.d[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // B fragments.  BPF = 1: one set, position p re-filled for the NEXT stage as soon as its MFMAs have issued (a stage of flight); BPF = 2: three
    // sets rotating with the vertical tap, position p of the stage AFTER the next fetched under position p of this one
    BF Bf[BPF == 1 ? 1 : 3][4];
    {
        f32x4 st_r[2];                 // the statistics table: Cin <= 1024 (the launcher refuses more) = at most two rows of four floats per thread
        if (XF == 2) {
            const float* st = p.in_stats + (size_t)cur.tb * p.Cin * 2;
#pragma unroll
            for (int r = 0; r < 2; ++r)
                if ((tid + r * NTHR) * 4 < p.Cin * 2) st_r[r] = *reinterpret_cast<const f32x4*>(st + (tid + r * NTHR) * 4);
        }
        const unsigned char* xb0 = xbase_of(cur, 0);
        const unsigned edge = edge_of(cur);
        Item I0[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int v = (tid + r * NTHR) >> 2;
            if (r < 2 || wave == 0)
#pragma unroll
                for (int i = 0; i < 4; ++i) I0[r].d[i] = load_px(xb0, rel_of(v), flg_of(v), edge, i);
        }
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const unsigned char* b = uf_src(0, 0, ps, cur.n0);
            Bf[0][ps].h = *reinterpret_cast<const bf16x8*>(b);
            Bf[0][ps].l = *reinterpret_cast<const bf16x8*>(b + 1024);
            if constexpr (BPF == 2) {
                const unsigned char* b1 = uf_src(1, 0, ps, cur.n0);
                Bf[BPF - 1][ps].h = *reinterpret_cast<const bf16x8*>(b1);
                Bf[BPF - 1][ps].l = *reinterpret_cast<const bf16x8*>(b1 + 1024);
            }
        }
        const unsigned char* xb1 = xbase_of(cur, 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) IA.d[i] = load_px(xb1, relA, flgA, edge, i);
        Qa = load_px(xb1, relQ, flgQ, edge, qa);
        Qb = load_px(xb1, relQ, flgQ, edge, qb);
        if (XF == 2) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
                if ((tid + r * NTHR) * 4 < p.Cin * 2) *reinterpret_cast<f32x4*>(s_in + (tid + r * NTHR) * 4) = st_r[r];
            __syncthreads();
        }
        f32x4 mu = {0.f, 0.f, 0.f, 0.f}, rs = {1.f, 1.f, 1.f, 1.f};
        stats_of(mu, rs, 0, 0);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int v = (tid + r * NTHR) >> 2;
            if (r < 2 || wave == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    fill_half(I0[r].d[i], mu, flg_of(v), edge, i, 0);
                    fill_half(I0[r].d[i], mu, flg_of(v), edge, i, 1);
                }
#pragma unroll
                for (int ps = 0; ps < 4; ++ps) {
                    unsigned h[2], l[2];
                    item_pair(I0[r], mu, rs, ps, 0, h[0], l[0]);
                    item_pair(I0[r], mu, rs, ps, 1, h[1], l[1]);
                    const int a = ps * A_PLANE + dst_of(v);
                    *reinterpret_cast<u32x2*>(sA + a) = u32x2{h[0], h[1]};
                    *reinterpret_cast<u32x2*>(sA + (a ^ 32)) = u32x2{l[0], l[1]};
                }
            }
        }
    }
    __syncthreads();

    int aoff[4][3];
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) aoff[tm][ky] = swz(tm * 32 + li + 8 * ky, kh);

    f32x16 acc[4][4];                 // [position][32-row group]
    AF Af[2];
    auto ldA = [&](AF& F, const unsigned char* Abuf, int ps, int ky, int part) {      // part: 2 tm + {0: h, 1: l}
        const unsigned char* a = Abuf + ps * A_PLANE;
        const int tm = part >> 1;
        if (part & 1) F.l[tm] = *reinterpret_cast<const bf16x8*>(a + (aoff[tm][ky] ^ 32));
        else F.h[tm] = *reinterpret_cast<const bf16x8*>(a + aoff[tm][ky]);
    };
    // fragments of (stage 0, position 0)
#pragma unroll
    for (int part = 0; part < 8; ++part) ldA(Af[0], sA, 0, 0, part);

    unsigned sg = 0, cg = 0;         // running stage / chunk counters: the LDS buffer parities and the plane ring continue across tiles
    int par = 0;                     // parity of the block's tile counter: s_in[par] holds the current tile's statistics
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, rs = {1.f, 1.f, 1.f, 1.f};
    float tv[2], th[2], qv[4], qth[4];       // pieces of the input transform in flight between slots
    unsigned hh[2], ll[2], qh[2], ql[2];
    for (;;) {
        if (has_next) load_stats(nxt, par ^ 1);      // first read when this tile's last chunk stores the next tile's items: barriers in between
        const unsigned edge_c = edge_of(cur), edge_n = edge_of(nxt);
#pragma unroll
        for (int ps = 0; ps < 4; ++ps)
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ps][tm][r] = 0.f;

        for (int chunk = 0; chunk < nchunk; ++chunk) {
            const bool in_tile = chunk + 1 < nchunk;            // the next chunk belongs to this tile
            const WTile& Tn = in_tile ? cur : nxt;              // owner of the next chunk (past the last tile: a harmless re-read of this one)
            const int c_n = in_tile ? chunk + 1 : 0;
            const int par_n = in_tile ? par : par ^ 1;
            const unsigned char* Ab = sA + (cg & 1) * A_BYTES;
            unsigned char* An = sA + ((cg + 1) & 1) * A_BYTES;
            // the chunk after the next one (its items A and Q are fetched in this chunk's last stage)
            const bool in2 = chunk + 2 < nchunk;
            const WTile& T2 = in2 ? cur : nxt;
            const int c_2 = in2 ? chunk + 2 : (chunk + 2 - nchunk);
            const unsigned edge_nn = in_tile ? edge_c : edge_n, edge_2 = in2 ? edge_c : edge_n;
            const unsigned char* xb_n = xbase_of(Tn, c_n);              // origin of the next chunk (item B)
            const unsigned char* xb_2 = xbase_of(T2, c_2);              // ... and of the one after (items A, Q)
            // (a generic lambda per vertical tap: `#pragma unroll` on a loop over this body is refused by the optimizer, and a runtime ts
            // would index aoff[][] dynamically -- scratch)
            auto stage = [&](auto ts_c) {
                constexpr int ts = decltype(ts_c)::value;
                // the next stage = (chunk, ts + 1) or (next chunk, 0): where its B fragments come from
                // the stage whose B fragments are fetched now: BPF stages ahead = (chunk, ts + BPF) or (next chunk, ts + BPF - 3)
                constexpr int ky1 = (ts + BPF) % 3;
                const int ch1 = ts + BPF < 3 ? chunk : c_n, n01 = ts + BPF < 3 ? cur.n0 : Tn.n0;
                constexpr int bs_cur = BPF == 1 ? 0 : ts, bs_ld = BPF == 1 ? 0 : (ts + 2) % 3;
#pragma unroll
                for (int ps = 0; ps < 4; ++ps) {
                    AF& Ac = Af[ps & 1];
                    AF& Ax = Af[(ps + 1) & 1];
                    const BF Bc = Bf[bs_cur][ps];
                    // next A fragments: position ps + 1 of this stage, or position 0 of the next stage (its V: this chunk's buffer with the next
                    // vertical tap, or the next chunk's)
                    const unsigned char* nA = ps < 3 ? Ab : (ts < 2 ? Ab : An);
                    const int nps = (ps + 1) & 3, nky = ps < 3 ? ts : (ts + 1) % 3;
                    const unsigned char* nb = uf_src(ky1, ch1, ps, n01);
#pragma unroll
                    for (int k = 0; k < 12; ++k) {
                        const int prod = k >> 2, tm = k & 3;
                        acc[ps][tm] = prod == 0 ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ac.h[tm], Bc.l, acc[ps][tm], 0, 0, 0)
                                    : prod == 1 ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ac.l[tm], Bc.h, acc[ps][tm], 0, 0, 0)
                                                : __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ac.h[tm], Bc.h, acc[ps][tm], 0, 0, 0);
                        // slots 0..7: one A fragment read each
                        if (VAR == 4) {
                            if (k == 0) Ax = Ac;
                        } else if (k < 8) ldA(Ax, nA, nps, nky, k);
                        // this position's B fragment for the NEXT stage, behind the sweeps that used the current one last (lo: hi x lo, slots 0..3;
                        // hi: slots 4..11): a whole stage of flight
                        if (VAR == 0 || VAR == 2) {
                            if (k == 8) Bf[bs_ld][ps].l = *reinterpret_cast<const bf16x8*>(nb + 1024);
                            if (k == 11) Bf[bs_ld][ps].h = *reinterpret_cast<const bf16x8*>(nb);
                        }
                        if (VAR == 0 || VAR == 1) {
                            // ---- the input transform, a piece per slot so that no MFMA gap carries more than ~5 VALU (one wave per SIMD:
                            // nothing else covers a longer gap).  Position P = 4 ts + ps of the chunk's twelve, slot k of its twelve; k 0..7
                            // also carry an A fragment read, k 8 / 11 a B fragment load, k 9 / 10 nothing else.  Pieces: "fill" = two channels
                            // of a padded pixel; "V" = one channel of one position; "hi" / "lo" = the two steps of a pair's split.
                            //   P 0      k 0, 1 {mean, rstd} of the next chunk; k 3..8, 11 (and P 1 k 0) fill A; k 9, 10 fetch item B (pixels 0, 1)
                            //   P 1      k 1..4 fill Q, k 5..8 V of Q, k 11 hi;                                   k 9, 10 fetch item B (pixels 2, 3)
                            //   P 2..5   item A, position P - 2: k 0, 1 V, 2 hi, 3 lo, 4, 5 V, 6 hi, 7 lo, k 9 / 10 the two stores
                            //            (k 8 / 11 of P 2, 3: the rest of Q and its stores; k 8..11 of P 4, 5: fill B)
                            //   P 6..9   item B, position P - 6, the same; k 8 / 11 of P 6, 7 fetch item A of the chunk after the next, of P 8 Q
                            // Stores to An lie between the barrier of stage 0 (it releases the buffer the previous chunk read) and the barrier
                            // of stage 2 (An is first read at P 11); a fetch has >= 47 slots (a stage) of flight before its first use ----
                            const int P = ts * 4 + ps;
                            if (P == 0 && k < 2) stats_half(mu, rs, c_n, par_n, k);
                            {
                                const int j = P == 0 ? (k >= 3 && k <= 8 ? k - 3 : (k == 11 ? 6 : -1)) : (P == 1 && k == 0 ? 7 : -1);
                                if (j >= 0) fill_half(IA.d[j >> 1], mu, flgA, edge_nn, j >> 1, j & 1);
                            }
                            if (P <= 1 && (k == 9 || k == 10)) IB.d[P * 2 + k - 9] = load_px(xb_n, relB, flgB, edge_nn, P * 2 + k - 9);
                            // the quarter item: this wave's position of a left-over item
                            if (P == 1 && (k == 1 || k == 2)) fill_half(Qa, mu, flgQ, edge_nn, qa, k - 1);
                            if (P == 1 && (k == 3 || k == 4)) fill_half(Qb, mu, flgQ, edge_nn, qb, k - 3);
                            if (P == 1 && k >= 5 && k <= 8) {
                                const bool nrm = XF == 2 && wave == 1;
                                qv[k - 5] = quarter_v<XF>(Qa[k - 5], Qb[k - 5], nrm ? mu[k - 5] : 0.f, qsg, rs[k - 5]);
                            }
                            if (P == 1 && k == 11) split_hi(qv[0], qv[1], qh[0], qth[0], qth[1]);
                            if (P == 2 && k == 8) split_hi(qv[2], qv[3], qh[1], qth[2], qth[3]);
                            if (P == 2 && k == 11) split_lo(qv[0], qv[1], qth[0], qth[1], ql[0]);
                            if (P == 3 && k == 8) {
                                split_lo(qv[2], qv[3], qth[2], qth[3], ql[1]);
                                *reinterpret_cast<u32x2*>(An + dstQ) = u32x2{qh[0], qh[1]};
                            }
                            if (P == 3 && k == 11) *reinterpret_cast<u32x2*>(An + (dstQ ^ 32)) = u32x2{ql[0], ql[1]};
                            if (P >= 2 && P <= 9) {               // items A, B of the next chunk
                                const Item& It = P < 6 ? IA : IB;
                                const int q = (P - 2) & 3, half = k >> 2;
                                if (k < 8 && (k & 3) < 2) tv[k & 3] = item_v(It, mu, rs, q, 2 * half + (k & 3));
                                if (k < 8 && (k & 3) == 2) split_hi(tv[0], tv[1], hh[half], th[0], th[1]);
                                if (k < 8 && (k & 3) == 3) split_lo(tv[0], tv[1], th[0], th[1], ll[half]);
                                const int a = q * A_PLANE + (P < 6 ? dstA : dstB);
                                if (k == 9) *reinterpret_cast<u32x2*>(An + a) = u32x2{hh[0], hh[1]};
                                if (k == 10) *reinterpret_cast<u32x2*>(An + (a ^ 32)) = u32x2{ll[0], ll[1]};
                            }
                            if ((P == 4 || P == 5) && k >= 8) {
                                const int j = (P - 4) * 4 + k - 8;
                                fill_half(IB.d[j >> 1], mu, flgB, edge_nn, j >> 1, j & 1);
                            }
                            // fetches of the chunk after the next: items A and Q
                            if ((P == 6 || P == 7) && (k == 8 || k == 11)) IA.d[(P - 6) * 2 + (k == 11 ? 1 : 0)] = load_px(xb_2, relA, flgA, edge_2, (P - 6) * 2 + (k == 11 ? 1 : 0));
                            if (P == 8 && k == 8) Qa = load_px(xb_2, relQ, flgQ, edge_2, qa);
                            if (P == 8 && k == 11) Qb = load_px(xb_2, relQ, flgQ, edge_2, qb);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (ps == 1 && VAR != 4) {
                        lds_barrier();
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                ++sg;
            };
            stage(std::integral_constant<int, 0>{});
            stage(std::integral_constant<int, 1>{});
            stage(std::integral_constant<int, 2>{});
            ++cg;
        }

        // ---- epilogue of the tile: output transform in registers, bias, activation, statistics, NHWC stores.  A wave holds ALL 128 rows of its
        // 32 channels: the per-(sample, channel, tile) statistics slot is complete inside the wave (no LDS, no barrier) ----
        {
            const float gain = (p.act == 1) ? p.gain : 1.f;
            const bool do_act = p.act != 0;
            const bool stats = p.stats_ws != nullptr;
            float* yb = p.y + (size_t)cur.tb * p.Ho * p.Wo * p.Cout;
            const int co = cur.n0 + wn * 32 + li;
            const float bsv = p.bias ? p.bias[co] : 0.f;
            const float slp = (p.act == 2) ? p.slope[co] : p.alpha;
            double st_s = 0.0, st_q = 0.0;
#pragma unroll
            for (int tm = 0; tm < 4; ++tm) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float y0[4], y1[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = 4 * g + i;
                        const float m0 = acc[0][tm][r], m1 = acc[1][tm][r], m2 = acc[2][tm][r], m3 = acc[3][tm][r];
                        float a = (m0 + m1) + m2 + bsv;
                        float b = (m1 - m2) - m3 + bsv;
                        if (do_act) {
                            a = (a > 0.f ? a : a * slp) * gain;
                            b = (b > 0.f ? b : b * slp) * gain;
                        }
                        y0[i] = a;
                        y1[i] = b;
                        if (stats) {
                            st_s += (double)a + (double)b;
                            st_q += (double)a * (double)a + (double)b * (double)b;
                        }
                    }
                    quad_transpose4(y0[0], y0[1], y0[2], y0[3], li);
                    quad_transpose4(y1[0], y1[1], y1[2], y1[3], li);
                    const int m = tm * 32 + (li & 3) + 8 * g + 4 * kh;
                    const int oy = cur.ty0 + (m >> 3), ox = cur.tx0 + 2 * (m & 7);
                    float* dst = yb + ((size_t)oy * p.Wo + ox) * p.Cout + (co - (li & 3));
                    *reinterpret_cast<f32x4*>(dst) = f32x4{y0[0], y0[1], y0[2], y0[3]};
                    *reinterpret_cast<f32x4*>(dst + p.Cout) = f32x4{y1[0], y1[1], y1[2], y1[3]};
                }
            }
            if (stats) {
                st_s += __shfl_xor(st_s, 32, 64);            // the two k-halves of a lane pair hold rows 4 kh .. of the same channel
                st_q += __shfl_xor(st_q, 32, 64);
                if (kh == 0) {
                    double* slot = p.stats_ws + (((size_t)cur.tb * p.Cout + co) * p.stats_slots + cur.slot) * 2;
                    slot[0] = st_s;
                    slot[1] = st_q;
                }
            }
        }
        if (!has_next) break;
        cur = nxt;
        par ^= 1;
        t_next += G;
        has_next = t_next < ntiles;
        if (has_next) nxt = decode(t_next);
    }
}

}  // namespace

// conv_wino.hip's launcher: launches without a K split
int e4s_launch_wino1w(const e4s_conv_params& p, int ntn, int tx_n, int per_img, int ntiles, int grid, hipStream_t st) {
    static std::atomic<uint64_t> m0{0}, m2{0};
    int e;
#ifdef E4S_ABLATIONS
    {
        const char* ev = getenv("E4S_WINO_1W_VAR");
        const int var = ev ? atoi(ev) : 0;
        const void* fn = nullptr;
#define WV(V) case V: fn = (const void*)conv_wino1w_kernel<0, V>; if ((e = (int)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_1W))) return e; \
              hipLaunchKernelGGL((conv_wino1w_kernel<0, V>), dim3((unsigned)grid), dim3(NTHR), SMEM_1W, st, p, ntn, tx_n, per_img, ntiles); \
              E4S_CHECK_LAUNCH(); return 0;
        switch (p.in_stats ? 0 : var) {
            WV(1) WV(2) WV(3) WV(4)
            default: break;
        }
#undef WV
    }
#endif
    if (p.in_stats) {
        if (p.Cin > 1024) return (int)hipErrorInvalidValue;
        if ((e = e4s_ensure_dyn_smem((const void*)conv_wino1w_kernel<2>, SMEM_1W + 16384, m2))) return e;
        hipLaunchKernelGGL(conv_wino1w_kernel<2>, dim3((unsigned)grid), dim3(NTHR), SMEM_1W + p.Cin * 16, st, p, ntn, tx_n, per_img, ntiles);
    } else {
        if ((e = e4s_ensure_dyn_smem((const void*)conv_wino1w_kernel<0>, SMEM_1W, m0))) return e;
        hipLaunchKernelGGL(conv_wino1w_kernel<0>, dim3((unsigned)grid), dim3(NTHR), SMEM_1W, st, p, ntn, tx_n, per_img, ntiles);
    }
    E4S_CHECK_LAUNCH();
    return 0;
}
