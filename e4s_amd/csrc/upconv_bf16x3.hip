// Exact up-sampling StyledConv on the bf16 matrix cores at fp32-class accuracy: conv_transpose2d(stride 2, 3x3) followed by the
// 4x4 FIR blur, NoiseInjection and FusedLeakyReLU (src/models/stylegan2/model.py:287-300, 206-213, 396-404) in ONE kernel at
// ~1.5x the layer's MACs (9 Cin Cout per INPUT pixel; 1.52x for the tile halo).  The polyphase form on e4s_conv_bf16x3_f32
// (ncls = 4: four 3x3 phase kernels) spends 4x; the two unmasked up-convs of a face swap (128 -> 64 into 512^2, 64 -> 32 into
// 1024^2) ran 4-7x above their HBM floor on it.
//
// (1) The transposed conv as a SUB-PIXEL GEMM.  With I[q] = sum_{2u + k = q} x[u] W[k] (no flip: conv_transpose2d), the four
//     parity classes of q are four small convolutions over the INPUT grid,
//         I[2a + dy, 2b + dx] = sum over shifts (sy, sx) in {0,-1}^2 with (sy == 0 or dy == 0) and (sx == 0 or dx == 0) of
//                               x[a + sy, b + sx] . W[dy - 2 sy, dx - 2 sx]
//     class (0,0) has 4 taps, (0,1) and (1,0) two, (1,1) one: 9 (class, shift) blocks = exactly the layer's MACs, and the
//     scatter-add of the transposed conv happens in the MFMA accumulators.  Arithmetic as conv_bf16x3.hip: three
//     v_mfma_f32_32x32x16_bf16 per product on hi/lo-split fp32 operands, fp32 accumulate.
// (2) Tile = 8 x 16 anchors a (the GEMM's 128 rows) x 32 output channels x 4 classes (128 columns): a 16 x 32 patch of I for 32
//     channels = 64 KB of LDS, from which the FIR epilogue produces the 12 x 28 output pixels whose 4x4 windows lie inside
//     (the anchors overlap by 2 between tiles: 1.52x the MACs -- still 2.6x fewer than the polyphase form).
//     out = act(d[b,co] * sum_j kflip[j] I[o + j - 1] + noise_w * noise[b,o] + bias[co]) * gain.
// (3) TWO persistent 256-thread blocks per CU (round 5, VERDICT r4 'next' 3).  The round-3 form was one 512-thread block per CU with
//     128 KB of LDS whose phases ran back to back -- the K stages, the accumulator -> I-tile write, the FIR pass, the re-staging of the
//     weights the I tile had overwritten -- and its ablations put the epilogue at 41 % of the launch with the matrix pipe idle and the
//     main loop at 59 % with the VALU and the store path idle (profiles/r03_ablations_conv_c32_upconv.json); nothing inside one block
//     overlaps them without a second I tile, which the LDS does not have.  Here a block is 74 KB: 16-channel K stages (A 2 x 12 KB,
//     B 2 x 23 KB), the I tile aliased over ALL stage buffers (the next tile's first stage waits in registers through the FIR pass),
//     four waves of 32 anchors x all four classes (9 blocks = 27 MFMAs per stage each: no class imbalance to hide).  A CU holds two
//     independent blocks at different points of their tiles and the hardware overlaps one block's FIR / stores with the other's MFMA
//     stages: 0.88 -> 0.77 ms (64 -> 32 into 1024^2) and 0.69 -> 0.60 ms (128 -> 64 into 512^2) on the same box; one such block per
//     CU alone runs 1.07 ms (profiles/r05_upconv_two_blocks.json).  A start skew between the two blocks changes nothing (measured).
// (4) The FIR as a 4-tap row pass + a 4-tap column pass when the blur kernel is an outer product (the reference's always is): 8
//     multiply-adds per output instead of 16, 0.77 -> 0.71 / 0.60 -> 0.57 ms.
// Weights arrive pre-packed and pre-split by e4s_subpixel_weights_f32: [Cin/32][Cout/32][9 blocks][32 co][32 hi | 32 lo bf16]; a stage
// takes one 16-channel half of a row.
#include "conv_launch.h"
#include <stdlib.h>

namespace {


constexpr int PKC = 32;                                    // input channels per chunk of the weight PACK (a K stage takes half a chunk)
constexpr int KC = 16, ROWB = 80, LO = 32;                 // LDS rows: [16 hi | 16 lo | 16 bytes of padding] (80 = 16 x 5: conflict free)
constexpr int TAH = 8, TAW = 16;                           // anchors per tile (GEMM rows: 128)
constexpr int HH = TAH + 1, HW = TAW + 1, HALO = HH * HW;  // 9 x 17 input pixels: anchors and their (-1,-1) neighbours
constexpr int OH = 2 * TAH - 4, OW = 2 * TAW - 4;          // 12 x 28 outputs per tile
constexpr int IQH = 2 * TAH, IQW = 2 * TAW;                // 16 x 32 positions of I
constexpr int BNC = 32;                                    // output channels per tile
constexpr int NTHR = 256, NBLK = 9;
constexpr int ITEMS = HALO * 2;                            // (halo pixel, 8-channel group) items of one stage = 306
constexpr int AJ = (ITEMS + NTHR - 1) / NTHR;              // 2
constexpr int BPIECES = NBLK * BNC * 4;                    // 16-byte weight pieces of one stage = 1152
constexpr int BJ = (BPIECES + NTHR - 1) / NTHR;            // 5
constexpr int A_BYTES = HALO * ROWB;                       // 12 240
constexpr int B_BYTES = NBLK * BNC * ROWB;                 // 23 040
constexpr int STAGE_BYTES = 2 * A_BYTES + 2 * B_BYTES;     // 70 560
constexpr int I_BYTES = IQH * IQW * BNC * 4;               // 65 536
constexpr int NZ = OH * OW;                                // 336
constexpr int MAXC = 512;                                  // in_scale rows of the current and the next tile's sample live in LDS
constexpr int SMEM = STAGE_BYTES + NZ * 4 + 2 * MAXC * 4;  // 76 000: two blocks per CU
static_assert(I_BYTES <= STAGE_BYTES, "the I tile aliases the stage buffers");
static_assert(2 * SMEM <= 160 * 1024, "two blocks per CU");
static_assert(8 * OW <= NTHR && NZ <= 2 * NTHR, "epilogue thread layout");

__device__ __forceinline__ void split_store(unsigned char* dst, const f32x8 v) {
    const bf16x8 h = __builtin_convertvector(v, bf16x8);
    const f32x8 r = v - __builtin_convertvector(h, f32x8);
    const bf16x8 l = __builtin_convertvector(r, bf16x8);
    *reinterpret_cast<bf16x8*>(dst) = h;
    *reinterpret_cast<bf16x8*>(dst + LO) = l;
}

struct TileId { int tb, ty, tx, nt; };

// XF: 0 none, 1 v * in_scale[b][c] while the halo is staged (one style per sample: unmasked StyledConv, model.py:655-657)
// PC: 1 = per-channel noise, NHWC [Bn][Ho][Wo][Cout]: read beside the output store, 16 bytes per lane at the store's own address
// pattern (the row table s_nz is not written)
template <int XF, int PC = 0>
__global__ __launch_bounds__(NTHR, 2) void upconv_fused_kernel(const e4s_conv_params p, const float* __restrict__ k4, const int ntn,
                                                           const int tx_n, const int per_img, const int ntiles, const int abl_arg) {
    // abl (profiling builds only, -DE4S_ABLATIONS + env E4S_UPCONV3_ABL; results WRONG): 1 no MFMA stages, 2 no FIR / output stores,
    // 3 no epilogue at all, 4 no global loads, 5 no LDS staging of the prefetched operands, 6 FIR without the output stores,
    // 7 FIR without the accumulator -> I-tile write
#ifdef E4S_ABLATIONS
    const int abl = abl_arg;
#else
    constexpr int abl = 0;
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sA = smem;                          // [2][HALO][ROWB]
    unsigned char* sB = smem + 2 * A_BYTES;            // [2][9][32][ROWB]
    float* sI = reinterpret_cast<float*>(smem);        // [IQH][IQW][BNC]  (epilogue; aliases every stage buffer)
    float* s_nz = reinterpret_cast<float*>(smem + STAGE_BYTES);          // [OH*OW] noise_w * noise of the tile's output pixels
    float* s_sty = s_nz + NZ;                                            // XF: [2 tile parities][MAXC] in_scale row of the tile's sample

    const int tid = threadIdx.x;
    const int lane = tid & 63, wm = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kh = lane >> 5;
    const int G = gridDim.x;
    const int first = xcd_remap(blockIdx.x, G);
    const int nchunk = p.Cin / KC;                     // even (Cin % 32 == 0)
    const unsigned char* wbytes = reinterpret_cast<const unsigned char*>(p.w);
    const size_t img_stride = (size_t)p.Hi * p.Wi * p.Cin;

    auto decode = [&](int t) -> TileId {
        TileId id;
        const int mt = t / ntn;
        id.nt = t - mt * ntn;
        id.tb = mt / per_img;
        const int rem = mt - id.tb * per_img;
        id.ty = rem / tx_n;
        id.tx = rem - id.ty * tx_n;
        return id;
    };
    // halo item -> global offset inside the sample (floats); halo pixel (hy, hx) = input (6 ty - 2 + hy, 14 tx - 2 + hx)
    auto item_src = [&](const TileId& id, int item, bool& ok) -> size_t {
        const int h = item >> 1, q = item & 1;
        const int hy = h / HW, hx = h - hy * HW;
        const int iy = id.ty * (OH / 2) - 2 + hy, ix = id.tx * (OW / 2) - 2 + hx;
        ok = item < ITEMS && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
        return ok ? ((size_t)iy * p.Wi + ix) * p.Cin + q * 8 : (size_t)(q * 8);
    };
    auto item_dst = [&](int item) -> int { return (item >> 1) * ROWB + (item & 1) * 16; };
    const f32x8 zero8 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // weights of (16-channel chunk c, nt): rows of 128 bytes [32 hi | 32 lo] in the 32-channel pack; piece i -> LDS row i / 4, 16-byte
    // slot i % 4 (hi 0, hi 1, lo 0, lo 1) = bytes (c & 1) * 32 + (i & 1) * 16 of the row's hi (i & 2 == 0) or lo half
    auto b_src = [&](int i, int c, int nt) -> size_t {
        return ((size_t)(c >> 1) * ntn + nt) * (NBLK * BNC * 128) + (size_t)(i >> 2) * 128 + ((i >> 1) & 1) * 64 + (c & 1) * 32 + (i & 1) * 16;
    };
    auto b_dst = [&](int i) -> int { return (i >> 2) * ROWB + (i & 3) * 16; };

    struct AReg {
        f32x8 a[AJ];
        bool ok[AJ];
    };
    typedef f32x4 BReg[BJ];
    auto fetch_a = [&](AReg& R, const TileId& id, int chunk, bool real) {
        const float* xb = p.x + (real ? (size_t)id.tb * img_stride + chunk * KC : 0);
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int item = tid + NTHR * j;
            const size_t off = item_src(id, item, R.ok[j]);
            if (abl != 4) R.a[j] = load8(xb + off);
        }
    };
    // the style row of a tile's sample -> s_sty[par] (read at store time: a prefetched halo does not carry its style through the stages)
    auto load_style = [&](const TileId& id, int par) {
        if (XF)
            for (int i = tid * 4; i < p.Cin; i += NTHR * 4)
                *reinterpret_cast<f32x4*>(s_sty + par * MAXC + i) = *reinterpret_cast<const f32x4*>(p.in_scale + (size_t)id.tb * p.Cin + i);
    };
    auto fetch_b = [&](BReg& R, const TileId& id, int chunk, bool real) {
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
            const int i = tid + NTHR * j;
            if (abl != 4) R[j] = *reinterpret_cast<const f32x4*>(wbytes + b_src(i < BPIECES ? i : 0, real ? chunk : 0, real ? id.nt : 0));
        }
    };
    auto store_a = [&](const AReg& R, int buf, int chunk, int par) {
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int item = tid + NTHR * j;
            if (item < ITEMS) {
                f32x8 v = R.a[j];
                if (XF) v = v * load8(s_sty + par * MAXC + chunk * KC + (item & 1) * 8);
                if (!R.ok[j]) v = zero8;                    // zero padding applies after the style scale
                split_store(sA + buf * A_BYTES + item_dst(item), v);
            }
        }
    };
    auto store_b = [&](const BReg& R, int buf) {
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
            const int i = tid + NTHR * j;
            if (i < BPIECES) *reinterpret_cast<f32x4*>(sB + buf * B_BYTES + b_dst(i)) = R[j];
        }
    };

    if (first >= ntiles) return;
    TileId cur = decode(first);
    int t_next = first + G;
    bool has_next = t_next < ntiles;
    TileId nxt = decode(has_next ? t_next : first);

    // Flat sequence of (tile, chunk) stages, unrolled by two: even stages live in LDS buffers 0, odd ones in buffers 1.  A stage's halo is
    // fetched two stages ahead (register sets RE / RO) and stored one stage ahead, its weights (L2-resident) are fetched one stage ahead
    // -- across the tile boundary both wait in registers until the FIR pass has released the LDS.
    AReg RE, RO;
    BReg RB;
    int par = 0;                                       // parity of the block's tile counter: s_sty[par] is the current tile's style
    fetch_a(RE, cur, 0, true);
    fetch_b(RB, cur, 0, true);
    load_style(cur, 0);
    if (XF) __syncthreads();
    store_a(RE, 0, 0, 0);
    store_b(RB, 0);
    fetch_a(RO, cur, 1, true);
    __syncthreads();

    // fragment rows: anchor m = 32 wm + li -> (ay, ax) = (m / 16, m % 16); shift (sy, sx) reads halo pixel (ay + 1 + sy, ax + 1 + sx)
    const int m_row = wm * 32 + li;
    const int arow = ((m_row / TAW) * HW + (m_row % TAW)) * ROWB + kh * 16;
    const int brow = li * ROWB + kh * 16;
    // FIR epilogue role: 4 output channels of one output column, all 12 rows
    const int e_c4 = tid & 7, e_ox = tid >> 3;
    const bool e_act = e_ox < OW;

    // The blur kernel of the reference is always an outer product (make_kernel, model.py:23-31): k4 = u v^T lets the FIR run as a 4-tap
    // row pass + a 4-tap column pass (8 multiply-adds per output instead of 16).  Checked here, once per block, on the values themselves;
    // any other 4x4 kernel takes the generic 16-tap pass.  Flipped taps (upfirdn2d is a true convolution, upfirdn2d_kernel.cu:77):
    // kf[ay][ax] = k4[3-ay][3-ax] = fu[ay] * fv[ax].
    float fu[4], fv[4];
    bool sep;
    {
        float kk[16], vmax = 0.f;
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            kk[a] = k4[a];
            vmax = fmaxf(vmax, fabsf(kk[a]));
        }
        sep = kk[0] != 0.f;
        const float inv = sep ? 1.f / kk[0] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fu[3 - i] = kk[4 * i];
            fv[3 - i] = kk[i] * inv;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) sep = sep && fabsf(kk[4 * i + j] - fu[3 - i] * fv[3 - j]) <= 1e-6f * vmax;
    }

    f32x16 acc[4];                                      // one per class (dy, dx) = (cls >> 1, cls & 1)
    // block order in LDS / in the packed weights: class 0: shifts 0,1,2,3 -> 0..3; class 1: shifts 0,2 -> 4,5;
    // class 2: shifts 0,1 -> 6,7; class 3: shift 0 -> 8
    auto contract = [&](int buf) {
        const unsigned char* Ab = sA + buf * A_BYTES + arow;
        const unsigned char* Bb = sB + buf * B_BYTES + brow;
        struct Frag { bf16x8 h, l; };
        auto ldA = [&](int shift) -> Frag {
            const unsigned char* a = Ab + ((1 - (shift >> 1)) * HW + (1 - (shift & 1))) * ROWB;
            return Frag{*reinterpret_cast<const bf16x8*>(a), *reinterpret_cast<const bf16x8*>(a + LO)};
        };
        auto ldB = [&](int blk) -> Frag {
            const unsigned char* b = Bb + blk * (BNC * ROWB);
            return Frag{*reinterpret_cast<const bf16x8*>(b), *reinterpret_cast<const bf16x8*>(b + LO)};
        };
        // term-major over the targets of one A fragment: consecutive MFMAs write different accumulators
        {
            const Frag a0 = ldA(0), b0 = ldB(0), b4 = ldB(4), b6 = ldB(6), b8 = ldB(8);
            const Frag a1 = ldA(1), b1 = ldB(1), b7 = ldB(7);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.l, b0.h, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.l, b4.h, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.l, b6.h, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.l, b8.h, acc[3], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.h, b0.l, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.h, b4.l, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.h, b6.l, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.h, b8.l, acc[3], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.h, b0.h, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.h, b4.h, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.h, b6.h, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.h, b8.h, acc[3], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1.l, b1.h, acc[0], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1.l, b7.h, acc[2], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1.h, b1.l, acc[0], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1.h, b7.l, acc[2], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1.h, b1.h, acc[0], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1.h, b7.h, acc[2], 0, 0, 0);
        }
        {
            const Frag a2 = ldA(2), b2 = ldB(2), b5 = ldB(5);
            const Frag a3 = ldA(3), b3 = ldB(3);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2.l, b2.h, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2.l, b5.h, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2.h, b2.l, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2.h, b5.l, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2.h, b2.h, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2.h, b5.h, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.l, b3.h, acc[0], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.h, b3.l, acc[0], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.h, b3.h, acc[0], 0, 0, 0);
        }
    };

    for (;;) {
        if (has_next) load_style(nxt, par ^ 1);        // first read after this tile's FIR pass: barriers away
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
        // epilogue operands of THIS tile, requested now so that their latency hides under the tile's MFMA stages
        float nz_reg[2] = {0.f, 0.f};
        if (!PC && p.noise) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int e = tid + NTHR * j;
                const int oy = cur.ty * OH + e / OW, ox = cur.tx * OW + e % OW;
                if (e < NZ && oy < p.Ho && ox < p.Wo) nz_reg[j] = p.noise[(int64_t)cur.tb * p.noise_bstride + (int64_t)oy * p.Wo + ox];
            }
        }
        f32x4 d_reg = {1.f, 1.f, 1.f, 1.f}, b_reg = {0.f, 0.f, 0.f, 0.f};
        if (e_act) {
            const int co0 = cur.nt * BNC + e_c4 * 4;
            if (p.out_scale) d_reg = *reinterpret_cast<const f32x4*>(p.out_scale + (size_t)cur.tb * p.Cout + co0);
            if (p.bias) b_reg = *reinterpret_cast<const f32x4*>(p.bias + co0);
        }
        const float nw_reg = p.noise ? p.noise_w[0] : 0.f;

        for (int c0 = 0; c0 < nchunk; c0 += 2) {
            const bool last_pair = (c0 + 2 == nchunk);
            const TileId& nid = last_pair ? nxt : cur;       // owner of the two stages after this pair
            const bool nreal = !last_pair || has_next;
            const int ce = last_pair ? 0 : c0 + 2, co = last_pair ? 1 : c0 + 3;
            // ---- even stage: chunk c0 in buffers 0 ----
            fetch_a(RE, nid, ce, nreal);                     // halo of the next even stage (two stages ahead)
            fetch_b(RB, cur, c0 + 1, true);                  // weights of the odd stage
            if (abl != 1) contract(0);
            if (abl != 5) {
                store_a(RO, 1, c0 + 1, par);                 // halo of the odd stage, fetched during the previous odd stage
                store_b(RB, 1);
            }
            __syncthreads();
            // ---- odd stage: chunk c0 + 1 in buffers 1 ----
            fetch_a(RO, nid, co, nreal);
            fetch_b(RB, nid, ce, nreal);                     // weights of the next even stage
            if (abl != 1) contract(1);
            // after the tile's last stage the I tile overwrites every stage buffer: the next tile's first stage waits in RE / RB
            if (!last_pair && abl != 5) {
                store_a(RE, 0, ce, par);
                store_b(RB, 0);
            }
            __syncthreads();
        }

        // ---- epilogue (a): accumulators -> I tile; anchor (ay, ax), class (dy, dx) -> I[2 ay + dy][2 ax + dx][co] ----
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (!PC && tid + NTHR * j < NZ) s_nz[tid + NTHR * j] = nw_reg * nz_reg[j];      // (outside the aliased region)
        if (abl == 3 || abl == 7) asm volatile("" :: "v"(acc[0][0]), "v"(acc[1][7]), "v"(acc[2][3]), "v"(acc[3][9]));
        if (abl != 3 && abl != 7)
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            const int dy = cls >> 1, dx = cls & 1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const int qy = 2 * (m / TAW) + dy, qx = 2 * (m % TAW) + dx;
                sI[(qy * IQW + qx) * BNC + li] = acc[cls][r];
            }
        }
        __syncthreads();
        // ---- epilogue (b): FIR + demodulation + noise + bias + activation.  Output (oyl, oxl) of the tile reads I rows
        // oyl + 1 .. oyl + 4, columns oxl + 1 .. oxl + 4 (tile origin of I = 2 * (first anchor) = output origin - 2) ----
        if (e_act && abl != 2 && abl != 3) {
            const int co0 = cur.nt * BNC + e_c4 * 4;
            const int ox = cur.tx * OW + e_ox;
            const f32x4 d = d_reg, bs = b_reg;
            const float gain = (p.act == 1) ? p.gain : 1.f;
            const int ycs = p.y_cstride ? p.y_cstride : p.Cout;
            const float* ip = sI + (IQW + e_ox + 1) * BNC + e_c4 * 4;
            auto finish = [&](f32x4 v, int r) {
                const int oy = cur.ty * OH + r;
                if (oy < p.Ho && ox < p.Wo) {
                    if (PC) {
                        const f32x4 nz = *reinterpret_cast<const f32x4*>(
                            p.noise + ((int64_t)cur.tb * p.noise_bstride + (int64_t)oy * p.Wo + ox) * p.Cout + co0);
                        f32x4 nzw;
#pragma unroll
                        for (int e = 0; e < 4; ++e) nzw[e] = e4s_mul_rn(nw_reg, nz[e]);
                        v = v * d + bs + nzw;
                    } else
                    v = v * d + bs + s_nz[r * OW + e_ox];
                    if (p.act) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = (v[e] > 0.f ? v[e] : v[e] * p.alpha) * gain;
                    }
                    f32x4* dst = reinterpret_cast<f32x4*>(p.y + (((size_t)cur.tb * p.Ho + oy) * p.Wo + ox) * ycs + co0);
                    if (abl == 6) asm volatile("" :: "v"(v));
                    else *dst = v;
                }
            };
            if (sep) {
                // row pass on the way in (one new I row per output row), column pass over the last four row results
                auto hrow = [&](int ry) -> f32x4 {
                    const float* q = ip + ry * IQW * BNC;
                    return *reinterpret_cast<const f32x4*>(q) * fv[0] + *reinterpret_cast<const f32x4*>(q + BNC) * fv[1] +
                           *reinterpret_cast<const f32x4*>(q + 2 * BNC) * fv[2] + *reinterpret_cast<const f32x4*>(q + 3 * BNC) * fv[3];
                };
                f32x4 h0 = hrow(0), h1 = hrow(1), h2 = hrow(2);
#pragma unroll
                for (int r = 0; r < OH; ++r) {
                    const f32x4 h3 = hrow(r + 3);
                    finish(h0 * fu[0] + h1 * fu[1] + h2 * fu[2] + h3 * fu[3], r);
                    h0 = h1;
                    h1 = h2;
                    h2 = h3;
                }
            } else {
                float kf[16];
#pragma unroll
                for (int a = 0; a < 16; ++a) kf[a] = k4[15 - a];
                f32x4 win[3][4];                        // sliding window: 3 I rows carried, one new row per output
#pragma unroll
                for (int ry = 0; ry < 3; ++ry)
#pragma unroll
                    for (int ax = 0; ax < 4; ++ax) win[ry][ax] = *reinterpret_cast<const f32x4*>(ip + (ry * IQW + ax) * BNC);
#pragma unroll
                for (int r = 0; r < OH; ++r) {
                    f32x4 nw[4];
#pragma unroll
                    for (int ax = 0; ax < 4; ++ax) nw[ax] = *reinterpret_cast<const f32x4*>(ip + ((r + 3) * IQW + ax) * BNC);
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ax = 0; ax < 4; ++ax)
                        v += win[0][ax] * kf[ax] + win[1][ax] * kf[4 + ax] + win[2][ax] * kf[8 + ax] + nw[ax] * kf[12 + ax];
#pragma unroll
                    for (int ax = 0; ax < 4; ++ax) { win[0][ax] = win[1][ax]; win[1][ax] = win[2][ax]; win[2][ax] = nw[ax]; }
                    finish(v, r);
                }
            }
        }
        if (!has_next) break;
        __syncthreads();                               // every FIR read of the I tile is done: the stage buffers are free again
        if (abl != 5) {
            store_a(RE, 0, 0, par ^ 1);                // the next tile's first stage, parked in registers since its prefetch
            store_b(RB, 0);
        }
        __syncthreads();
        cur = nxt;
        par ^= 1;
        t_next += G;
        has_next = t_next < ntiles;
        if (has_next) nxt = decode(t_next);
    }
}

// w [Cout,Cin,3,3] -> the operand of upconv_fused_kernel, packed AND split: [Cin/32][Cout/32][9 blocks][32 co][32 hi | 32 lo] bf16.
// block -> (class, shift): 0..3 = class 0 shifts 0..3; 4,5 = class 1 shifts 0,2; 6,7 = class 2 shifts 0,1; 8 = class 3 shift 0;
// class (dy,dx) = (cls >> 1, cls & 1), shift s = (sy, sx) = (-(s >> 1), -(s & 1)); the tap is W[dy - 2 sy][dx - 2 sx].
__global__ void subpixel_weights_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int Cout, int Cin,
                                        int64_t n8) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // one (row, 8-channel group)
    if (i >= n8) return;
    const int q = (int)(i & 3);
    int64_t r = i >> 2;
    const int col = (int)(r % BNC); r /= BNC;
    const int blk = (int)(r % NBLK); r /= NBLK;
    const int ntn = Cout / BNC;
    const int nt = (int)(r % ntn), chunk = (int)(r / ntn);
    const int cls_of[9] = {0, 0, 0, 0, 1, 1, 2, 2, 3}, sh_of[9] = {0, 1, 2, 3, 0, 2, 0, 1, 0};
    const int cls = cls_of[blk], s = sh_of[blk];
    const int ky = (cls >> 1) + 2 * (s >> 1), kx = (cls & 1) + 2 * (s & 1);
    const int co = nt * BNC + col, ci0 = chunk * PKC + q * 8;
    f32x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = w[(((size_t)co * Cin + ci0 + e) * 3 + ky) * 3 + kx];
    const bf16x8 h = __builtin_convertvector(v, bf16x8);
    const f32x8 res = v - __builtin_convertvector(h, f32x8);
    const bf16x8 l = __builtin_convertvector(res, bf16x8);
    unsigned short* d = out + (i >> 2) * 64 + q * 8;
    *reinterpret_cast<bf16x8*>(d) = h;
    *reinterpret_cast<bf16x8*>(d + 32) = l;
}

}  // namespace

// out: (Cin/32) * (Cout/32) * 9 * 32 * 64 bf16 = 9 * Cout * Cin * 4 bytes (an opaque buffer only e4s_upconv_bf16x3_f32 reads)
extern "C" int e4s_subpixel_weights_f32(const float* w, void* out, int Cout, int Cin, void* stream) {
    if (Cout % BNC || Cin % PKC || Cout <= 0 || Cin <= 0) return (int)hipErrorInvalidValue;
    const int64_t n8 = (int64_t)(Cin / PKC) * (Cout / BNC) * NBLK * BNC * 4;
    hipLaunchKernelGGL(subpixel_weights_kernel, dim3(cdiv(n8, 256)), dim3(256), 0, as_stream(stream), w,
                       reinterpret_cast<unsigned short*>(out), Cout, Cin, n8);
    E4S_CHECK_LAUNCH();
    return 0;
}

// p: x NHWC [B,H,W,Cin], w = e4s_subpixel_weights_f32's output, y NHWC [B,2H,2W,Cout (or y_cstride)], in_scale [B,Cin] | null,
// out_scale [B,Cout] | null, noise (per pixel, or per channel [Bn][Ho][Wo][Cout], 16-byte aligned) / noise_w / bias / act / alpha /
// gain as e4s_conv_bf16x3_f32; k4: DEVICE pointer to the 4x4
// blur kernel (model.py:206-213, already x4).
extern "C" int e4s_upconv_bf16x3_f32(const e4s_conv_params* pp, const float* k4, void* stream) {
    const e4s_conv_params& p = *pp;
    // Cin % 32: the stage pipeline is unrolled by two 16-channel chunks
    if (p.Cin % (2 * KC) || p.Cin > MAXC || p.Cout % BNC || !k4 || p.labels || p.tiles || p.in_stats || p.act == 2 ||
        p.Ho != 2 * p.Hi || p.Wo != 2 * p.Wi || p.B <= 0 || (p.y_cstride && p.y_cstride % 4))
        return (int)hipErrorInvalidValue;
    hipStream_t st = as_stream(stream);
    const bool pc = p.noise && p.noise_per_channel;            // the editor's noise [Bn][Ho][Wo][Cout]: styled layers only (XF = 1)
    if (pc && (!p.in_scale || !p.noise_w || !aligned16(p.noise) || (p.noise_bstride != 0 && p.noise_bstride != (int64_t)p.Ho * p.Wo)))
        return (int)hipErrorInvalidValue;
    auto kern = pc ? upconv_fused_kernel<1, 1> : p.in_scale ? upconv_fused_kernel<1, 0> : upconv_fused_kernel<0, 0>;
    static std::atomic<uint64_t> smem_set0{0}, smem_set1{0}, smem_set2{0};
    if (int e = e4s_ensure_dyn_smem(reinterpret_cast<const void*>(kern), SMEM, pc ? smem_set2 : p.in_scale ? smem_set1 : smem_set0)) return e;
    const int ntn = p.Cout / BNC;
    const int tx_n = (p.Wo + OW - 1) / OW, per_img = ((p.Ho + OH - 1) / OH) * tx_n;
    const int64_t ntiles = (int64_t)p.B * per_img * ntn;
    if (ntiles >= (1ll << 31)) return (int)hipErrorInvalidValue;
    const int slots = 2 * e4s_num_cus();                    // two co-resident blocks per CU
    const int grid = (int)(ntiles < slots ? ntiles : slots);
    int abl = 0;
#ifdef E4S_ABLATIONS
    if (const char* e = getenv("E4S_UPCONV3_ABL")) abl = atoi(e);
#endif
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NTHR), SMEM, st, p, k4, ntn, tx_n, per_img, (int)ntiles, abl);
    E4S_CHECK_LAUNCH();
    return 0;
}
