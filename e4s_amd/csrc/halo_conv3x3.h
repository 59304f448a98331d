// The halo-tiled 3x3 MFMA conv of the restoration networks: Real-ESRNet's dense-block convs (rrdb.hip) and ParseNet's reflect-padded
// conv family (parsenet.hip) are this one kernel.  NHWC fp32, Cin a multiple of 32, 32 output channels per block.
//   stride   1: 16 x 16 output pixels per block, 18 x 18 halo; 2: 8 x 16 output pixels, 17 x 33 halo
//   up2      the grid the conv runs on is the nearest x2 upsampling of x; grid position g reads source g >> 1, the upsampled map is
//            never written
//   Pad      what a grid position off the image reads (ZeroPad, ReflectPad below), folded into the halo staging: no padded copy
//   Epi      what happens to an accumulator on its way out (passed by value in the kernel arguments):
//              Epi::Chan chan(c)          the per-channel constants of output channel c, read once per lane
//              float point(acc, chan)     per accumulator, before the staging tile (bias, scale, LeakyReLU)
//              f32x4 store(v, off, c)     per 16-byte store of output pixel off, channels c .. c + 3 (the residual reads)
// A block computes 32 output channels of its pixel tile (blockIdx.y picks the 32); four waves own a quarter of the pixels each as 32-row
// MFMA tiles.  The input channels go by in chunks of 32: per chunk the halo (128 bytes per pixel) and the chunk's 9 x 32 x 32 weights
// (36 KB, pre-packed by halo_conv3x3_pack) are staged in LDS while the next chunk's global loads are in flight in registers.  LDS rows
// are 128 bytes with the 16-byte granule XOR-swizzled (mfma_rows.h).  Arithmetic: split-bf16 (rows hold [32 hi | 32 lo] bf16; three
// v_mfma_f32_32x32x16_bf16 per product, lo x hi first, fp32 accumulate) or exact fp32 (v_mfma_f32_32x32x2_f32) -- the same tile code.
// The summation order of an output is fixed (chunk, tap, k-step): its bits do not depend on the batch or on the tile's place.  Tiles
// that overhang the image are masked.
#pragma once
#include "mfma_rows.h"

// Intended to hold for the rest of the including file too: an Epi policy reproduces its net's arithmetic operation for operation only
// without fused multiply-adds, so every includer is compiled under it (both set it themselves as well).
#pragma clang fp contract(off)

namespace {

constexpr int BN = 32, NTHR = 256, TW = 16;
constexpr int BPIECES = 9 * BN * 8, BJ = BPIECES / NTHR;                        // 2304 16-byte pieces, 9 per thread and chunk
constexpr int B_BYTES = 9 * BN * ROWB;                                          // 36 864
constexpr int YLD = 36;                                                         // floats per pixel row of the output staging tile
static_assert(BPIECES % NTHR == 0, "thread layout");

template <int S>
struct Tile {
    static constexpr int TH = S == 2 ? 8 : 16;
    static constexpr int BM = TH * TW, TM = BM / 128;                           // 256 / 128 pixels; 2 / 1 MFMA row tiles per wave
    static constexpr int HALO_H = (TH - 1) * S + 3, HALO_W = (TW - 1) * S + 3;  // 18 x 18 / 17 x 33
    static constexpr int HALO = HALO_H * HALO_W;                                // 324 / 561 halo pixels
    static constexpr int ITEMS = HALO * 4, AJ = (ITEMS + NTHR - 1) / NTHR;      // 8-channel items: 6 / 9 per thread
    static constexpr int A_BYTES = HALO * ROWB;                                 // 41 472 / 71 808
    static constexpr int SMEM = B_BYTES + A_BYTES + BM * 4;                     // 79 360 (two blocks per CU) / 109 184 (one)
    static constexpr int OCC = 2 * SMEM <= 160 * 1024 ? 2 : 1;
    static_assert(BM * YLD * 4 <= A_BYTES, "the output staging tile aliases the halo buffer");
    static_assert(SMEM <= 160 * 1024, "LDS of one CU");
};

// ReflectionPad2d(1) on a grid of n >= 2 positions: -1 -> 1, n -> n - 2 (g is in [-1, n])
__device__ __forceinline__ int reflect1(int g, int n) { return g < 0 ? -g : (g >= n ? 2 * n - 2 - g : g); }

// Pad: is grid position g (in [-1, n] and past, where a tile overhangs) of a grid of n read at all, and from which position
struct ZeroPad {
    static __device__ __forceinline__ bool live(int g, int n) { return (unsigned)g < (unsigned)n; }
    static __device__ __forceinline__ int src(int g, int) { return g; }
};
struct ReflectPad {                                             // positions past the reflected border (n + 1 ..) belong to no live output
    static __device__ __forceinline__ bool live(int g, int n) { return g <= n; }
    static __device__ __forceinline__ int src(int g, int n) { return reflect1(g, n); }
};

// x: the first Cin channels of [B,Hi,Wi,x_cstride]; w: packed by halo_conv3x3_pack; y: channels [y_coff, y_coff + 32 gridDim.y) of
// [B,Ho,Wo,y_cstride]
struct HaloConvArgs {
    const float* x;
    const float* w;
    float* y;
    int B, Hi, Wi, Cin;
    int x_cstride, y_cstride, y_coff;
};

// F32: 1 = exact fp32 MFMA, 0 = split-bf16; S: stride; UP2: 1 = the grid is the nearest x2 upsampling of x [B,Hi,Wi,..]
template <int F32, int S, int UP2, class Pad, class Epi>
__global__ __launch_bounds__(NTHR, Tile<S>::OCC) void halo_conv3x3_kernel(const HaloConvArgs p, const Epi epi, const int Ho, const int Wo,
                                                                          const int tx_n, const int per_img) {
    typedef Tile<S> T;
    constexpr int TH = T::TH, BM = T::BM, TM = T::TM, HALO_W = T::HALO_W, ITEMS = T::ITEMS, AJ = T::AJ, A_BYTES = T::A_BYTES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sB = smem;                                   // [9][32][ROWB]  weights of the current chunk
    unsigned char* sA = smem + B_BYTES;                         // [HALO][ROWB]   halo of the current chunk
    float* sY = reinterpret_cast<float*>(sA);                   // [BM][YLD]      output staging tile (aliases the halo)
    int* s_out = reinterpret_cast<int*>(sA + A_BYTES);          // [BM] output pixel index or -1

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int Hg = UP2 ? 2 * p.Hi : p.Hi, Wg = UP2 ? 2 * p.Wi : p.Wi;          // the grid the padding applies on
    const int tb = blockIdx.x / per_img;
    const int rem = blockIdx.x - tb * per_img;
    const int tyb = rem / tx_n, txb = rem - tyb * tx_n;
    const int co = blockIdx.y * BN;                             // output channels co .. co + 31 (of the conv's own)
    const int nchunk = p.Cin / KC;

    // this thread's halo items: (halo pixel, 8-channel group) -> offset of channel group 0 of the source pixel, the same for every
    // chunk.  Positions that Pad does not read stay zero.
    size_t aoff[AJ];
    bool aok[AJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        const int item = tid + NTHR * j;
        const int h = item >> 2, q = item & 3;
        const int hy = h / HALO_W, hx = h - hy * HALO_W;
        const int gy = tyb * TH * S + hy - 1, gx = txb * TW * S + hx - 1;
        aok[j] = item < ITEMS && Pad::live(gy, Hg) && Pad::live(gx, Wg);
        const int ry = Pad::src(gy, Hg), rx = Pad::src(gx, Wg);
        const int iy = UP2 ? ry >> 1 : ry, ix = UP2 ? rx >> 1 : rx;
        aoff[j] = aok[j] ? (((size_t)tb * p.Hi + iy) * p.Wi + ix) * p.x_cstride + q * 8 : 0;
    }
    const f32x8 zero8 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x8 ra[AJ];
    f32x4 rb[BJ];
    const unsigned char* wbase = reinterpret_cast<const unsigned char*>(p.w) + (size_t)blockIdx.y * nchunk * B_BYTES;
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int j = 0; j < AJ; ++j) ra[j] = aok[j] ? load8(p.x + aoff[j] + chunk * KC) : zero8;
        const unsigned char* wb = wbase + (size_t)chunk * B_BYTES;
#pragma unroll
        for (int j = 0; j < BJ; ++j) rb[j] = *reinterpret_cast<const f32x4*>(wb + (size_t)(tid + NTHR * j) * 16);
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int item = tid + NTHR * j;
            if (item < ITEMS) {
                if (F32) {
                    *reinterpret_cast<f32x4*>(sA + swz_halo<HALO_W>(item >> 2, 2 * (item & 3))) = f32x4{ra[j][0], ra[j][1], ra[j][2], ra[j][3]};
                    *reinterpret_cast<f32x4*>(sA + swz_halo<HALO_W>(item >> 2, 2 * (item & 3) + 1)) =
                        f32x4{ra[j][4], ra[j][5], ra[j][6], ra[j][7]};
                } else {
                    split_store(sA, swz_halo<HALO_W>(item >> 2, item & 3), ra[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
            const int i = tid + NTHR * j;
            *reinterpret_cast<f32x4*>(sB + swz(i >> 3, i & 7)) = rb[j];
        }
    };

    if (tid < BM) {                                             // (BM is 128 at stride 2)
        const int ay = tyb * TH + tid / TW, ax = txb * TW + tid % TW;
        s_out[tid] = (ay < Ho && ax < Wo) ? (tb * Ho + ay) * Wo + ax : -1;
    }
    // fragment rows: wave w owns pixels 32 TM w .. 32 TM (w + 1) - 1 of the tile as TM 32-row MFMA tiles; ro[tm][tap] = byte offset of
    // (halo row of the pixel's window shifted by the tap, granule kh); further granules are XORs of the offset
    int ro[TM][9];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int m_row = (wave * TM + tm) * 32 + li;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
            ro[tm][tap] = swz_halo<HALO_W>(((m_row / TW) * S + tap / 3) * HALO_W + (m_row % TW) * S + tap % 3, kh);
    }
    const int brow = swz(li, kh);                               // + tap * BN * ROWB (a multiple of 16 rows: the swizzle term is the row's own)

    f32x16 acc[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tm][r] = 0.f;

    fetch(0);
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        __syncthreads();                                        // every reader of the previous chunk's LDS image is done
        stage();
        if (chunk + 1 < nchunk) fetch(chunk + 1);
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const unsigned char* Bt = sB + tap * (BN * ROWB);
            if (F32) {
                // lane (li, kh) holds channels 4 (2 gp + kh) + s of its row, for A and B alike: k-step (gp, s) contracts channels
                // 8 gp + s and 8 gp + 4 + s
#pragma unroll
                for (int gp = 0; gp < 4; ++gp) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(Bt + (brow ^ (gp * 32)));
                    f32x4 a4[TM];
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) a4[tm] = *reinterpret_cast<const f32x4*>(sA + (ro[tm][tap] ^ (gp * 32)));
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int tm = 0; tm < TM; ++tm) acc[tm] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tm][s], b4[s], acc[tm], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const bf16x8 bh = *reinterpret_cast<const bf16x8*>(Bt + (brow ^ (kk * 32)));
                    const bf16x8 bl = *reinterpret_cast<const bf16x8*>(Bt + (brow ^ (kk * 32) ^ LO));
                    bf16x8 ah[TM], al[TM];
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) {
                        ah[tm] = *reinterpret_cast<const bf16x8*>(sA + (ro[tm][tap] ^ (kk * 32)));
                        al[tm] = *reinterpret_cast<const bf16x8*>(sA + (ro[tm][tap] ^ (kk * 32) ^ LO));
                    }
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) acc[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[tm], bh, acc[tm], 0, 0, 0);
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) acc[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[tm], bl, acc[tm], 0, 0, 0);
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) acc[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[tm], bh, acc[tm], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue: Epi::point into the LDS staging tile, then 16-byte stores through Epi::store, 8 lanes per pixel's 128-byte slice ----
    const typename Epi::Chan ch = epi.chan(co + li);
    __syncthreads();                                            // every wave is through with the halo: sY may overwrite it
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (wave * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            sY[row * YLD + li] = epi.point(acc[tm][r], ch);
        }
    __syncthreads();
    const int c4 = tid & 7;
#pragma unroll
    for (int ps = 0; ps < BM / (NTHR / 8); ++ps) {
        const int px = ps * (NTHR / 8) + (tid >> 3);
        const int off = s_out[px];
        if (off < 0) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(sY + px * YLD + c4 * 4);
        *reinterpret_cast<f32x4*>(p.y + (size_t)off * p.y_cstride + p.y_coff + co + c4 * 4) = epi.store(v, (size_t)off, co + c4 * 4);
    }
}

// w [Cout][Cin][3][3] -> [Cout / 32][Cin / 32][9][32 co][128 bytes] (mfma_rows.h: pack_row_store)
template <int SPLIT>
__global__ void halo_conv3x3_pack_kernel(const float* __restrict__ w, unsigned char* __restrict__ out, int Cin, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ci = (int)(i & 31), co = (int)((i >> 5) & 31);
    const int64_t rest = i >> 10;
    const int nchunk = Cin / KC;
    const int tap = (int)(rest % 9);
    const int64_t cc = rest / 9;
    const int chunk = (int)(cc % nchunk), cb = (int)(cc / nchunk);
    pack_row_store<SPLIT>(out + (size_t)(i >> 5) * ROWB, ci, w[((size_t)(cb * BN + co) * Cin + chunk * KC + ci) * 9 + tap]);
}

// bytes of the packed weights; 0: not a shape the kernel takes
inline int64_t halo_conv3x3_pack_bytes(int Cin, int Cout) {
    return Cin >= KC && Cin % KC == 0 && Cout >= BN && Cout % BN == 0 ? (int64_t)(Cout / BN) * (Cin / KC) * B_BYTES : 0;
}

inline int halo_conv3x3_pack(const float* w, void* out, int Cin, int Cout, int split, hipStream_t st) {
    const int64_t n = (int64_t)(Cout / BN) * (Cin / KC) * 9 * BN * KC;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (split) hipLaunchKernelGGL(halo_conv3x3_pack_kernel<1>, grid, dim3(256), 0, st, w, static_cast<unsigned char*>(out), Cin, n);
    else hipLaunchKernelGGL(halo_conv3x3_pack_kernel<0>, grid, dim3(256), 0, st, w, static_cast<unsigned char*>(out), Cin, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

// Ho x Wo output pixels per image, Cout (a multiple of 32) output channels
template <int F32, int S, int UP2, class Pad, class Epi>
int halo_conv3x3_launch(const HaloConvArgs& p, const Epi& epi, int Ho, int Wo, int Cout, hipStream_t st) {
    typedef Tile<S> T;
    auto kern = halo_conv3x3_kernel<F32, S, UP2, Pad, Epi>;
    static std::atomic<uint64_t> smem_set{0};
    if (int e = e4s_ensure_dyn_smem(reinterpret_cast<const void*>(kern), T::SMEM, smem_set)) return e;
    const int tx_n = (Wo + TW - 1) / TW, per_img = ((Ho + T::TH - 1) / T::TH) * tx_n;
    const int64_t ntiles = (int64_t)p.B * per_img;
    if (ntiles >= (1ll << 31) || Cout / BN > 65535) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3((unsigned)ntiles, (unsigned)(Cout / BN)), dim3(NTHR), T::SMEM, st, p, epi, Ho, Wo, tx_n, per_img);
    E4S_CHECK_LAUNCH();
    return 0;
}

}  // namespace
