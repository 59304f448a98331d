// GPEN's ParseNet (e4s_amd/parsenet.py; src/pretrained/gpen/face_parse/): the reflect-padded 3x3 conv family, the net's head and tail.
//
// Every conv of the net is ReflectionPad2d(1) + Conv2d(3x3, padding 0), stride 1 or 2, some behind a nearest x2 upsampling.  One
// halo-tiled MFMA kernel covers all of them for Cin, Cout multiples of 32 (the net uses 64, 128 and 256):
//   reflect  the map is folded into the halo staging: grid index -1 reads 1, index n reads n - 2.  No padded copy is ever written.
//   up2      the grid is the nearest x2 upsampling of x; the reflect map applies on that grid, then >> 1 gives the source pixel, so
//            the 4x map is never written (csrc/rrdb.hip does the same for its zero-padded up-convs)
//   stride   1: 16 x 16 output pixels per block, 18 x 18 halo; 2: 8 x 16 output pixels, 17 x 33 halo; Ho = (H + 2 - 3) / s + 1
//   epilogue v = acc * scale[c] + bias[c] (eval-mode BatchNorm folded on the host; either may be NULL), then optional LeakyReLU,
//            then optional + r0, then optional + r1 (NHWC maps at the output resolution: a block's identity + res, and the net's
//            feat + body(feat) on the last body block)
// A block computes 32 output channels of its pixel tile (blockIdx.y picks the 32); four waves own a quarter of the pixels each as 32-row
// MFMA tiles.  The input channels go by in chunks of 32: per chunk the halo (128 bytes per pixel) and the chunk's 9 x 32 x 32 weights
// (36 KB, pre-packed by e4s_pconv_pack_f32) are staged in LDS while the next chunk's global loads are in flight in registers.  LDS
// rows are 128 bytes with the 16-byte granule XOR-swizzled (csrc/conv_c32.hip).  Arithmetic: split-bf16 (rows hold [32 hi | 32 lo]
// bf16; three v_mfma_f32_32x32x16_bf16 per product, lo x hi first, fp32 accumulate) or exact fp32 (v_mfma_f32_32x32x2_f32) -- the
// same tile code.  The summation order of an output is fixed (chunk, tap, k-step): its bits do not depend on the batch or on the
// tile's place.  Tiles that overhang the image are masked.
//
// Head: the encoder's first conv (3 -> Cout <= 64) straight from uint8 HWC pixels (x / 255 * 2 - 1 as face_parsing.py:59-63 computes
//       it, in double, optional BGR <-> RGB flip) or an fp32 NCHW image; reflect pad, + bias.
// Tail: out_mask_conv (Cin <= 64 -> 19), reflect pad, + bias, fused with the argmax over classes (first maximum, as torch.argmax) and
//       the MASK_COLORMAP lookup of face_parsing.py:30 (classes 0, 14 and 18 -> 0, every other -> 255).
#include "common.h"

#pragma clang fp contract(off)

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

constexpr int KC = 32, ROWB = 128, LO = 64;                                     // one 32-channel chunk per 128-byte LDS row
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

// byte offset of 16-byte granule g (0..7) of row r.  split-bf16: granules 0..3 hold 8 hi channels each, g + 4 (offset ^ 64) their lo
// halves; fp32: granule g holds channels 4 g .. 4 g + 3.  Weight rows key the swizzle on the row, halo rows on the halo column.
__device__ __forceinline__ int swz(int r, int g) { return r * ROWB + ((g ^ ((r >> 1) & 7)) << 4); }
template <int HALO_W>
__device__ __forceinline__ int swz_halo(int h, int g) { return h * ROWB + ((g ^ (((h % HALO_W) >> 1) & 7)) << 4); }

__device__ __forceinline__ void split_store(unsigned char* base, int off, const f32x8 v) {
    const bf16x8 h = __builtin_convertvector(v, bf16x8);
    const f32x8 r = v - __builtin_convertvector(h, f32x8);
    const bf16x8 l = __builtin_convertvector(r, bf16x8);
    *reinterpret_cast<bf16x8*>(base + off) = h;
    *reinterpret_cast<bf16x8*>(base + (off ^ LO)) = l;
}

__device__ __forceinline__ f32x8 load8(const float* src) {
    const f32x4 lo4 = *reinterpret_cast<const f32x4*>(src);
    const f32x4 hi4 = *reinterpret_cast<const f32x4*>(src + 4);
    return f32x8{lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
}

// ReflectionPad2d(1) on a grid of n >= 2 positions: -1 -> 1, n -> n - 2 (g is in [-1, n])
__device__ __forceinline__ int reflect1(int g, int n) { return g < 0 ? -g : (g >= n ? 2 * n - 2 - g : g); }

// F32: 1 = exact fp32 MFMA, 0 = split-bf16; S: stride; UP2: 1 = the grid is the nearest x2 upsampling of x [B,Hi,Wi,..]
template <int F32, int S, int UP2>
__global__ __launch_bounds__(NTHR, Tile<S>::OCC) void pconv_kernel(const e4s_pconv_params p, const int Ho, const int Wo, const int tx_n,
                                                                   const int per_img) {
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
    const int Hg = UP2 ? 2 * p.Hi : p.Hi, Wg = UP2 ? 2 * p.Wi : p.Wi;          // the grid the reflect map applies on
    const int tb = blockIdx.x / per_img;
    const int rem = blockIdx.x - tb * per_img;
    const int tyb = rem / tx_n, txb = rem - tyb * tx_n;
    const int cb = blockIdx.y;                                  // output channels 32 cb .. 32 cb + 31
    const int nchunk = p.Cin / KC;

    // this thread's halo items: (halo pixel, 8-channel group) -> offset of channel group 0 of the source pixel, the same for every
    // chunk.  Grid positions past the reflected border (-1 and n) belong to no live output and stay zero.
    size_t aoff[AJ];
    bool aok[AJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        const int item = tid + NTHR * j;
        const int h = item >> 2, q = item & 3;
        const int hy = h / HALO_W, hx = h - hy * HALO_W;
        const int gy = tyb * TH * S + hy - 1, gx = txb * TW * S + hx - 1;
        aok[j] = item < ITEMS && gy <= Hg && gx <= Wg;
        const int ry = reflect1(gy, Hg), rx = reflect1(gx, Wg);
        const int iy = UP2 ? ry >> 1 : ry, ix = UP2 ? rx >> 1 : rx;
        aoff[j] = aok[j] ? (((size_t)tb * p.Hi + iy) * p.Wi + ix) * p.x_cstride + q * 8 : 0;
    }
    const f32x8 zero8 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x8 ra[AJ];
    f32x4 rb[BJ];
    const unsigned char* wbase = reinterpret_cast<const unsigned char*>(p.w) + (size_t)cb * nchunk * B_BYTES;
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

    if (tid < BM) {
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

    // ---- epilogue: scale, bias and LeakyReLU into the LDS staging tile, then 16-byte stores, 8 lanes per pixel's 128-byte slice ----
    const int co = cb * BN;
    const float scv = p.scale ? p.scale[co + li] : 1.f;
    const float bsv = p.bias ? p.bias[co + li] : 0.f;
    __syncthreads();                                            // every wave is through with the halo: sY may overwrite it
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (wave * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            float v = acc[tm][r] * scv + bsv;
            if (p.lrelu) v = v > 0.f ? v : v * p.slope;
            sY[row * YLD + li] = v;
        }
    __syncthreads();
    const int c4 = tid & 7;
#pragma unroll
    for (int ps = 0; ps < BM / (NTHR / 8); ++ps) {
        const int px = ps * (NTHR / 8) + (tid >> 3);
        const int off = s_out[px];
        if (off < 0) continue;
        f32x4 v = *reinterpret_cast<const f32x4*>(sY + px * YLD + c4 * 4);
        if (p.r0) v = *reinterpret_cast<const f32x4*>(p.r0 + (size_t)off * p.r0_cstride + co + c4 * 4) + v;
        if (p.r1) v = *reinterpret_cast<const f32x4*>(p.r1 + (size_t)off * p.r1_cstride + co + c4 * 4) + v;
        *reinterpret_cast<f32x4*>(p.y + (size_t)off * p.y_cstride + co + c4 * 4) = v;
    }
}

// w [Cout][Cin][3][3] -> [Cout / 32][Cin / 32][9][32 co][128 bytes]: 32 floats (SPLIT = 0) or [32 hi | 32 lo] bf16 (SPLIT = 1)
template <int SPLIT>
__global__ void pconv_pack_kernel(const float* __restrict__ w, unsigned char* __restrict__ out, int Cin, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ci = (int)(i & 31), co = (int)((i >> 5) & 31);
    const int64_t rest = i >> 10;
    const int nchunk = Cin / KC;
    const int tap = (int)(rest % 9);
    const int64_t cc = rest / 9;
    const int chunk = (int)(cc % nchunk), cb = (int)(cc / nchunk);
    const float v = w[((size_t)(cb * BN + co) * Cin + chunk * KC + ci) * 9 + tap];
    unsigned char* row = out + (size_t)(i >> 5) * ROWB;
    if (SPLIT) {
        const __bf16 h = (__bf16)v;
        const __bf16 l = (__bf16)(v - (float)h);
        reinterpret_cast<__bf16*>(row)[ci] = h;
        reinterpret_cast<__bf16*>(row + LO)[ci] = l;
    } else {
        reinterpret_cast<float*>(row)[ci] = v;
    }
}

constexpr int HEAD_CMAX = 64;

// head: thread = (pixel, 8 of the Cout output channels); wp [27][Cout] ((ky, kx, ci)-major), reflect padding 1
template <bool U8>
__global__ __launch_bounds__(256) void parsenet_head_kernel(const void* __restrict__ src, const float* __restrict__ wp,
                                                            const float* __restrict__ bias, float* __restrict__ y, int Cout, int H, int W,
                                                            int flip, int64_t n) {
    __shared__ float sw[27 * HEAD_CMAX + HEAD_CMAX];
    for (int k = threadIdx.x; k < 28 * Cout; k += 256) sw[k] = k < 27 * Cout ? wp[k] : bias[k - 27 * Cout];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int ng = Cout >> 3;
    const int g = (int)(i % ng);
    const int64_t pix = i / ng;
    const int ox = (int)(pix % W);
    const int oy = (int)((pix / W) % H);
    const int64_t b = pix / ((int64_t)W * H);
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = sw[27 * Cout + g * 8 + k];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = reflect1(oy + ky - 1, H);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = reflect1(ox + kx - 1, W);
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const int cs = flip ? 2 - ci : ci;
                float px;
                if constexpr (U8) px = (float)((double)static_cast<const uint8_t*>(src)[((b * H + iy) * W + ix) * 3 + cs] / 255.0 * 2.0 - 1.0);
                else px = static_cast<const float*>(src)[((b * 3 + cs) * H + iy) * W + ix];
                const float* wr = sw + ((ky * 3 + kx) * 3 + ci) * Cout + g * 8;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] = fmaf(px, wr[k], acc[k]);
            }
        }
    }
    float* o = y + pix * Cout + g * 8;
    *reinterpret_cast<f32x4*>(o) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4*>(o + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

constexpr int NCLS = 19, NCLS_PAD = 20, TAIL_CMAX = 64;

// tail: thread = pixel; wp [9][Cin][20] (class-minor, the 20th column zero) in LDS, read by every lane at the same address (a
// broadcast); 19 accumulators, summed in the fixed order (tap, channel).  Then the first maximum and the colour map.
__global__ __launch_bounds__(256) void parsenet_tail_kernel(const float* __restrict__ x, int x_cs, int Cin, const float* __restrict__ wp,
                                                            const float* __restrict__ bias, uint8_t* __restrict__ mask,
                                                            uint8_t* __restrict__ labels, float* __restrict__ logits, int H, int W,
                                                            int64_t npix) {
    __shared__ __attribute__((aligned(16))) float sw[9 * TAIL_CMAX * NCLS_PAD];
    const int nw = 9 * Cin * NCLS_PAD;
    for (int k = threadIdx.x * 4; k < nw; k += 256 * 4) *reinterpret_cast<f32x4*>(sw + k) = *reinterpret_cast<const f32x4*>(wp + k);
    __syncthreads();
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= npix) return;
    const int64_t hw = (int64_t)H * W;
    const int ox = (int)(pix % W);
    const int oy = (int)((pix / W) % H);
    const int64_t b = pix / hw;
    float acc[NCLS_PAD];
#pragma unroll
    for (int k = 0; k < NCLS_PAD; ++k) acc[k] = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = reflect1(oy + tap / 3 - 1, H), ix = reflect1(ox + tap % 3 - 1, W);
        const float* xp = x + ((b * H + iy) * W + ix) * x_cs;
        const float* wt = sw + tap * Cin * NCLS_PAD;
#pragma unroll 1
        for (int c = 0; c < Cin; c += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(xp + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int q = 0; q < NCLS_PAD / 4; ++q) {
                    const f32x4 w4 = *reinterpret_cast<const f32x4*>(wt + (c + e) * NCLS_PAD + q * 4);
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[q * 4 + k] = fmaf(v[e], w4[k], acc[q * 4 + k]);
                }
            }
        }
    }
    int best = 0;
    float bv = 0.f;
#pragma unroll
    for (int k = 0; k < NCLS; ++k) {
        const float v = acc[k] + bias[k];
        if (logits) logits[(b * NCLS + k) * hw + (pix - b * hw)] = v;
        if (k == 0 || v > bv) {                                 // strictly greater: the first maximum
            bv = v;
            best = k;
        }
    }
    if (labels) labels[pix] = (uint8_t)best;
    if (mask) mask[pix] = (best == 0 || best == 14 || best == 18) ? 0 : 255;
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

template <int F32, int S, int UP2>
int launch(const e4s_pconv_params& p, int Ho, int Wo, hipStream_t st) {
    typedef Tile<S> T;
    auto kern = pconv_kernel<F32, S, UP2>;
    static std::atomic<uint64_t> smem_set{0};
    if (int e = e4s_ensure_dyn_smem(reinterpret_cast<const void*>(kern), T::SMEM, smem_set)) return e;
    const int tx_n = (Wo + TW - 1) / TW, per_img = ((Ho + T::TH - 1) / T::TH) * tx_n;
    const int64_t ntiles = (int64_t)p.B * per_img;
    if (ntiles >= (1ll << 31) || p.Cout / BN > 65535) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3((unsigned)ntiles, (unsigned)(p.Cout / BN)), dim3(NTHR), T::SMEM, st, p, Ho, Wo, tx_n, per_img);
    E4S_CHECK_LAUNCH();
    return 0;
}

// output size of reflect pad 1 + 3x3 at the given stride on a grid of n (2 n with up2) positions; 0: a grid below 2 cannot be reflected
int out_size(int n, int stride, int up2) {
    const int g = up2 ? 2 * n : n;
    return g < 2 ? 0 : (g + 2 - 3) / stride + 1;
}

}  // namespace

extern "C" int e4s_pconv_f32(const e4s_pconv_params* pp, void* stream) {
    const e4s_pconv_params& p = *pp;
    if (!p.x || !p.w || !p.y || p.B < 1 || p.Hi < 1 || p.Wi < 1) return (int)hipErrorInvalidValue;
    if (p.Cin < KC || p.Cin % KC || p.Cout < BN || p.Cout % BN) return (int)hipErrorInvalidValue;
    if (p.x_cstride < p.Cin || p.x_cstride % 4 || p.y_cstride < p.Cout || p.y_cstride % 4) return (int)hipErrorInvalidValue;
    if ((p.stride != 1 && p.stride != 2) || (p.up2 != 0 && p.up2 != 1) || (p.up2 && p.stride != 1)) return (int)hipErrorInvalidValue;
    if ((p.lrelu != 0 && p.lrelu != 1) || (p.precision != 0 && p.precision != 1)) return (int)hipErrorInvalidValue;
    if (!aligned16(p.x) || !aligned16(p.w) || !aligned16(p.y) || p.y == p.x) return (int)hipErrorInvalidValue;
    if (p.r0 && (!aligned16(p.r0) || p.r0_cstride < p.Cout || p.r0_cstride % 4)) return (int)hipErrorInvalidValue;
    if (p.r1 && (!aligned16(p.r1) || p.r1_cstride < p.Cout || p.r1_cstride % 4)) return (int)hipErrorInvalidValue;
    const int Ho = out_size(p.Hi, p.stride, p.up2), Wo = out_size(p.Wi, p.stride, p.up2);
    if (Ho < 1 || Wo < 1) return (int)hipErrorInvalidValue;                       // reflect padding 1 needs a grid of 2 or more
    if ((int64_t)p.B * Ho * Wo >= (1ll << 31) || (int64_t)p.B * p.Hi * p.Wi >= (1ll << 31)) return (int)hipErrorInvalidValue;
    {
        const uintptr_t xa = reinterpret_cast<uintptr_t>(p.x), ya = reinterpret_cast<uintptr_t>(p.y);
        const uintptr_t xe = xa + (size_t)p.B * p.Hi * p.Wi * p.x_cstride * 4, ye = ya + (size_t)p.B * Ho * Wo * p.y_cstride * 4;
        if (xa < ye && ya < xe) return (int)hipErrorInvalidValue;               // y must not overlap x: its pixels are other tiles' halo
    }
    hipStream_t st = as_stream(stream);
    if (p.precision == 1) {
        if (p.stride == 2) return launch<1, 2, 0>(p, Ho, Wo, st);
        return p.up2 ? launch<1, 1, 1>(p, Ho, Wo, st) : launch<1, 1, 0>(p, Ho, Wo, st);
    }
    if (p.stride == 2) return launch<0, 2, 0>(p, Ho, Wo, st);
    return p.up2 ? launch<0, 1, 1>(p, Ho, Wo, st) : launch<0, 1, 0>(p, Ho, Wo, st);
}

extern "C" int64_t e4s_pconv_pack_bytes(int Cin, int Cout) {
    return Cin >= KC && Cin % KC == 0 && Cout >= BN && Cout % BN == 0 ? (int64_t)(Cout / BN) * (Cin / KC) * B_BYTES : 0;
}

extern "C" int e4s_pconv_pack_f32(const float* w, void* out, int Cin, int Cout, int split, void* stream) {
    if (!w || !out || !aligned16(out) || e4s_pconv_pack_bytes(Cin, Cout) == 0) return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)(Cout / BN) * (Cin / KC) * 9 * BN * KC;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (split) hipLaunchKernelGGL(pconv_pack_kernel<1>, grid, dim3(256), 0, as_stream(stream), w, static_cast<unsigned char*>(out), Cin, n);
    else hipLaunchKernelGGL(pconv_pack_kernel<0>, grid, dim3(256), 0, as_stream(stream), w, static_cast<unsigned char*>(out), Cin, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_parsenet_head_f32(const void* src, int is_u8, int flip, const float* wp, const float* bias, float* y, int Cout, int B,
                                     int H, int W, void* stream) {
    if (!src || !wp || !bias || !y || B < 1 || H < 2 || W < 2) return (int)hipErrorInvalidValue;
    if (Cout < 8 || Cout % 8 || Cout > HEAD_CMAX || !aligned16(y)) return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)B * H * W * (Cout / 8);
    if ((n + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (is_u8) hipLaunchKernelGGL(parsenet_head_kernel<true>, grid, dim3(256), 0, as_stream(stream), src, wp, bias, y, Cout, H, W,
                                  flip ? 1 : 0, n);
    else hipLaunchKernelGGL(parsenet_head_kernel<false>, grid, dim3(256), 0, as_stream(stream), src, wp, bias, y, Cout, H, W,
                            flip ? 1 : 0, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_parsenet_tail_f32(const float* x, int x_cstride, int Cin, const float* wp, const float* bias, uint8_t* mask,
                                     uint8_t* labels, float* logits, int B, int H, int W, void* stream) {
    if (!x || !wp || !bias || (!mask && !labels && !logits) || B < 1 || H < 2 || W < 2) return (int)hipErrorInvalidValue;
    if (Cin < 4 || Cin % 4 || Cin > TAIL_CMAX || x_cstride < Cin || x_cstride % 4 || !aligned16(x) || !aligned16(wp))
        return (int)hipErrorInvalidValue;
    const int64_t npix = (int64_t)B * H * W;
    if ((npix + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(parsenet_tail_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, as_stream(stream), x, x_cstride, Cin, wp,
                       bias, mask, labels, logits, H, W, npix);
    E4S_CHECK_LAUNCH();
    return 0;
}
