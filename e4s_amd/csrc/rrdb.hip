// Real-ESRNet x4 (RRDBNet, e4s_amd/sr.py; src/pretrained/gpen/sr_model/rrdbnet_arch.py): the dense-block 3x3 conv and the net's head and tail.
//
// A residual dense block is five stride-1 3x3 convs with 32 outputs over a growing concatenation (Cin = 32, 64, 96, 128, 160).  The
// concatenation is never copied: a block lives in ONE NHWC buffer of 160 channels per pixel; conv k reads the first 32 k channels and
// writes channels [32 k, 32 k + 32) of the same buffer (disjoint from what any tile reads), conv5 writes into another buffer (its
// channels [0, 32) are halo inputs of the neighbouring tiles).  So the kernel takes a channel stride on both sides:
//   x      the first Cin channels of a buffer with x_cstride channels per pixel
//   y      32 channels at y + y_coff of a buffer with y_cstride channels per pixel
//   up2    the input is read at (y >> 1, x >> 1): F.interpolate(scale_factor=2, mode="nearest") folded into the halo staging of
//          conv_up1 / conv_up2 (rrdbnet_arch.py:115-116); the 4x intermediate is never written
//   epilogue (after + bias[32])   0: LeakyReLU(slope)   1: acc * s0 + r0   2: (acc * s0 + r0) * s1 + r1
//          (1 with s0 = 0.2: x5 * 0.2 + x; 2: the RRDB's outer out * 0.2 + x on its third block; 1 with s0 = 1: feat + conv_body(..))
// Tile: 16 x 16 output pixels x 32 channels per 256-thread block (the layout of conv_c32.hip: four waves of 64 pixels, two 32x32
// accumulators each), two blocks per CU.  The input channels go by in chunks of 32: per chunk the 18 x 18 halo (128 bytes per pixel)
// and the chunk's 9 x 32 x 32 weights (36 KB, pre-packed by e4s_rrdb_pack_f32) are staged in LDS, the next chunk's global loads are
// in flight (registers) while the 9 taps of this one run.  LDS rows are 128 bytes with the 16-byte granule XOR-swizzled (conv_c32.hip).
// Arithmetic: split-bf16 (rows hold [32 hi | 32 lo] bf16; three v_mfma_f32_32x32x16_bf16 per product, lo x hi first, fp32 accumulate)
// or exact fp32 (rows hold 32 floats; v_mfma_f32_32x32x2_f32) -- the same tile code.  The summation order of an output is fixed
// (chunk, tap, k-step) and does not depend on the batch or on the tile's place.  Tiles that overhang the image are masked.
//
// Head: conv_first (3 -> 32) straight from uint8 HWC pixels (x / 255, optional BGR <-> RGB flip) or an fp32 NCHW image.
// Tail: conv_last (32 -> 3) to fp32 (NHWC or NCHW) and / or clamp(0, 1) * 255 rounded half-to-even to uint8 HWC (real_esrnet.py:53-55).
#include "common.h"

#pragma clang fp contract(off)

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

constexpr int KC = 32, ROWB = 128, LO = 64;                                     // one 32-channel chunk per 128-byte LDS row
constexpr int TW = 16, TH = 16, HALO_W = TW + 2, HALO = (TH + 2) * HALO_W;      // 16 x 16-pixel tiles, 324 halo pixels
constexpr int BM = TH * TW, BN = 32, NTHR = 256;                                // 4 waves x (64 pixels x 32 channels)
constexpr int ITEMS = HALO * 4, AJ = (ITEMS + NTHR - 1) / NTHR;                 // 1296 8-channel items, 6 per thread
constexpr int BPIECES = 9 * BN * 8, BJ = BPIECES / NTHR;                        // 2304 16-byte pieces, 9 per thread and chunk
constexpr int A_BYTES = HALO * ROWB, B_BYTES = 9 * BN * ROWB;                   // 41 472 + 36 864
constexpr int YLD = 36;                                                         // floats per pixel row of the output staging tile
constexpr int SMEM = B_BYTES + A_BYTES + BM * 4;                                // 79 360: two blocks per CU
static_assert(BPIECES % NTHR == 0 && BM == NTHR, "thread layout");
static_assert(BM * YLD * 4 <= A_BYTES, "the output staging tile aliases the halo buffer");
static_assert(2 * SMEM <= 160 * 1024, "two blocks per CU");

// byte offset of 16-byte granule g (0..7) of row r.  split-bf16: granules 0..3 hold 8 hi channels each, g + 4 (offset ^ 64) their lo
// halves; fp32: granule g holds channels 4 g .. 4 g + 3.  Weight rows key the swizzle on the row, halo rows on the halo column (the
// bank analysis is conv_c32.hip's).
__device__ __forceinline__ int swz(int r, int g) { return r * ROWB + ((g ^ ((r >> 1) & 7)) << 4); }
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

// F32: 1 = exact fp32 MFMA, 0 = split-bf16; UP2: 1 = the input is the nearest x2 upsampling of x [B,Hi,Wi,..]
template <int F32, int UP2>
__global__ __launch_bounds__(NTHR, 2) void rrdb_conv_kernel(const e4s_rrdb_params p, const int tx_n, const int per_img) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sB = smem;                                   // [9][32][ROWB]  weights of the current chunk
    unsigned char* sA = smem + B_BYTES;                         // [HALO][ROWB]   halo of the current chunk
    float* sY = reinterpret_cast<float*>(sA);                   // [BM][YLD]      output staging tile (aliases the halo)
    int* s_out = reinterpret_cast<int*>(sA + A_BYTES);          // [BM] output pixel index or -1

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int Ho = UP2 ? 2 * p.Hi : p.Hi, Wo = UP2 ? 2 * p.Wi : p.Wi;
    const int tb = blockIdx.x / per_img;
    const int rem = blockIdx.x - tb * per_img;
    const int tyb = rem / tx_n, txb = rem - tyb * tx_n;
    const int nchunk = p.Cin / KC;

    // this thread's halo items: (halo pixel, 8-channel group) -> offset of channel group 0 of the source pixel, the same for every chunk
    size_t aoff[AJ];
    bool aok[AJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        const int item = tid + NTHR * j;
        const int h = item >> 2, q = item & 3;
        const int hy = h / HALO_W, hx = h - hy * HALO_W;
        const int oy = tyb * TH + hy - 1, ox = txb * TW + hx - 1;
        aok[j] = item < ITEMS && (unsigned)oy < (unsigned)Ho && (unsigned)ox < (unsigned)Wo;
        const int iy = UP2 ? oy >> 1 : oy, ix = UP2 ? ox >> 1 : ox;
        aoff[j] = aok[j] ? (((size_t)tb * p.Hi + iy) * p.Wi + ix) * p.x_cstride + q * 8 : 0;
    }
    const f32x8 zero8 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x8 ra[AJ];
    f32x4 rb[BJ];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int j = 0; j < AJ; ++j) ra[j] = aok[j] ? load8(p.x + aoff[j] + chunk * KC) : zero8;
        const unsigned char* wb = reinterpret_cast<const unsigned char*>(p.w) + (size_t)chunk * B_BYTES;
#pragma unroll
        for (int j = 0; j < BJ; ++j) rb[j] = *reinterpret_cast<const f32x4*>(wb + (size_t)(tid + NTHR * j) * 16);
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int item = tid + NTHR * j;
            if (item < ITEMS) {
                if (F32) {
                    *reinterpret_cast<f32x4*>(sA + swz_halo(item >> 2, 2 * (item & 3))) = f32x4{ra[j][0], ra[j][1], ra[j][2], ra[j][3]};
                    *reinterpret_cast<f32x4*>(sA + swz_halo(item >> 2, 2 * (item & 3) + 1)) = f32x4{ra[j][4], ra[j][5], ra[j][6], ra[j][7]};
                } else {
                    split_store(sA, swz_halo(item >> 2, item & 3), ra[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
            const int i = tid + NTHR * j;
            *reinterpret_cast<f32x4*>(sB + swz(i >> 3, i & 7)) = rb[j];
        }
    };

    {
        const int ay = tyb * TH + tid / TW, ax = txb * TW + tid % TW;
        s_out[tid] = (ay < Ho && ax < Wo) ? (tb * Ho + ay) * Wo + ax : -1;
    }
    // fragment rows: wave w owns pixels 64 w .. 64 w + 63 of the tile (four image rows) as two 32-row MFMA tiles; ro[tm][tap] = byte
    // offset of (halo row of the pixel shifted by the tap, granule kh); further granules are XORs of the offset
    int ro[2][9];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
        const int m_row = wave * 64 + tm * 32 + li;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
            ro[tm][tap] = swz_halo((m_row / TW + tap / 3) * HALO_W + (m_row % TW) + tap % 3, kh);
    }
    const int brow = swz(li, kh);                               // + tap * BN * ROWB (a multiple of 16 rows: the swizzle term is the row's own)

    f32x16 acc[2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
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
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(sA + (ro[0][tap] ^ (gp * 32)));
                    const f32x4 a1 = *reinterpret_cast<const f32x4*>(sA + (ro[1][tap] ^ (gp * 32)));
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b4[s], acc[0], 0, 0, 0);
                        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b4[s], acc[1], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const bf16x8 bh = *reinterpret_cast<const bf16x8*>(Bt + (brow ^ (kk * 32)));
                    const bf16x8 bl = *reinterpret_cast<const bf16x8*>(Bt + (brow ^ (kk * 32) ^ LO));
                    bf16x8 ah[2], al[2];
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm) {
                        ah[tm] = *reinterpret_cast<const bf16x8*>(sA + (ro[tm][tap] ^ (kk * 32)));
                        al[tm] = *reinterpret_cast<const bf16x8*>(sA + (ro[tm][tap] ^ (kk * 32) ^ LO));
                    }
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[0], bh, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[1], bh, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[0], bl, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[1], bl, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[0], bh, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[1], bh, acc[1], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue: + bias (and LeakyReLU) into the LDS staging tile, then 16-byte stores, 8 lanes per pixel's 128-byte slice ----
    const float bsv = p.bias[li];
    __syncthreads();                                            // every wave is through with the halo: sY may overwrite it
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wave * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            float v = acc[tm][r] + bsv;
            if (p.epilogue == 0) v = v > 0.f ? v : v * p.slope;
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
        if (p.epilogue >= 1) {
            const f32x4 r0 = *reinterpret_cast<const f32x4*>(p.r0 + (size_t)off * p.r0_cstride + p.r0_coff + c4 * 4);
            v = v * p.s0 + r0;
            if (p.epilogue == 2) {
                const f32x4 r1 = *reinterpret_cast<const f32x4*>(p.r1 + (size_t)off * p.r1_cstride + p.r1_coff + c4 * 4);
                v = v * p.s1 + r1;
            }
        }
        *reinterpret_cast<f32x4*>(p.y + (size_t)off * p.y_cstride + p.y_coff + c4 * 4) = v;
    }
}

// w [32][Cin][3][3] -> [Cin / 32][9][32 co][128 bytes]: 32 floats (SPLIT = 0) or [32 hi | 32 lo] bf16 (SPLIT = 1) of channels 32 chunk ..
template <int SPLIT>
__global__ void rrdb_pack_kernel(const float* __restrict__ w, unsigned char* __restrict__ out, int Cin, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ci = i & 31, co = (i >> 5) & 31;
    const int rest = i >> 10;
    const int tap = rest % 9, chunk = rest / 9;
    const float v = w[((size_t)co * Cin + chunk * KC + ci) * 9 + tap];
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

// conv_first: thread = (pixel, 8 of the 32 output channels); wp [27][32] ((ky, kx, ci)-major), zero padding 1
template <bool U8>
__global__ __launch_bounds__(256) void rrdb_head_kernel(const void* __restrict__ src, const float* __restrict__ wp,
                                                        const float* __restrict__ bias, float* __restrict__ y, int y_cs,
                                                        float* __restrict__ y2, int y2_cs, int H, int W, int flip, int64_t n) {
    __shared__ float sw[27 * 32 + 32];
    for (int k = threadIdx.x; k < 27 * 32 + 32; k += 256) sw[k] = k < 27 * 32 ? wp[k] : bias[k - 27 * 32];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int g = (int)(i & 3);
    const int64_t pix = i >> 2;
    const int ox = (int)(pix % W);
    const int oy = (int)((pix / W) % H);
    const int64_t b = pix / ((int64_t)W * H);
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = sw[27 * 32 + g * 8 + k];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy + ky - 1;
        if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox + kx - 1;
            if ((unsigned)ix >= (unsigned)W) continue;
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const int cs = flip ? 2 - ci : ci;
                float px;
                if constexpr (U8) px = (float)static_cast<const uint8_t*>(src)[((b * H + iy) * W + ix) * 3 + cs] / 255.f;
                else px = static_cast<const float*>(src)[((b * 3 + cs) * H + iy) * W + ix];
                const float* wr = sw + ((ky * 3 + kx) * 3 + ci) * 32 + g * 8;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] = fmaf(px, wr[k], acc[k]);
            }
        }
    }
    const f32x4 v0 = {acc[0], acc[1], acc[2], acc[3]}, v1 = {acc[4], acc[5], acc[6], acc[7]};
    float* o = y + pix * y_cs + g * 8;
    *reinterpret_cast<f32x4*>(o) = v0;
    *reinterpret_cast<f32x4*>(o + 4) = v1;
    if (y2) {
        o = y2 + pix * y2_cs + g * 8;
        *reinterpret_cast<f32x4*>(o) = v0;
        *reinterpret_cast<f32x4*>(o + 4) = v1;
    }
}

constexpr int TAIL_PASSES = 8;                                  // pixels per block = 32 * TAIL_PASSES

// conv_last: 8 lanes per pixel (4 input channels each; a pixel's 128-byte slice is one coalesced read), the lane's 27 weight quads in
// registers, the three sums combined over the 8 lanes by a butterfly (fixed order).  wp [9][3][32].
__global__ __launch_bounds__(256) void rrdb_tail_kernel(const float* __restrict__ x, int x_cs, const float* __restrict__ wp,
                                                        const float* __restrict__ bias, float* __restrict__ yf, int nchw,
                                                        uint8_t* __restrict__ yu, int flip, int H, int W, int64_t npix) {
    const int c4 = threadIdx.x & 7;
    f32x4 wq[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) wq[k] = *reinterpret_cast<const f32x4*>(wp + k * 32 + c4 * 4);
    const int64_t hw = (int64_t)H * W;
#pragma unroll 1
    for (int it = 0; it < TAIL_PASSES; ++it) {
        const int64_t pix = ((int64_t)blockIdx.x * TAIL_PASSES + it) * 32 + (threadIdx.x >> 3);
        const bool live = pix < npix;                           // (no early exit: the shuffles below want every lane)
        const int ox = live ? (int)(pix % W) : 0;
        const int oy = live ? (int)((pix / W) % H) : 0;
        const int64_t b = live ? pix / hw : 0;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy + ky - 1;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox + kx - 1;
                if (!live || (unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((b * H + iy) * W + ix) * x_cs + c4 * 4);
                const int t = (ky * 3 + kx) * 3;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a0 = fmaf(v[e], wq[t][e], a0);
                    a1 = fmaf(v[e], wq[t + 1][e], a1);
                    a2 = fmaf(v[e], wq[t + 2][e], a2);
                }
            }
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            a0 += __shfl_xor(a0, o, 64);
            a1 += __shfl_xor(a1, o, 64);
            a2 += __shfl_xor(a2, o, 64);
        }
        if (!live || c4 >= 3) continue;
        const float val = (c4 == 0 ? a0 : c4 == 1 ? a1 : a2) + bias[c4];
        if (yf) {
            if (nchw) yf[(b * 3 + c4) * hw + (pix - b * hw)] = val;
            else yf[pix * 3 + c4] = val;
        }
        if (yu) yu[pix * 3 + (flip ? 2 - c4 : c4)] = (uint8_t)rintf(fminf(fmaxf(val, 0.f), 1.f) * 255.f);
    }
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

template <int F32, int UP2>
int launch(const e4s_rrdb_params& p, int Ho, int Wo, hipStream_t st) {
    auto kern = rrdb_conv_kernel<F32, UP2>;
    static std::atomic<uint64_t> smem_set{0};
    if (int e = e4s_ensure_dyn_smem(reinterpret_cast<const void*>(kern), SMEM, smem_set)) return e;
    const int tx_n = (Wo + TW - 1) / TW, per_img = ((Ho + TH - 1) / TH) * tx_n;
    const int64_t ntiles = (int64_t)p.B * per_img;
    if (ntiles >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(NTHR), SMEM, st, p, tx_n, per_img);
    E4S_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int e4s_rrdb_conv_f32(const e4s_rrdb_params* pp, void* stream) {
    const e4s_rrdb_params& p = *pp;
    if (!p.x || !p.w || !p.bias || !p.y || p.B < 1 || p.Hi < 1 || p.Wi < 1) return (int)hipErrorInvalidValue;
    if (p.Cin < KC || p.Cin % KC || p.Cin > 160 || p.x_cstride < p.Cin || p.x_cstride % 4) return (int)hipErrorInvalidValue;
    if (p.y_cstride % 4 || p.y_coff % 4 || p.y_coff < 0 || p.y_coff + BN > p.y_cstride) return (int)hipErrorInvalidValue;
    if (p.epilogue < 0 || p.epilogue > 2 || (p.up2 != 0 && p.up2 != 1) || (p.precision != 0 && p.precision != 1))
        return (int)hipErrorInvalidValue;
    if (!aligned16(p.x) || !aligned16(p.w) || !aligned16(p.y)) return (int)hipErrorInvalidValue;
    // in place: only into channels the conv does not read (conv5 and the up-convs need another buffer)
    if (p.y == p.x && (p.up2 || p.y_cstride != p.x_cstride || p.y_coff < p.Cin)) return (int)hipErrorInvalidValue;
    if (p.epilogue >= 1 &&
        (!p.r0 || !aligned16(p.r0) || p.r0_cstride % 4 || p.r0_coff % 4 || p.r0_coff < 0 || p.r0_coff + BN > p.r0_cstride))
        return (int)hipErrorInvalidValue;
    if (p.epilogue == 2 &&
        (!p.r1 || !aligned16(p.r1) || p.r1_cstride % 4 || p.r1_coff % 4 || p.r1_coff < 0 || p.r1_coff + BN > p.r1_cstride))
        return (int)hipErrorInvalidValue;
    const int Ho = p.up2 ? 2 * p.Hi : p.Hi, Wo = p.up2 ? 2 * p.Wi : p.Wi;
    if ((int64_t)p.B * Ho * Wo >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipStream_t st = as_stream(stream);
    if (p.precision == 1) return p.up2 ? launch<1, 1>(p, Ho, Wo, st) : launch<1, 0>(p, Ho, Wo, st);
    return p.up2 ? launch<0, 1>(p, Ho, Wo, st) : launch<0, 0>(p, Ho, Wo, st);
}

extern "C" int64_t e4s_rrdb_pack_bytes(int Cin) { return Cin >= KC && Cin % KC == 0 ? (int64_t)(Cin / KC) * B_BYTES : 0; }

extern "C" int e4s_rrdb_pack_f32(const float* w, void* out, int Cin, int split, void* stream) {
    if (!w || !out || Cin < KC || Cin % KC || !aligned16(out)) return (int)hipErrorInvalidValue;
    const int n = (Cin / KC) * 9 * BN * KC;
    if (split) hipLaunchKernelGGL(rrdb_pack_kernel<1>, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), w,
                                  static_cast<unsigned char*>(out), Cin, n);
    else hipLaunchKernelGGL(rrdb_pack_kernel<0>, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), w,
                            static_cast<unsigned char*>(out), Cin, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_rrdb_head_f32(const void* src, int is_u8, int flip, const float* wp, const float* bias, float* y, int y_cstride,
                                 float* y2, int y2_cstride, int B, int H, int W, void* stream) {
    if (!src || !wp || !bias || !y || B < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
    if (y_cstride < 32 || y_cstride % 4 || !aligned16(y) || (y2 && (y2_cstride < 32 || y2_cstride % 4 || !aligned16(y2))))
        return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)B * H * W * 4;
    if ((n + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (is_u8) hipLaunchKernelGGL(rrdb_head_kernel<true>, grid, dim3(256), 0, as_stream(stream), src, wp, bias, y, y_cstride, y2,
                                  y2_cstride, H, W, flip ? 1 : 0, n);
    else hipLaunchKernelGGL(rrdb_head_kernel<false>, grid, dim3(256), 0, as_stream(stream), src, wp, bias, y, y_cstride, y2,
                            y2_cstride, H, W, flip ? 1 : 0, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_rrdb_tail_f32(const float* x, int x_cstride, const float* wp, const float* bias, float* yf, int nchw, uint8_t* yu,
                                 int flip, int B, int H, int W, void* stream) {
    if (!x || !wp || !bias || (!yf && !yu) || B < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
    if (x_cstride < 32 || x_cstride % 4 || !aligned16(x) || !aligned16(wp)) return (int)hipErrorInvalidValue;
    const int64_t npix = (int64_t)B * H * W;
    const int64_t blocks = (npix + 32 * TAIL_PASSES - 1) / (32 * TAIL_PASSES);
    if (blocks >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(rrdb_tail_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, x_cstride, wp, bias, yf,
                       nchw ? 1 : 0, yu, flip ? 1 : 0, H, W, npix);
    E4S_CHECK_LAUNCH();
    return 0;
}
