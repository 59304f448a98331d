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
// The kernel is the shared halo-tile kernel of halo_conv3x3.h (reflect padding, blockIdx.y picks 32 of the Cout channels, weights pre-packed
// by e4s_pconv_pack_f32): its tiles, LDS layout, arithmetic (split-bf16 or exact fp32) and fixed summation order are described there.
//
// Head: the encoder's first conv (3 -> Cout <= 64) straight from uint8 HWC pixels (x / 255 * 2 - 1 as face_parsing.py:59-63 computes
//       it, in double, optional BGR <-> RGB flip) or an fp32 NCHW image; reflect pad, + bias.
// Tail: out_mask_conv (Cin <= 64 -> 19), reflect pad, + bias, fused with the argmax over classes (first maximum, as torch.argmax) and
//       the MASK_COLORMAP lookup of face_parsing.py:30 (classes 0, 14 and 18 -> 0, every other -> 255).
#include "halo_conv3x3.h"

#pragma clang fp contract(off)

namespace {

// v = acc * scale[c] + bias[c] (either NULL: 1 and 0), optional LeakyReLU, then r0 + v, then r1 + v (either NULL: skipped)
struct PconvEpi {
    const float* scale;
    const float* bias;
    const float* r0;
    const float* r1;
    int r0_cstride, r1_cstride, lrelu;
    float slope;
    struct Chan { float scale, bias; };
    __device__ __forceinline__ Chan chan(int c) const { return {scale ? scale[c] : 1.f, bias ? bias[c] : 0.f}; }
    __device__ __forceinline__ float point(float acc, Chan k) const {
        float v = acc * k.scale + k.bias;
        if (lrelu) v = v > 0.f ? v : v * slope;
        return v;
    }
    __device__ __forceinline__ f32x4 store(f32x4 v, size_t off, int c) const {
        if (r0) v = *reinterpret_cast<const f32x4*>(r0 + off * r0_cstride + c) + v;
        if (r1) v = *reinterpret_cast<const f32x4*>(r1 + off * r1_cstride + c) + v;
        return v;
    }
};

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

template <int F32, int S, int UP2>
int launch(const e4s_pconv_params& p, int Ho, int Wo, hipStream_t st) {
    const HaloConvArgs a = {p.x, p.w, p.y, p.B, p.Hi, p.Wi, p.Cin, p.x_cstride, p.y_cstride, 0};
    const PconvEpi epi = {p.scale, p.bias, p.r0, p.r1, p.r0_cstride, p.r1_cstride, p.lrelu, p.slope};
    return halo_conv3x3_launch<F32, S, UP2, ReflectPad>(a, epi, Ho, Wo, p.Cout, st);
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

extern "C" int64_t e4s_pconv_pack_bytes(int Cin, int Cout) { return halo_conv3x3_pack_bytes(Cin, Cout); }

extern "C" int e4s_pconv_pack_f32(const float* w, void* out, int Cin, int Cout, int split, void* stream) {
    if (!w || !out || !aligned16(out) || e4s_pconv_pack_bytes(Cin, Cout) == 0) return (int)hipErrorInvalidValue;
    return halo_conv3x3_pack(w, out, Cin, Cout, split, as_stream(stream));
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
