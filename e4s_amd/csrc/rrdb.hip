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
// The conv is the shared halo-tile kernel of halo_conv3x3.h (stride 1, zero padding, one 32-channel output block, weights pre-packed by
// e4s_rrdb_pack_f32): its tile, LDS layout, arithmetic (split-bf16 or exact fp32) and fixed summation order are described there.
//
// Head: conv_first (3 -> 32) straight from uint8 HWC pixels (x / 255, optional BGR <-> RGB flip) or an fp32 NCHW image.
// Tail: conv_last (32 -> 3) to fp32 (NHWC or NCHW) and / or clamp(0, 1) * 255 rounded half-to-even to uint8 HWC (real_esrnet.py:53-55).
#include "halo_conv3x3.h"

#pragma clang fp contract(off)

namespace {

// after + bias[c]:   0: LeakyReLU(slope)   1: v * s0 + r0   2: (v * s0 + r0) * s1 + r1, r0 / r1 read at their own channel offsets
struct RrdbEpi {
    const float* bias;
    const float* r0;
    const float* r1;
    int r0_cstride, r0_coff, r1_cstride, r1_coff, epilogue;
    float s0, s1, slope;
    struct Chan { float bias; };
    __device__ __forceinline__ Chan chan(int c) const { return {bias[c]}; }
    __device__ __forceinline__ float point(float acc, Chan k) const {
        float v = acc + k.bias;
        if (epilogue == 0) v = v > 0.f ? v : v * slope;
        return v;
    }
    __device__ __forceinline__ f32x4 store(f32x4 v, size_t off, int c) const {
        if (epilogue >= 1) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(r0 + off * r0_cstride + r0_coff + c);
            v = v * s0 + a0;
            if (epilogue == 2) {
                const f32x4 a1 = *reinterpret_cast<const f32x4*>(r1 + off * r1_cstride + r1_coff + c);
                v = v * s1 + a1;
            }
        }
        return v;
    }
};

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

template <int F32, int UP2>
int launch(const e4s_rrdb_params& p, int Ho, int Wo, hipStream_t st) {
    const HaloConvArgs a = {p.x, p.w, p.y, p.B, p.Hi, p.Wi, p.Cin, p.x_cstride, p.y_cstride, p.y_coff};
    const RrdbEpi epi = {p.bias, p.r0, p.r1, p.r0_cstride, p.r0_coff, p.r1_cstride, p.r1_coff, p.epilogue, p.s0, p.s1, p.slope};
    return halo_conv3x3_launch<F32, 1, UP2, ZeroPad>(a, epi, Ho, Wo, BN, st);
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

extern "C" int64_t e4s_rrdb_pack_bytes(int Cin) { return halo_conv3x3_pack_bytes(Cin, BN); }

extern "C" int e4s_rrdb_pack_f32(const float* w, void* out, int Cin, int split, void* stream) {
    if (!w || !out || Cin < KC || Cin % KC || !aligned16(out)) return (int)hipErrorInvalidValue;
    return halo_conv3x3_pack(w, out, Cin, BN, split, as_stream(stream));
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
