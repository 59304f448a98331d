// face-vid2vid's SPADE decoder (e4s_amd/spade.py; src/pretrained/face_vid2vid/modules/generator.py:121-159, util.py:419-481): what a SPADE
// layer needs beyond the plain convs of e4s_rconv_f32 -- all of it on the tile of gather_gemm.h, with the weights packed by
// e4s_rconv_pack_f32 (row blocks of 64 output channels).
//
// mlp_shared (e4s_spade_shared_f32): relu(3x3 conv of seg + bias) at the resolution of the map the SPADE modulates, seg being read
// through the nearest upsampling by 2^shift: output pixel (oy, ox) of the [Hs << shift, Ws << shift] grid reads seg at ((oy + ky - 1)
// >> shift, (ox + kx - 1) >> shift); the zero padding applies on the grid (a tap is live iff its grid coordinate is inside it).  The
// upsampled seg is never written.  floor(dst * 0.5) and floor(dst * 0.25) are exact in ATen's float arithmetic, so the shift IS
// F.interpolate(mode='nearest').  All SPADEs of one resolution read the same seg: their mlp_shared weights are concatenated along the
// output channels on the host and run as one launch; each SPADE's activation is a 128-channel slice of the result.
//
// The modulating conv (e4s_spade_conv_f32): mlp_gamma and mlp_beta of one SPADE as ONE implicit GEMM a -> 2 C, the rows of the two
// weights interleaved on the host ([gamma_c, beta_c, gamma_c+1, beta_c+1, ...]), so that the four consecutive channels of an
// Epi::store are gamma and beta of two output channels.  Neither gamma nor beta is stored: the epilogue reads x at (oy >> xs, ox >>
// xs) (xs = 1: x is the map before the nearest x2 upsampling, whose InstanceNorm statistics are those of the upsampled map: every
// value occurs four times) and that sample's {mean, rstd}, and writes
//     v = (x - mean) * rstd * (1 + (gamma + bias_gamma)) + (beta + bias_beta),      then v > 0 ? v : 0.2 v with act.
// Both activations map an exact zero to zero, so the zero padding of the conv that follows is unchanged by them.
// Arithmetic of both: split-bf16 or exact fp32 from the same tile code; the summation order of an output is (tap, chunk, k-step)
// whatever the batch or the tile's place.
//
// The tail (e4s_spade_tail_f32): sigmoid(conv_img(leaky_relu(x, 0.2))), 3x3, 64 -> 3, a streaming kernel in exact fp32 in either
// precision mode: 16 lanes per pixel (4 input channels each; a pixel's 256-byte slice is one coalesced read), the lane's 27 weight
// quads in registers, the three sums combined over the 16 lanes by a butterfly (fixed order).
#include "gather_gemm.h"                                        // the tile (gather_gemm_kernel)

#pragma clang fp contract(off)

namespace {

// Gather of gather_gemm.h: a zero-padded 3x3 conv at stride 1 on the grid [B,Ho,Wo], the source [B,Ho >> s,Wo >> s,x_cstride] read
// through the nearest upsampling by 2^s (s = 0: a plain conv)
struct SpadeGather {
    const float* x;
    int Hi, Wi, x_cstride, s, Ho, Wo;
    struct Item { int b, y, x, c; bool live; };
    struct Tap { int ky, kx; };
    __device__ __forceinline__ int ntaps() const { return 9; }
    __device__ __forceinline__ Item item(int m, bool live, int q) const {
        const int mm = live ? m : 0;
        const int ox = mm % Wo, t = mm / Wo;
        return Item{t / Ho, t % Ho - 1, ox - 1, q * 8, live};
    }
    __device__ __forceinline__ Tap tap(int t) const {
        const int ky = t / 3;
        return Tap{ky, t - ky * 3};
    }
    __device__ __forceinline__ bool src(const Item& it, const Tap& t, int chunk, const float*& ptr) const {
        const int gy = it.y + t.ky, gx = it.x + t.kx;
        const bool ok = it.live && (unsigned)gy < (unsigned)Ho && (unsigned)gx < (unsigned)Wo;
        const int iy = ok ? gy >> s : 0, ix = ok ? gx >> s : 0;
        ptr = x + (((size_t)it.b * Hi + iy) * Wi + ix) * x_cstride + chunk * KC + it.c;
        return ok;
    }
};

// Epi of mlp_shared: bias, ReLU, a channel slice of y
struct SharedEpi {
    const float* bias_p;
    float* y;
    int y_cstride, y_coff;
    __device__ __forceinline__ float bias(int c) const { return bias_p ? bias_p[c] : 0.f; }
    __device__ __forceinline__ void store(int pix, int c, f32x4 v) const {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        *reinterpret_cast<f32x4*>(y + (size_t)pix * y_cstride + y_coff + c) = v;
    }
};

// Epi of the modulating conv: conv channel c = 2 ch is gamma of output channel ch, c + 1 its beta
struct ModEpi {
    const float* bias_p;                                        // [2 C], interleaved like the rows
    const float* x;                                             // [B,xH,xW,x_cstride]
    const float* stats;                                         // [B,C,2] {mean, rstd}
    float* y;
    int Ho, Wo, xH, xW, xs, x_cstride, y_cstride, y_coff, C, act;
    __device__ __forceinline__ float bias(int c) const { return bias_p[c]; }
    __device__ __forceinline__ void store(int pix, int c, f32x4 v) const {
        const int ox = pix % Wo, t = pix / Wo;
        const int oy = t % Ho, b = t / Ho;
        const int ch = c >> 1;
        const float* xp = x + (((size_t)b * xH + (oy >> xs)) * xW + (ox >> xs)) * x_cstride + ch;
        const f32x4 st = *reinterpret_cast<const f32x4*>(stats + ((size_t)b * C + ch) * 2);
        float o0 = (xp[0] - st[0]) * st[1] * (1.f + v[0]) + v[1];
        float o1 = (xp[1] - st[2]) * st[3] * (1.f + v[2]) + v[3];
        if (act) {
            o0 = o0 > 0.f ? o0 : 0.2f * o0;
            o1 = o1 > 0.f ? o1 : 0.2f * o1;
        }
        float* dst = y + (size_t)pix * y_cstride + y_coff + ch;
        dst[0] = o0;
        dst[1] = o1;
    }
};

template <int F32, int BN, class Epi>
int launch_spade(const SpadeGather& g, const Epi& epi, const float* w, int Cin, int Cout, int M, hipStream_t st) {
    hipLaunchKernelGGL((gg::gather_gemm_kernel<F32, BN, SpadeGather, Epi>), dim3((unsigned)((M + gg::BM - 1) / gg::BM), (unsigned)(Cout / BN)),
                       dim3(gg::NTHR), 0, st, g, epi, w, Cin / KC, M);
    E4S_CHECK_LAUNCH();
    return 0;
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

constexpr int TAIL_C = 64, TAIL_PASSES = 8;                     // pixels per block = 16 * TAIL_PASSES

// wp [9][3][64]
__global__ __launch_bounds__(256) void spade_tail_kernel(const float* __restrict__ x, int x_cs, const float* __restrict__ wp,
                                                         const float* __restrict__ bias, float* __restrict__ yf, int nchw,
                                                         uint8_t* __restrict__ yu, float* __restrict__ logits, int H, int W, int64_t npix) {
    const int c4 = threadIdx.x & 15;
    f32x4 wq[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) wq[k] = *reinterpret_cast<const f32x4*>(wp + k * TAIL_C + c4 * 4);
    const int64_t hw = (int64_t)H * W;
#pragma unroll 1
    for (int it = 0; it < TAIL_PASSES; ++it) {
        const int64_t pix = ((int64_t)blockIdx.x * TAIL_PASSES + it) * 16 + (threadIdx.x >> 4);
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
                f32x4 v = *reinterpret_cast<const f32x4*>(x + ((b * H + iy) * W + ix) * x_cs + c4 * 4);
                const int t = (ky * 3 + kx) * 3;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float l = v[e] > 0.f ? v[e] : 0.2f * v[e];
                    a0 = fmaf(l, wq[t][e], a0);
                    a1 = fmaf(l, wq[t + 1][e], a1);
                    a2 = fmaf(l, wq[t + 2][e], a2);
                }
            }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            a0 += __shfl_xor(a0, o, 64);
            a1 += __shfl_xor(a1, o, 64);
            a2 += __shfl_xor(a2, o, 64);
        }
        if (!live || c4 >= 3) continue;
        const float z = (c4 == 0 ? a0 : c4 == 1 ? a1 : a2) + bias[c4];
        const float val = 1.f / (1.f + expf(-z));
        if (logits) logits[(b * 3 + c4) * hw + (pix - b * hw)] = z;
        if (yf) {
            if (nchw) yf[(b * 3 + c4) * hw + (pix - b * hw)] = val;
            else yf[pix * 3 + c4] = val;
        }
        if (yu) yu[pix * 3 + c4] = (uint8_t)rintf(fminf(fmaxf(val, 0.f), 1.f) * 255.f);
    }
}

}  // namespace

extern "C" int e4s_spade_shared_f32(const e4s_spade_shared_params* pp, void* stream) {
    if (!pp) return (int)hipErrorInvalidValue;
    const e4s_spade_shared_params& p = *pp;
    if (!p.seg || !p.w || !p.y || p.B < 1 || p.Hs < 1 || p.Ws < 1) return (int)hipErrorInvalidValue;
    if (p.Cin < KC || p.Cin % KC || p.Cout < 64 || p.Cout % 64 || p.Cout / 64 > 65535) return (int)hipErrorInvalidValue;
    if (p.shift < 0 || p.shift > 2 || (p.precision != 0 && p.precision != 1)) return (int)hipErrorInvalidValue;
    if (p.seg_cstride < p.Cin || p.seg_cstride % 4 || p.y_coff < 0 || p.y_coff % 4 || p.y_cstride < p.y_coff + p.Cout || p.y_cstride % 4)
        return (int)hipErrorInvalidValue;
    if (!aligned16(p.seg) || !aligned16(p.w) || !aligned16(p.y)) return (int)hipErrorInvalidValue;
    const int64_t Ho = (int64_t)p.Hs << p.shift, Wo = (int64_t)p.Ws << p.shift;
    const int64_t M = (int64_t)p.B * Ho * Wo;
    if (Ho >= (1ll << 30) || Wo >= (1ll << 30) || M >= (1ll << 31) - gg::BM) return (int)hipErrorInvalidValue;
    if (overlaps(p.seg, (size_t)p.B * p.Hs * p.Ws * p.seg_cstride * 4, p.y, (size_t)M * p.y_cstride * 4)) return (int)hipErrorInvalidValue;
    const SpadeGather g = {p.seg, p.Hs, p.Ws, p.seg_cstride, p.shift, (int)Ho, (int)Wo};
    const SharedEpi epi = {p.bias, p.y, p.y_cstride, p.y_coff};
    hipStream_t st = as_stream(stream);
    if (p.Cout % 128 == 0)
        return p.precision == 1 ? launch_spade<1, 128>(g, epi, p.w, p.Cin, p.Cout, (int)M, st) : launch_spade<0, 128>(g, epi, p.w, p.Cin, p.Cout, (int)M, st);
    return p.precision == 1 ? launch_spade<1, 64>(g, epi, p.w, p.Cin, p.Cout, (int)M, st) : launch_spade<0, 64>(g, epi, p.w, p.Cin, p.Cout, (int)M, st);
}

extern "C" int e4s_spade_conv_f32(const e4s_spade_conv_params* pp, void* stream) {
    if (!pp) return (int)hipErrorInvalidValue;
    const e4s_spade_conv_params& p = *pp;
    if (!p.a || !p.w || !p.bias || !p.x || !p.stats || !p.y || p.B < 1 || p.H < 1 || p.W < 1) return (int)hipErrorInvalidValue;
    if (p.Cin < KC || p.Cin % KC || p.C < 64 || p.C % 64 || 2 * p.C / 128 > 65535) return (int)hipErrorInvalidValue;
    if ((p.xs != 0 && p.xs != 1) || (p.act != 0 && p.act != 1) || (p.precision != 0 && p.precision != 1)) return (int)hipErrorInvalidValue;
    if (p.xH < 1 || p.xW < 1 || ((int64_t)p.xH << p.xs) != p.H || ((int64_t)p.xW << p.xs) != p.W) return (int)hipErrorInvalidValue;
    if (p.a_coff < 0 || p.a_coff % 4 || p.a_cstride < p.a_coff + p.Cin || p.a_cstride % 4) return (int)hipErrorInvalidValue;
    if (p.y_coff < 0 || p.y_coff % 4 || p.y_cstride < p.y_coff + p.C || p.y_cstride % 4) return (int)hipErrorInvalidValue;
    if (p.x_cstride < p.C || p.x_cstride % 4) return (int)hipErrorInvalidValue;
    if (!aligned16(p.a) || !aligned16(p.w) || !aligned16(p.x) || !aligned16(p.stats) || !aligned16(p.y)) return (int)hipErrorInvalidValue;
    const int64_t M = (int64_t)p.B * p.H * p.W;
    if (M >= (1ll << 31) - gg::BM) return (int)hipErrorInvalidValue;
    const size_t y_bytes = (size_t)M * p.y_cstride * 4;
    if (overlaps(p.a, (size_t)M * p.a_cstride * 4, p.y, y_bytes) || overlaps(p.x, (size_t)p.B * p.xH * p.xW * p.x_cstride * 4, p.y, y_bytes) ||
        overlaps(p.stats, (size_t)p.B * p.C * 8, p.y, y_bytes))
        return (int)hipErrorInvalidValue;
    const SpadeGather g = {p.a + p.a_coff, p.H, p.W, p.a_cstride, 0, p.H, p.W};
    const ModEpi epi = {p.bias, p.x, p.stats, p.y, p.H, p.W, p.xH, p.xW, p.xs, p.x_cstride, p.y_cstride, p.y_coff, p.C, p.act};
    hipStream_t st = as_stream(stream);
    return p.precision == 1 ? launch_spade<1, 128>(g, epi, p.w, p.Cin, 2 * p.C, (int)M, st) : launch_spade<0, 128>(g, epi, p.w, p.Cin, 2 * p.C, (int)M, st);
}

extern "C" int e4s_spade_tail_f32(const float* x, int x_cstride, const float* wp, const float* bias, float* yf, int nchw, uint8_t* yu,
                                  float* logits, int B, int H, int W, void* stream) {
    if (!x || !wp || !bias || (!yf && !yu) || B < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
    if (x_cstride < TAIL_C || x_cstride % 4 || !aligned16(x) || !aligned16(wp)) return (int)hipErrorInvalidValue;
    const int64_t npix = (int64_t)B * H * W;
    const int64_t blocks = (npix + 16 * TAIL_PASSES - 1) / (16 * TAIL_PASSES);
    if (blocks >= (1ll << 31)) return (int)hipErrorInvalidValue;
    const size_t x_bytes = (size_t)npix * x_cstride * 4;
    if ((yf && overlaps(x, x_bytes, yf, (size_t)npix * 12)) || (yu && overlaps(x, x_bytes, yu, (size_t)npix * 3)) ||
        (logits && overlaps(x, x_bytes, logits, (size_t)npix * 12)))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spade_tail_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, x_cstride, wp, bias, yf, nchw ? 1 : 0,
                       yu, logits, H, W, npix);
    E4S_CHECK_LAUNCH();
    return 0;
}
