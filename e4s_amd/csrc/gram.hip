// VGG16 Gram-matrix StyleLoss (src/criteria/style_loss.py:82-221, coach.py:446-450) -- the kernels around the VGG16 convs:
//
//   e4s_style_prep_f32 / _bwd   bilinear resize (align_corners=False) of the NCHW image + ImageNet normalisation + multiplication with the
//                               bilinearly resized mask in ONE streaming pass -> NHWC; the backward is the transpose of that linear map as a
//                               gather over the output pixels that read an image pixel, in (oy, ox) order: deterministic, no float atomics
//   e4s_gram_f32                G = A^T A / (N HW C) with A[p][n C + c] = F[n,p,c] (the reference's view of the batch as ONE [N C, HW] matrix,
//                               cross-sample blocks included).  Both MFMA operands of a k-step are 32 consecutive channels of one pixel: they
//                               come straight from global memory, 128 contiguous bytes per half wave, no LDS, no transpose.  One WAVE owns one
//                               64 x 64 tile of the upper block triangle over one slice of the pixels; the partial tiles go to a workspace
//                               and a second kernel adds the slices in slice order (in fp64), scales and writes G[i][j] and G[j][i] from the SAME sum
//                               (bit-symmetric, two calls bit-identical).  Exact-fp32 MFMA (32x32x2) whatever E4S_PRECISION says: these are
//                               sums of up to 65 536 non-negative products
//   e4s_gram_mse_f32            D = G_x - G_xhat, term = mean(D^2) (ordered: fp32 per thread, fp64 from the wave on), acc (+)= weight * term
//   e4s_gram_grad_f32           dF[n,p,c] (+)= s * sum_j A[p][j] D[j][n C + c], s = coef * gloss[0] read on the device: a [HW x NC].[NC x NC]
//                               GEMM whose K runs ACROSS the samples; one wave per 64 pixels x 64 columns, A as 16-byte runs of one pixel,
//                               D rows as 128-byte runs, both from global memory
#include "common.h"

namespace {

// ATen's area_pixel_compute_source_index for align_corners=False without a scale factor (UpSample.h): scale = in / out in float,
// src = max(scale (d + 0.5) - 0.5, 0), upper neighbour clamped to in - 1.  Forward and backward share this one definition.
__device__ __forceinline__ void bilinear_taps(int d, int in, int out, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
    const float scale = (float)in / (float)out;
    float s = scale * ((float)d + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i0 = i0 < in - 1 ? i0 : in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - (float)i0;
    l0 = 1.f - l1;
}

__device__ __forceinline__ float bilinear_at(const float* __restrict__ pl, int W, int y0, int y1, int x0, int x1, float ly0, float ly1,
                                             float lx0, float lx1) {
#pragma clang fp contract(off)
    const float top = lx0 * pl[(int64_t)y0 * W + x0] + lx1 * pl[(int64_t)y0 * W + x1];
    const float bot = lx0 * pl[(int64_t)y1 * W + x0] + lx1 * pl[(int64_t)y1 * W + x1];
    return ly0 * top + ly1 * bot;
}

struct PrepNorm {
    float mean[3], std[3];
};

__global__ __launch_bounds__(256) void style_prep_kernel(const float* __restrict__ x, const float* __restrict__ mask, float* __restrict__ y,
                                                         int B, int H, int W, int Hm, int Wm, int oh, int ow, int normalize, PrepNorm nm) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * oh * ow) return;
    const int ox = (int)(i % ow), oy = (int)((i / ow) % oh), b = (int)(i / ((int64_t)ow * oh));
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    bilinear_taps(oy, H, oh, y0, y1, ly0, ly1);
    bilinear_taps(ox, W, ow, x0, x1, lx0, lx1);
    float m = 1.f;
    if (mask) {
        int my0, my1, mx0, mx1;
        float a0, a1, c0, c1;
        bilinear_taps(oy, Hm, oh, my0, my1, a0, a1);
        bilinear_taps(ox, Wm, ow, mx0, mx1, c0, c1);
        m = bilinear_at(mask + (int64_t)b * Hm * Wm, Wm, my0, my1, mx0, mx1, a0, a1, c0, c1);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = bilinear_at(x + ((int64_t)b * 3 + c) * H * W, W, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
        if (normalize) v = ((v + 1.f) * 0.5f - nm.mean[c]) / nm.std[c];
        y[i * 3 + c] = mask ? v * m : v;
    }
}

// candidate output rows of input row r: every d whose lower tap is r - 1 or r, i.e. src(d) in [r - 1, r + 1), widened by one on both
// sides against the float rounding of src; the exact membership is decided per d by bilinear_taps itself
__device__ __forceinline__ void prep_bwd_range(int r, int in, int out, int& lo, int& hi) {
    const float inv = (float)out / (float)in;
    lo = (int)floorf(((float)r - 0.5f) * inv - 0.5f) - 1;
    hi = (int)ceilf(((float)r + 1.5f) * inv - 0.5f) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > out - 1 ? out - 1 : hi;
}

__global__ __launch_bounds__(256) void style_prep_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ mask, float* __restrict__ dx,
                                                             int B, int H, int W, int Hm, int Wm, int oh, int ow, int normalize, PrepNorm nm) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * H * W) return;
    const int xx = (int)(i % W), yy = (int)((i / W) % H), b = (int)(i / ((int64_t)W * H));
    int oy_lo, oy_hi, ox_lo, ox_hi;
    prep_bwd_range(yy, H, oh, oy_lo, oy_hi);
    prep_bwd_range(xx, W, ow, ox_lo, ox_hi);
    float g[3] = {0.f, 0.f, 0.f};
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
        int y0, y1;
        float ly0, ly1;
        bilinear_taps(oy, H, oh, y0, y1, ly0, ly1);
        const float wy = (y0 == yy ? ly0 : 0.f) + (y1 == yy ? ly1 : 0.f);
        if (y0 != yy && y1 != yy) continue;
        int my0 = 0, my1 = 0;
        float a0 = 0.f, a1 = 0.f;
        if (mask) bilinear_taps(oy, Hm, oh, my0, my1, a0, a1);
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            int x0, x1;
            float lx0, lx1;
            bilinear_taps(ox, W, ow, x0, x1, lx0, lx1);
            if (x0 != xx && x1 != xx) continue;
            const float wx = (x0 == xx ? lx0 : 0.f) + (x1 == xx ? lx1 : 0.f);
            float wgt = wy * wx;
            if (mask) {
                int mx0, mx1;
                float c0, c1;
                bilinear_taps(ox, Wm, ow, mx0, mx1, c0, c1);
                wgt = wgt * bilinear_at(mask + (int64_t)b * Hm * Wm, Wm, my0, my1, mx0, mx1, a0, a1, c0, c1);
            }
            const float* d = dy + (((int64_t)b * oh + oy) * ow + ox) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = g[c] + wgt * d[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dx[(((int64_t)b * 3 + c) * H + yy) * W + xx] = normalize ? g[c] * (0.5f / nm.std[c]) : g[c];
}

// ---- Gram matrix ------------------------------------------------------------------------------------------------------------------
constexpr int GT = 64;                           // tile side: 2 x 2 MFMA 32x32 blocks per wave

struct GramPlan {
    int T, ntile, nsplit, chunk;                 // tiles per side, tiles of the upper block triangle, pixel slices, pixels per slice (even)
};

// 1024 waves = one per SIMD of 256 CUs.  NC = 128 over 65 536 pixels: 3 tiles x 342 slices of 192 pixels; NC = 1024 over 1 024 pixels: 136
// tiles x 8 slices of 128.  A slice has at least 32 pixels (16 k-steps) unless the map is smaller.
inline GramPlan gram_plan(int N, int HW, int C) {
    GramPlan g;
    g.T = N * C / GT;
    g.ntile = g.T * (g.T + 1) / 2;
    int want = cdiv(1024, g.ntile), most = HW / 32 > 1 ? HW / 32 : 1;
    want = want < most ? want : most;
    g.chunk = (cdiv(HW, want) + 1) & ~1;
    g.nsplit = cdiv(HW, g.chunk);
    return g;
}

__global__ __launch_bounds__(256) void gram_partial_kernel(const float* __restrict__ F, float* __restrict__ ws, int HW, int C, GramPlan g) {
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= g.ntile * g.nsplit) return;      // whole waves leave: no barrier below
    const int tile = wave % g.ntile, split = wave / g.ntile;     // the waves of a block share a pixel slice
    int ti = 0, rem = tile;
    while (rem >= g.T - ti) { rem -= g.T - ti; ++ti; }
    const int tj = ti + rem;
    const int col = lane & 31, kh = lane >> 5;
    const int i0 = ti * GT, j0 = tj * GT;
    const float* Fa = F + (int64_t)(i0 / C) * HW * C + (i0 % C) + col;
    const float* Fb = F + (int64_t)(j0 / C) * HW * C + (j0 % C) + col;
    const int p0 = split * g.chunk, p1 = p0 + g.chunk < HW ? p0 + g.chunk : HW;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    int p = p0;
    for (; p + 8 <= p1; p += 8) {                // 4 k-steps of 2 pixels: 16 loads in flight, then 16 MFMAs
        float a[4][2], b[4][2];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t o = (int64_t)(p + 2 * s + kh) * C;
            a[s][0] = Fa[o]; a[s][1] = Fa[o + 32];
            b[s][0] = Fb[o]; b[s][1] = Fb[o + 32];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][m], b[s][n], acc[m][n], 0, 0, 0);
    }
    for (; p < p1; p += 2) {                     // tail; an odd pixel count leaves the upper half of the last k-pair empty
        const int q = p + kh;
        const bool ok = q < p1;
        const int64_t o = (int64_t)(ok ? q : p) * C;
        const float a0 = ok ? Fa[o] : 0.f, a1 = ok ? Fa[o + 32] : 0.f, b0 = ok ? Fb[o] : 0.f, b1 = ok ? Fb[o + 32] : 0.f;
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    float* out = ws + ((int64_t)split * g.ntile + tile) * (GT * GT);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                out[row * GT + n * 32 + col] = acc[m][n][r];
            }
}

// G[i][j] = G[j][i] = (slice 0 + slice 1 + ...) / denom, read from the upper-triangle entry (min, max) of the partial tiles
__global__ __launch_bounds__(256) void gram_reduce_kernel(const float* __restrict__ ws, float* __restrict__ G, int NC, float denom, GramPlan g) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)NC * NC) return;
    const int i = (int)(e / NC), j = (int)(e % NC);
    const int a = i < j ? i : j, b = i < j ? j : i;
    const int ti = a / GT, tj = b / GT;
    const int tile = ti * g.T - ti * (ti - 1) / 2 + (tj - ti);
    const float* src = ws + (int64_t)tile * (GT * GT) + (a % GT) * GT + (b % GT);
    double s = 0.0;                              // up to 342 slices: added in fp64, so the slicing costs no accuracy; one cast
    for (int k = 0; k < g.nsplit; ++k) s += (double)src[(int64_t)k * g.ntile * (GT * GT)];
    G[e] = (float)s / denom;
}

// ---- MSE of two Gram matrices ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

inline int gram_mse_blocks(int64_t n) {
    const int64_t b = (n + 4095) / 4096;
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

__global__ __launch_bounds__(256) void gram_mse_partial_kernel(const float* __restrict__ gx, const float* __restrict__ gy, float* __restrict__ D,
                                                               double* __restrict__ ws, int64_t n, int64_t chunk) {
    __shared__ double part[4];
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    float s = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const float d = gx[i] - gy[i];
        D[i] = d;
        s += d * d;
    }
    const double w = wave_sum_f64((double)s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) ws[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

__global__ __launch_bounds__(64) void gram_mse_final_kernel(const double* __restrict__ ws, int nblk, int64_t n, float weight, int init,
                                                            float* __restrict__ term, float* __restrict__ acc) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) s += ws[i];
    s = wave_sum_f64(s);
    if (threadIdx.x == 0) {
        const float t = (float)(s / (double)n);
        term[0] = t;
        acc[0] = init ? weight * t : acc[0] + weight * t;
    }
}

// ---- tap gradient -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gram_grad_kernel(const float* __restrict__ F, const float* __restrict__ D, const float* __restrict__ gloss,
                                                        float coef, const float* __restrict__ addend, float* __restrict__ dF, int N, int HW, int C) {
    const int NC = N * C, T = NC / GT, ptiles = (HW + GT - 1) / GT;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= T * ptiles) return;
    const int ct = wave % T, pt = wave / T;      // the waves of a block share 64 pixels (A) and walk different columns of D
    const int row = lane & 31, kh = lane >> 5;
    const int c0 = ct * GT, p0 = pt * GT;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const bool ok0 = p0 + row < HW, ok1 = p0 + 32 + row < HW;
    const int64_t pa0 = (int64_t)(ok0 ? p0 + row : 0) * C, pa1 = (int64_t)(ok1 ? p0 + 32 + row : 0) * C;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < NC; j0 += 8) {         // lane (row, kh) carries k = j0 + 4 kh + s in MFMA step s, on both operands
        const int j = j0 + 4 * kh;
        const float* Fj = F + (int64_t)(j / C) * HW * C + (j % C);
        const f32x4 a0 = ok0 ? *reinterpret_cast<const f32x4*>(Fj + pa0) : zero;
        const f32x4 a1 = ok1 ? *reinterpret_cast<const f32x4*>(Fj + pa1) : zero;
        float b[4][2];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float* Dr = D + (int64_t)(j + s) * NC + c0 + row;
            b[s][0] = Dr[0];
            b[s][1] = Dr[32];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b[s][0], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b[s][1], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b[s][0], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b[s][1], acc[1][1], 0, 0, 0);
        }
    }
    const float s = coef * gloss[0];
    const int64_t base = (int64_t)(c0 / C) * HW * C + (c0 % C) + row;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = p0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (p >= HW) continue;
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int64_t o = base + (int64_t)p * C + n * 32;
                const float v = acc[m][n][r] * s;
                dF[o] = addend ? addend[o] + v : v;
            }
        }
}

inline bool gram_shape_ok(int N, int HW, int C) { return N > 0 && HW > 0 && C > 0 && C % GT == 0 && (int64_t)N * C <= 16384 && (int64_t)N * HW * C < (1ll << 31); }

}  // namespace

static const PrepNorm kImageNet = {{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}};

extern "C" int e4s_style_prep_f32(const float* x, const float* mask, float* y, int B, int H, int W, int Hm, int Wm, int oh, int ow,
                                  int normalize, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0 || (mask && (Hm <= 0 || Wm <= 0))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(style_prep_kernel, grid1((int64_t)B * oh * ow), dim3(256), 0, as_stream(stream), x, mask, y, B, H, W, Hm, Wm, oh, ow,
                       normalize, kImageNet);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_style_prep_bwd_f32(const float* dy, const float* mask, float* dx, int B, int H, int W, int Hm, int Wm, int oh, int ow,
                                      int normalize, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0 || (mask && (Hm <= 0 || Wm <= 0))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(style_prep_bwd_kernel, grid1((int64_t)B * H * W), dim3(256), 0, as_stream(stream), dy, mask, dx, B, H, W, Hm, Wm, oh, ow,
                       normalize, kImageNet);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t e4s_gram_ws_floats(int N, int HW, int C) {
    if (!gram_shape_ok(N, HW, C)) return 0;
    const GramPlan g = gram_plan(N, HW, C);
    return (int64_t)g.nsplit * g.ntile * GT * GT;
}

extern "C" int e4s_gram_f32(const float* F, float* G, float* ws, int N, int HW, int C, void* stream) {
    if (!gram_shape_ok(N, HW, C)) return (int)hipErrorInvalidValue;
    const GramPlan g = gram_plan(N, HW, C);
    const int NC = N * C;
    hipLaunchKernelGGL(gram_partial_kernel, dim3((unsigned)cdiv((int64_t)g.ntile * g.nsplit, 4)), dim3(256), 0, as_stream(stream), F, ws, HW, C, g);
    E4S_CHECK_LAUNCH();
    hipLaunchKernelGGL(gram_reduce_kernel, grid1((int64_t)NC * NC), dim3(256), 0, as_stream(stream), ws, G, NC, (float)((int64_t)N * HW * C), g);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t e4s_gram_mse_ws_doubles(int64_t n) { return n > 0 ? gram_mse_blocks(n) : 0; }

extern "C" int e4s_gram_mse_f32(const float* gx, const float* gy, float* D, float* term, float* acc, float weight, int init, double* ws,
                                int64_t n, void* stream) {
    if (n <= 0) return (int)hipErrorInvalidValue;
    const int nblk = gram_mse_blocks(n);
    const int64_t chunk = (n + nblk - 1) / nblk;
    hipLaunchKernelGGL(gram_mse_partial_kernel, dim3(nblk), dim3(256), 0, as_stream(stream), gx, gy, D, ws, n, chunk);
    E4S_CHECK_LAUNCH();
    hipLaunchKernelGGL(gram_mse_final_kernel, dim3(1), dim3(64), 0, as_stream(stream), ws, nblk, n, weight, init, term, acc);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_gram_grad_f32(const float* F, const float* D, const float* gloss, float coef, const float* addend, float* dF, int N,
                                 int HW, int C, void* stream) {
    if (!gram_shape_ok(N, HW, C) || !aligned16(F)) return (int)hipErrorInvalidValue;
    const int64_t waves = (int64_t)(N * C / GT) * cdiv(HW, GT);
    hipLaunchKernelGGL(gram_grad_kernel, dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, as_stream(stream), F, D, gloss, coef, addend, dF, N, HW, C);
    E4S_CHECK_LAUNCH();
    return 0;
}
