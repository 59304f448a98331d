// Pasting GPEN's restored faces back into a frame (e4s_amd/face_paste.py; src/pretrained/gpen/face_enhancement.py:44-49, 68-108):
// the mask post-processing, cv2.warpAffine, cv2.filter2D with the 3x3 binomial kernel, and the merge and blend of the faces.
//
// cv2 is not a dependency: the kernels restate OpenCV's published algorithms (imgwarp.cpp, smooth / filter), as csrc/stitch.hip does.
//   warpAffine(flags=3: INTER_AREA, which warpAffine turns into INTER_LINEAR; constant border 0).  The caller passes the INVERSE map
//     A = [a00 a01 b0; a10 a11 b1] in double.  Column x: adelta = cvRound(a00 x 1024), bdelta = cvRound(a10 x 1024); row y:
//     X0 = cvRound((a01 y + b0) 1024) + 16, Y0 likewise; X = (X0 + adelta) >> 5: integer part X >> 5, fraction X & 31 (1/32 pixel).
//     uint8: integer weights (32 - fx)(32 - fy) 32 .. (they sum to 32768), result (sum + 16384) >> 15.  fp32: float weights
//     (1 - fy/32)(1 - fx/32) .., summed tap 0 to 3.  Taps outside the source read 0.  cvRound is round-half-to-even on doubles.
//   GaussianBlur is separable: rows, then columns, float taps, fp32 accumulation in tap order, BORDER_REFLECT_101.
//   filter2D([1 2 1] x [1 2 1] / 16) on uint8, BORDER_REFLECT_101: the sum is an exact integer, rounded half to even.
//   merge and blend: per pixel over the faces in order, a face takes the pixel where its mask exceeds the running mask; then
//     convertScaleAbs(bg (1 - m) + face m) in fp32, in that order: |.|, round half to even, saturate.
#include "common.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

__device__ __forceinline__ int cv_round(double v) { return (int)rint(v); }

// one thread per destination pixel; C channels of T
template <typename T, int C>
__global__ __launch_bounds__(256) void warp_affine_kernel(const T* __restrict__ src, T* __restrict__ dst, int Hs, int Ws, int Hd, int Wd,
                                                          double a00, double a01, double b0, double a10, double a11, double b1) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= Wd || y >= Hd) return;
    const int adelta = cv_round(a00 * x * 1024.0), bdelta = cv_round(a10 * x * 1024.0);
    const int X0 = cv_round((a01 * y + b0) * 1024.0) + 16, Y0 = cv_round((a11 * y + b1) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
    const bool x0 = (unsigned)sx < (unsigned)Ws, x1 = (unsigned)(sx + 1) < (unsigned)Ws;
    const bool y0 = (unsigned)sy < (unsigned)Hs, y1 = (unsigned)(sy + 1) < (unsigned)Hs;
    const size_t o00 = ((size_t)sy * Ws + sx) * C;
    T* d = dst + ((size_t)y * Wd + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const T p0 = (y0 && x0) ? src[o00 + c] : (T)0, p1 = (y0 && x1) ? src[o00 + C + c] : (T)0;
        const T p2 = (y1 && x0) ? src[o00 + (size_t)Ws * C + c] : (T)0, p3 = (y1 && x1) ? src[o00 + (size_t)Ws * C + C + c] : (T)0;
        if constexpr (sizeof(T) == 1) {
            const int w0 = (32 - fx) * (32 - fy) * 32, w1 = fx * (32 - fy) * 32, w2 = (32 - fx) * fy * 32, w3 = fx * fy * 32;
            d[c] = (T)((w0 * (int)p0 + w1 * (int)p1 + w2 * (int)p2 + w3 * (int)p3 + 16384) >> 15);
        } else {
            const float cx1 = fx * (1.f / 32), cx0 = 1.f - cx1, cy1 = fy * (1.f / 32), cy0 = 1.f - cy1;
            d[c] = p0 * (cy0 * cx0) + p1 * (cy0 * cx1) + p2 * (cy1 * cx0) + p3 * (cy1 * cx1);
        }
    }
}

// mask / 255 as fp32 with a frame of `thres` pixels zeroed (face_enhancement.py:45-46)
__global__ __launch_bounds__(256) void mask_prep_kernel(const uint8_t* __restrict__ m, float* __restrict__ out, int H, int W, int thres,
                                                        int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const bool frame = y < thres || y >= H - thres || x < thres || x >= W - thres;
    out[i] = frame ? 0.f : (float)m[i] / 255.f;
}

// one 1-D pass of a separable filter over [B,H,W]: axis 1 = along x (rows), 0 = along y (columns); K taps, BORDER_REFLECT_101
__global__ __launch_bounds__(256) void blur_pass_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ taps,
                                                        int K, int H, int W, int axis, int64_t n) {
    extern __shared__ float st[];
    for (int k = threadIdx.x; k < K; k += 256) st[k] = taps[k];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const float* img = in + (i - ((int64_t)y * W + x));
    const int r = K / 2;
    float acc = 0.f;
    if (axis) {
        for (int k = 0; k < K; ++k) acc += st[k] * img[(int64_t)y * W + reflect101(x + k - r, W)];
    } else {
        for (int k = 0; k < K; ++k) acc += st[k] * img[(int64_t)reflect101(y + k - r, H) * W + x];
    }
    out[i] = acc;
}

// [1 2 1] x [1 2 1] / 16 on uint8 [B,H,W,C], BORDER_REFLECT_101, round half to even
__global__ __launch_bounds__(256) void binomial3_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W, int C,
                                                        int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const int x = (int)((i / C) % W), y = (int)((i / ((int64_t)C * W)) % H);
    const uint8_t* img = in + (i - (((int64_t)y * W + x) * C + c));
    int s = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = reflect101(y + dy, H);
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = reflect101(x + dx, W);
            s += (2 - (dy != 0)) * (2 - (dx != 0)) * (int)img[((int64_t)yy * W + xx) * C + c];
        }
    }
    const int q = s >> 4, r = s & 15;
    out[i] = (uint8_t)(q + ((r > 8 || (r == 8 && (q & 1))) ? 1 : 0));
}

// masks [n,H,W] fp32, faces [n,H,W,3] uint8, bg / out [H,W,3] uint8 (out may be bg)
__global__ __launch_bounds__(256) void merge_blend_kernel(const float* __restrict__ masks, const uint8_t* __restrict__ faces,
                                                          const uint8_t* bg, uint8_t* out, int nfaces, int64_t npix) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    float m = 0.f;
    int who = -1;
    for (int f = 0; f < nfaces; ++f) {
        const float t = masks[f * npix + i];
        if (t - m > 0.f) {
            m = t;
            who = f;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float fv = who >= 0 ? (float)faces[((int64_t)who * npix + i) * 3 + c] : 0.f;
        const float v = (float)bg[i * 3 + c] * (1.f - m) + fv * m;
        const float r = rintf(fabsf(v));
        out[i * 3 + c] = (uint8_t)(r > 255.f ? 255.f : r);
    }
}

}  // namespace

extern "C" int e4s_warp_affine(const void* src, void* dst, int is_f32, int Hs, int Ws, int Hd, int Wd, double a00, double a01,
                               double b0, double a10, double a11, double b1, void* stream) {
    if (!src || !dst || src == dst || Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1 || Hs > 32767 || Ws > 32767 || Hd > 32767 || Wd > 32767)
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)cdiv(Wd, 64), (unsigned)cdiv(Hd, 4));
    if (is_f32) hipLaunchKernelGGL((warp_affine_kernel<float, 1>), grid, dim3(256), 0, as_stream(stream), static_cast<const float*>(src),
                                   static_cast<float*>(dst), Hs, Ws, Hd, Wd, a00, a01, b0, a10, a11, b1);
    else hipLaunchKernelGGL((warp_affine_kernel<uint8_t, 3>), grid, dim3(256), 0, as_stream(stream), static_cast<const uint8_t*>(src),
                            static_cast<uint8_t*>(dst), Hs, Ws, Hd, Wd, a00, a01, b0, a10, a11, b1);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_mask_prep_f32(const uint8_t* mask, float* out, int B, int H, int W, int thres, void* stream) {
    if (!mask || !out || B < 1 || H < 1 || W < 1 || thres < 0) return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)B * H * W;
    if ((n + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), mask, out, H, W, thres, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_blur_pass_f32(const float* in, float* out, const float* taps, int K, int B, int H, int W, int axis, void* stream) {
    if (!in || !out || in == out || !taps || K < 1 || K > 1023 || !(K & 1) || B < 1 || H < 1 || W < 1 || (axis != 0 && axis != 1))
        return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)B * H * W;
    if ((n + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(blur_pass_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), K * sizeof(float), as_stream(stream), in, out, taps,
                       K, H, W, axis, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_binomial3_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int C, void* stream) {
    if (!in || !out || in == out || B < 1 || H < 1 || W < 1 || C < 1) return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)B * H * W * C;
    if ((n + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(binomial3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), in, out, H, W, C, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_merge_blend_u8(const float* masks, const uint8_t* faces, const uint8_t* bg, uint8_t* out, int nfaces, int H, int W,
                                  void* stream) {
    if (!bg || !out || nfaces < 0 || (nfaces > 0 && (!masks || !faces)) || H < 1 || W < 1) return (int)hipErrorInvalidValue;
    const int64_t npix = (int64_t)H * W;
    if ((npix + 255) / 256 >= (1ll << 31) || (int64_t)nfaces * npix * 3 >= (1ll << 40)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(merge_blend_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, as_stream(stream), masks, faces, bg, out,
                       nfaces, npix);
    E4S_CHECK_LAUNCH();
    return 0;
}
