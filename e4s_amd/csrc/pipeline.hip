// The joins of the face-swap pipeline (e4s_amd/pipeline.py) that had no native form: what scripts/face_swap.py does between its
// stages in numpy / skimage / cv2 / torchvision, each as one streaming kernel.
//   e4s_resize_aa4_u8_f32  face_swap.py:194   skimage.transform.resize(im / 255.0, (256, 256)) of a 1024^2 crop: scikit-image 0.20
//                                             for an exact factor of 4 = a Gaussian (sigma 1.5, truncate 4, 'mirror') followed by
//                                             the order-1 zoom whose samples fall half way between input pixels 4i+1 and 4i+2:
//                                             per axis 14 taps t[k] = (g[k] + g[k-1]) / 2 at inputs 4i-5 .. 4i+8, mirrored
//   e4s_driven_seam_f32    face_swap.py:204   (pred * 255).astype(np.uint8): the fp32 product TRUNCATED, and pred[:, :, ::-1];
//                          face_enhancement.py:66  cv2.resize(img, img_sr.shape[:2][::-1]): OpenCV's 8-bit INTER_LINEAR (resize.cpp
//                                             HResizeLinear / VResizeLinear, 11-bit coefficients), which is NOT the correctly
//                                             rounded bilinear value
//   e4s_face_to_net_u8     face_swap.py:209, 224-225  drivens[0][:, :, ::-1] and ToTensor + Normalize(0.5, 0.5)
// All are a few MB per image and launch-bound; they are written for whole-dword traffic, not tuned further.  skimage and cv2 are
// restated from their sources (neither library is a dependency); DESIGN.md 3.23.
#include <math.h>
#include "common.h"

namespace {

struct u32x3 { uint32_t v[3]; };        // 12 bytes, 4-byte aligned: four 24-bit pixels
__device__ __forceinline__ bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
__device__ __forceinline__ u32x3 pack12(const uint32_t (&p)[4]) {
    return u32x3{{p[0] | p[1] << 24, p[1] >> 8 | p[2] << 16, p[2] >> 16 | p[3] << 8}};
}

// ---- e4s_resize_aa4_u8_f32 -----------------------------------------------------------------------------------------------
constexpr int RT = 16;                       // output tile side
constexpr int RTAPS = 14;
constexpr int RHALO = 4 * (RT - 1) + RTAPS;  // 74: input rows / columns 4 t0 - 5 .. 4 t0 + 68 of a tile that starts at output t0
constexpr int RPITCH = 224;                  // bytes per staged row: one lead byte + 74 x 3, as 56 dwords
constexpr int RROW = RT * 3;                 // 48 floats of a tile's output row

struct AaTaps { float t[RTAPS]; };

// scipy.ndimage 'mirror' (d c b | a b c d | c b a); one reflection suffices for n >= 8.  The final clamp only serves halo entries
// that no output inside the image reads (tiles that overhang the right / lower edge).
__device__ __forceinline__ int mirror(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// One block per 16 x 16 output tile: the 74 x 74 x 3 uint8 halo goes to LDS (whole dwords where the tile lies inside the image: the
// halo's first byte sits at 12 ox0 - 15 of a row whose pitch is a multiple of 12, so one byte earlier is dword aligned), the
// horizontal pass leaves 74 x 48 fp32 values in [0,1], the vertical pass reads those four floats at a time.  Channels never mix and sit
// 3 apart on both sides, so both passes run over the 48 floats of an output row without telling them apart.
__global__ __launch_bounds__(256) void resize_aa4_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int H, int W,
                                                         const AaTaps taps, int src_dwords) {
    __shared__ __attribute__((aligned(16))) uint8_t halo[RHALO * RPITCH];
    __shared__ __attribute__((aligned(16))) float hbuf[RHALO * RROW];
    const int Ho = H >> 2, Wo = W >> 2;
    const int b = blockIdx.z, ox0 = blockIdx.x * RT, oy0 = blockIdx.y * RT;
    const int ix0 = 4 * ox0 - 5, iy0 = 4 * oy0 - 5;
    const uint8_t* img = src + (int64_t)b * H * W * 3;
    const int tid = threadIdx.x;

    // columns need no mirror: 56 aligned dwords per row, the last of which ends with the first byte of column ix0 + 74 (hence <)
    if (src_dwords && ix0 >= 1 && ix0 + RHALO < W) {
        for (int i = tid; i < RHALO * (RPITCH / 4); i += 256) {
            const int r = i / (RPITCH / 4), j = i % (RPITCH / 4);
            const uint8_t* row = img + ((int64_t)mirror(iy0 + r, H) * W + ix0) * 3 - 1;
            reinterpret_cast<uint32_t*>(halo)[r * (RPITCH / 4) + j] = reinterpret_cast<const uint32_t*>(row)[j];
        }
    } else {
        for (int i = tid; i < RHALO * RHALO * 3; i += 256) {
            const int r = i / (RHALO * 3), cb = i % (RHALO * 3);
            halo[r * RPITCH + 1 + cb] = img[((int64_t)mirror(iy0 + r, H) * W + mirror(ix0 + cb / 3, W)) * 3 + cb % 3];
        }
    }
    __syncthreads();

    for (int i = tid; i < RHALO * RROW; i += 256) {
        const int r = i / RROW, f = i % RROW;
        const uint8_t* p = halo + r * RPITCH + 1 + 12 * (f / 3) + f % 3;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < RTAPS; ++k) acc += taps.t[k] * (float)p[3 * k];
        hbuf[i] = acc / 255.f;
    }
    __syncthreads();

    if (tid >= RT * (RROW / 4)) return;
    const int oy = tid / (RROW / 4), f0 = 4 * (tid % (RROW / 4));
    if (oy0 + oy >= Ho) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < RTAPS; ++k) acc += taps.t[k] * *reinterpret_cast<const f32x4*>(hbuf + (4 * oy + k) * RROW + f0);
    const int valid = min(RT, Wo - ox0) * 3;                     // floats of this row that lie inside the image
    float* o = dst + (((int64_t)b * Ho + oy0 + oy) * Wo + ox0) * 3 + f0;
    if (f0 + 4 <= valid && ((uintptr_t)o & 15) == 0) {
        *reinterpret_cast<f32x4*>(o) = acc;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (f0 + j < valid) o[j] = acc[j];
    }
}

AaTaps aa4_taps() {
    // scipy.ndimage._gaussian_kernel1d(sigma 1.5, order 0, radius int(4.0 * 1.5 + 0.5) = 6), then the half-way average of the zoom
    double g[13], sum = 0.0;
    for (int k = 0; k < 13; ++k) sum += g[k] = exp(-0.5 / (1.5 * 1.5) * (double)((k - 6) * (k - 6)));
    AaTaps t;
    for (int k = 0; k < RTAPS; ++k) t.t[k] = (float)(0.5 * ((k < 13 ? g[k] : 0.0) + (k > 0 ? g[k - 1] : 0.0)) / sum);
    return t;
}

// ---- e4s_driven_seam_f32 -------------------------------------------------------------------------------------------------
constexpr int SW = 32, SH = 8;               // source pixels per block (-> 128 x 32 enlarged pixels)
constexpr int SLW = SW + 2, SLH = SH + 2;    // with the one-pixel ring the interpolation reads

// OpenCV resize.cpp, INTER_LINEAR, scale 1/4: fx = (d + 0.5) / 4 - 0.5, sx = floor(fx), fx -= sx; sx < 0: (0, 0); sx >= n - 1:
// (n - 1, 0); coefficient of the second sample = saturate_cast<short>(fx * 2048), of the first 2048 minus it.  For d = 4 q + phase
// the fractions are 5/8, 7/8, 1/8, 3/8, all exact.
__device__ __forceinline__ void cv_linear_x4(int d, int n, int& s, int& c1) {
    const int ph = d & 3;
    s = (d >> 2) - (ph < 2 ? 1 : 0);
    c1 = ph == 0 ? 1280 : ph == 1 ? 1792 : ph == 2 ? 256 : 768;
    if (s < 0) { s = 0; c1 = 0; }
    if (s >= n - 1) { s = n - 1; c1 = 0; }
}

// One block per 32 x 8 source pixels: they and their ring are truncated to uint8 BGR into LDS (clamped at the image's edge, where the
// rule above gives the ring weight 0), the interior leaves as output 1, then every thread makes four groups of 4 enlarged pixels
// (12 bytes, three dwords; a row of the enlarged image is 12 w bytes, always whole dwords).
__global__ __launch_bounds__(256) void driven_seam_kernel(const float* __restrict__ pred, uint8_t* __restrict__ out,
                                                          uint8_t* __restrict__ big, int h, int w, int out_dwords, int big_dwords) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(4))) uint8_t px[SLH * SLW * 3];
    const int n = blockIdx.z, x0 = blockIdx.x * SW, y0 = blockIdx.y * SH;
    const int tid = threadIdx.x;
    const float* p = pred + (int64_t)n * 3 * h * w;
    for (int i = tid; i < 3 * SLH * SLW; i += 256) {
        const int c = i / (SLH * SLW), r = i / SLW % SLH, col = i % SLW;
        const int y = min(max(y0 + r - 1, 0), h - 1), x = min(max(x0 + col - 1, 0), w - 1);
        const int v = (int)(p[((int64_t)c * h + y) * w + x] * 255.f);              // numpy's astype: towards zero
        px[(r * SLW + col) * 3 + (2 - c)] = (uint8_t)min(max(v, 0), 255);          // (in range for p in [0,1]; RGB -> BGR)
    }
    __syncthreads();

    uint8_t* o = out + ((int64_t)n * h * w) * 3;
    if (out_dwords && x0 + SW <= w) {                                              // 24 dwords per tile row
        if (tid < SH * (SW * 3 / 4)) {
            const int r = tid / (SW * 3 / 4), j = tid % (SW * 3 / 4);
            if (y0 + r < h) {
                const uint8_t* s = px + ((r + 1) * SLW + 1) * 3 + 4 * j;
                reinterpret_cast<uint32_t*>(o + ((int64_t)(y0 + r) * w + x0) * 3)[j] =
                    s[0] | s[1] << 8 | s[2] << 16 | (uint32_t)s[3] << 24;
            }
        }
    } else {
        for (int i = tid; i < SH * SW * 3; i += 256) {
            const int r = i / (SW * 3), cb = i % (SW * 3);
            if (y0 + r < h && x0 + cb / 3 < w) o[((int64_t)(y0 + r) * w + x0) * 3 + cb] = px[((r + 1) * SLW + 1) * 3 + cb];
        }
    }
    if (!big) return;

    const int gx = tid & 31;                                                       // group of 4 enlarged pixels: columns 4 (x0 + gx) ..
    if (x0 + gx >= w) return;
    int sx[4], a1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        cv_linear_x4(4 * (x0 + gx) + q, w, sx[q], a1[q]);
        sx[q] -= x0 - 1;                                                           // -> column of px (the second sample: + 1, staged clamped)
    }
    uint8_t* bigimg = big + (int64_t)n * 16 * h * w * 3;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int dy = 4 * y0 + (tid >> 5) + 8 * it;
        if (dy >= 4 * h) break;
        int sy, b1;
        cv_linear_x4(dy, h, sy, b1);
        const int b0 = 2048 - b1;
        const uint8_t* r0 = px + (sy - (y0 - 1)) * SLW * 3;
        const uint8_t* r1 = r0 + SLW * 3;
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int a0 = 2048 - a1[q];
            uint32_t pix = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int S0 = r0[sx[q] * 3 + c] * a0 + r0[sx[q] * 3 + 3 + c] * a1[q];     // HResizeLinear: int32, 11 fraction bits
                const int S1 = r1[sx[q] * 3 + c] * a0 + r1[sx[q] * 3 + 3 + c] * a1[q];
                pix |= (uint32_t)((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2) << (8 * c);   // VResizeLinear
            }
            v[q] = pix;
        }
        uint8_t* d = bigimg + ((int64_t)dy * 4 * w + 4 * (x0 + gx)) * 3;
        if (big_dwords) {
            *reinterpret_cast<u32x3*>(d) = pack12(v);
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) d[i] = (uint8_t)(v[i / 3] >> (8 * (i % 3)));
        }
    }
}

// ---- e4s_face_to_net_u8 --------------------------------------------------------------------------------------------------
// A thread takes four consecutive pixels of one image: 12 bytes in, 12 bytes out (RGB), three float4 out (one per plane).
__global__ __launch_bounds__(256) void face_to_net_kernel(const uint8_t* __restrict__ src, int bgr, uint8_t* __restrict__ rgb,
                                                          float* __restrict__ net, int64_t npix, int64_t groups, int64_t total) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / groups, p0 = (i % groups) * 4;
    const int cnt = (int)min((int64_t)4, npix - p0);
    const uint8_t* s = src + (b * npix + p0) * 3;
    uint32_t px[4] = {0u, 0u, 0u, 0u};
    if (cnt == 4 && aligned4(s)) {
        const u32x3 w = *reinterpret_cast<const u32x3*>(s);
        px[0] = w.v[0] & 0xFFFFFFu;
        px[1] = (w.v[0] >> 24 | w.v[1] << 8) & 0xFFFFFFu;
        px[2] = (w.v[1] >> 16 | w.v[2] << 16) & 0xFFFFFFu;
        px[3] = w.v[2] >> 8;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < cnt) px[q] = s[q * 3] | s[q * 3 + 1] << 8 | (uint32_t)s[q * 3 + 2] << 16;
    }
    if (bgr) {
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = (px[q] & 0xFF00u) | px[q] >> 16 | (px[q] & 0xFFu) << 16;
    }
    if (rgb) {
        uint8_t* o = rgb + (b * npix + p0) * 3;
        if (cnt == 4 && aligned4(o)) {
            *reinterpret_cast<u32x3*>(o) = pack12(px);
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j)
                if (j / 3 < cnt) o[j] = (uint8_t)(px[j / 3] >> (8 * (j % 3)));
        }
    }
    if (net) {                                  // ToTensor + Normalize(0.5, 0.5) as align.hip's quad crop states it: (v / 255 - 0.5) / 0.5
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* o = net + (b * 3 + c) * npix + p0;
            f32x4 v;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = ((float)(px[q] >> (8 * c) & 0xFFu) / 255.f - 0.5f) / 0.5f;
            if (cnt == 4 && ((uintptr_t)o & 15) == 0) {
                *reinterpret_cast<f32x4*>(o) = v;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < cnt) o[q] = v[q];
            }
        }
    }
}

}  // namespace

extern "C" int e4s_resize_aa4_u8_f32(const uint8_t* src, float* dst, int B, int H, int W, void* stream) {
    if (!src || !dst || B <= 0 || B > 65535 || H < 8 || W < 8 || (H & 3) || (W & 3) || H > (1 << 20) || W > (1 << 20))
        return (int)hipErrorInvalidValue;
    static const AaTaps taps = aa4_taps();
    const dim3 grid(cdiv(W / 4, RT), cdiv(H / 4, RT), B);
    if (grid.y > 65535) return (int)hipErrorInvalidValue;
    // W % 4 == 0 makes every row and every image start a whole number of dwords after src
    hipLaunchKernelGGL(resize_aa4_kernel, grid, dim3(256), 0, as_stream(stream), src, dst, H, W, taps, ((uintptr_t)src & 3) == 0 ? 1 : 0);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_driven_seam_f32(const float* pred, uint8_t* out_u8, uint8_t* enlarged_u8, int N, int h, int w, void* stream) {
    if (!pred || !out_u8 || N <= 0 || N > 65535 || h <= 0 || w <= 0 || h > (1 << 16) || w > (1 << 16)) return (int)hipErrorInvalidValue;
    const dim3 grid(cdiv(w, SW), cdiv(h, SH), N);
    if (grid.y > 65535) return (int)hipErrorInvalidValue;
    const int out_dwords = ((uintptr_t)out_u8 & 3) == 0 && (w & 3) == 0;           // rows of 3 w bytes
    const int big_dwords = ((uintptr_t)enlarged_u8 & 3) == 0;                      // rows of 12 w bytes
    hipLaunchKernelGGL(driven_seam_kernel, grid, dim3(256), 0, as_stream(stream), pred, out_u8, enlarged_u8, h, w, out_dwords, big_dwords);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_face_to_net_u8(const uint8_t* src, int bgr, uint8_t* rgb_u8, float* net_f32, int B, int H, int W, void* stream) {
    if (!src || (!rgb_u8 && !net_f32) || B <= 0 || H <= 0 || W <= 0) return (int)hipErrorInvalidValue;
    const int64_t npix = (int64_t)H * W, groups = (npix + 3) / 4, total = groups * B;
    if ((total + 255) / 256 > 0x7FFFFFFF) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(face_to_net_kernel, grid1(total), dim3(256), 0, as_stream(stream), src, bgr ? 1 : 0, rgb_u8, net_f32, npix, groups,
                       total);
    E4S_CHECK_LAUNCH();
    return 0;
}
