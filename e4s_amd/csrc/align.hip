// The first and the last link of the face-swap chain on the device: the aligned crop of a face out of a camera frame and the
// paste of the swapped face back into it.
//   e4s_quad_crop_u8          src/utils/alignmengt.py:113-140 crop_image: img.crop(window) ->
//                             img.transform((S, S), Image.QUAD, quad + 0.5, Image.BILINEAR)
//   e4s_perspective_paste_u8  scripts/face_swap.py:313-327: putalpha(255) -> transform(orig.size, Image.PERSPECTIVE, coeffs,
//                             Image.BILINEAR) -> alpha_composite.  The projected alpha is 255 where the back-projected point lies
//                             in the face and 0 elsewhere, so the composite is a select.
// Both are gathers with Pillow's arithmetic (libImaging/Geometry.c: quad_transform, perspective_transform, bilinear_filter32RGB),
// restated in fp64 in Pillow's operation order; the result is truncated to uint8, so one ulp of a coordinate can flip a level
// and fp32 coordinates do (1e-4 .. 6e-4 of the pixels).  Contraction is off: a fused a + b * c rounds once where Pillow rounds twice.
//
// Shape: one 256-thread block per 32 x 32 tile of OUTPUT pixels, a thread makes 4 horizontally adjacent pixels, a wave a 32 x 8
// patch -- under rotation its source footprint stays a patch of a few rows, not a long diagonal.  The 12 bytes of a thread
// leave as three dwords where the address allows (always, when the row pitch is a multiple of 4 bytes), else byte by byte.
// Coefficients and windows are read from device memory: no host synchronisation, a captured graph replays with new quads.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PX = 4;                   // pixels per thread
constexpr int TILE = 32;                // 8 threads x 4 pixels wide, 32 rows

struct u32x3 { uint32_t v[3]; };        // 12 bytes, 4-byte aligned: one global_{load,store}_dwordx3

__device__ __forceinline__ bool in_image(double xin, double yin, int w, int h) {
    return xin >= 0.0 && xin < (double)w && yin >= 0.0 && yin < (double)h;     // (a NaN coordinate is outside)
}

// bilinear_filter32RGB (as r | g << 8 | b << 16) at (xin, yin), which in_image() accepted, of the w x h pixel image at `img`
// whose rows are `pitch` bytes apart
__device__ __forceinline__ uint32_t bilinear_rgb(const uint8_t* img, int64_t pitch, int w, int h, double xin, double yin) {
    xin -= 0.5;
    yin -= 0.5;
    const int x = (int)floor(xin), y = (int)floor(yin);              // -1 .. w - 1, -1 .. h - 1
    const double dx = xin - x, dy = yin - y;
    const int x0 = (x < 0 ? 0 : x) * 3, x1 = (x + 1 > w - 1 ? w - 1 : x + 1) * 3;
    const uint8_t* r0 = img + (int64_t)(y < 0 ? 0 : y) * pitch;
    const uint8_t* r1 = y + 1 < h ? img + (int64_t)(y + 1) * pitch : r0;      // no row below: v2 = v1
    uint32_t rgb = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a0 = r0[x0 + c], b0 = r0[x1 + c], a1 = r1[x0 + c], b1 = r1[x1 + c];
        const double v1 = a0 + (b0 - a0) * dx;
        const double v2 = a1 + (b1 - a1) * dx;
        rgb |= (uint32_t)(int)(v1 + (v2 - v1) * dy) << (8 * c);      // truncated, as Pillow's (UINT8) cast
    }
    return rgb;
}

// four 24-bit pixels <-> the 12 bytes they occupy
__device__ __forceinline__ u32x3 pack12(const uint32_t (&p)[PX]) {
    return u32x3{{p[0] | p[1] << 24, p[1] >> 8 | p[2] << 16, p[2] >> 16 | p[3] << 8}};
}

__device__ __forceinline__ uint32_t unpack12(const u32x3 w, const int p) {
    return p == 0 ? w.v[0] & 0xFFFFFFu : p == 1 ? (w.v[0] >> 24 | w.v[1] << 8) & 0xFFFFFFu
         : p == 2 ? (w.v[1] >> 16 | w.v[2] << 16) & 0xFFFFFFu : w.v[2] >> 8;
}

__device__ __forceinline__ bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

__global__ __launch_bounds__(256) void quad_crop_kernel(const uint8_t* __restrict__ frames, const double* __restrict__ coeffs,
                                                        const int* __restrict__ windows, uint8_t* __restrict__ out,
                                                        float* __restrict__ norm, int H, int W, int S) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * TILE + (threadIdx.x & 7) * PX, y = blockIdx.y * TILE + (threadIdx.x >> 3);
    if (x >= S || y >= S) return;
    const double* a = coeffs + (int64_t)b * 8;
    const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7];
    // Pillow's cropped sub-image; clamped to the frame, so whatever the window array holds no read leaves the frame
    const int wx0 = max(windows[b * 4 + 0], 0), wy0 = max(windows[b * 4 + 1], 0);
    const int w = min(windows[b * 4 + 2], W) - wx0, h = min(windows[b * 4 + 3], H) - wy0;
    const int64_t pitch = (int64_t)W * 3;
    const uint8_t* img = frames + (int64_t)b * H * pitch + (int64_t)wy0 * pitch + (int64_t)wx0 * 3;

    uint32_t px[PX];
    const double yi = y + 0.5;
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        const double xi = (x + p) + 0.5;
        const double xs = a0 + a1 * xi + a2 * yi + a3 * xi * yi;
        const double ys = a4 + a5 * xi + a6 * yi + a7 * xi * yi;
        px[p] = x + p < S && in_image(xs, ys, w, h) ? bilinear_rgb(img, pitch, w, h, xs, ys) : 0u;
    }

    const bool full = x + PX <= S;
    uint8_t* o = out + (((int64_t)b * S + y) * S + x) * 3;
    if (full && aligned4(o)) {
        *reinterpret_cast<u32x3*>(o) = pack12(px);
    } else {
#pragma unroll
        for (int i = 0; i < PX * 3; ++i)                       // (constant indices keep px in registers)
            if (x + i / 3 < S) o[i] = (uint8_t)(px[i / 3] >> (8 * (i % 3)));
    }
    if (norm) {                                    // TO_TENSOR + NORMALIZE(0.5, 0.5): (v / 255 - 0.5) / 0.5, fp32, this order
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* n = norm + (((int64_t)b * 3 + c) * S + y) * S + x;
            f32x4 v;
#pragma unroll
            for (int p = 0; p < PX; ++p) v[p] = ((float)(px[p] >> (8 * c) & 0xFFu) / 255.f - 0.5f) / 0.5f;
            if (full && ((uintptr_t)n & 15) == 0) {
                *reinterpret_cast<f32x4*>(n) = v;
            } else {
#pragma unroll
                for (int p = 0; p < PX; ++p)
                    if (x + p < S) n[p] = v[p];
            }
        }
    }
}

// frames and out may be the same buffer (a thread reads only the pixels it writes), so neither is __restrict__
__global__ __launch_bounds__(256) void perspective_paste_kernel(const uint8_t* __restrict__ faces, const uint8_t* frames,
                                                                const double* __restrict__ coeffs, uint8_t* out, int H, int W,
                                                                int S) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * TILE + (threadIdx.x & 7) * PX, y = blockIdx.y * TILE + (threadIdx.x >> 3);
    if (x >= W || y >= H) return;
    const double* a = coeffs + (int64_t)b * 8;
    const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7];
    const uint8_t* face = faces + (int64_t)b * S * S * 3;
    const bool inplace = frames == out;

    uint32_t px[PX] = {0u, 0u, 0u, 0u};
    unsigned inside = 0;
    const double yi = y + 0.5, lim = (double)(S + 1);
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        const double xi = (x + p) + 0.5;
        const double d = a6 * xi + a7 * yi + 1;
        const double nx = a0 * xi + a1 * yi + a2, ny = a3 * xi + a4 * yi + a5;
        // most of a frame is far from the face: a point more than a pixel outside it (n / d < -1 or > S + 1, a margin 2^50 times
        // the rounding of these products) needs no division.  Everything else, d <= 0 and NaN included, takes Pillow's test.
        const bool far = d > 0.0 && (nx < -d || ny < -d || nx > lim * d || ny > lim * d);
        if (x + p < W && !far) {
            const double xs = nx / d, ys = ny / d;
            if (in_image(xs, ys, S, S)) {
                px[p] = bilinear_rgb(face, (int64_t)S * 3, S, S, xs, ys);
                inside |= 1u << p;
            }
        }
    }
    if (inplace && !inside) return;                          // the frame's own pixels are already there

    const int64_t off = (((int64_t)b * H + y) * W + x) * 3;
    const uint8_t* f = frames + off;
    uint8_t* o = out + off;
    if (x + PX <= W && aligned4(o) && aligned4(f)) {
        if (inside != (1u << PX) - 1) {
            const u32x3 fv = *reinterpret_cast<const u32x3*>(f);
#pragma unroll
            for (int p = 0; p < PX; ++p)
                if (!(inside >> p & 1)) px[p] = unpack12(fv, p);
        }
        *reinterpret_cast<u32x3*>(o) = pack12(px);
    } else {
#pragma unroll
        for (int i = 0; i < PX * 3; ++i) {
            const bool in = inside >> (i / 3) & 1;
            if (x + i / 3 < W && (in || !inplace)) o[i] = in ? (uint8_t)(px[i / 3] >> (8 * (i % 3))) : f[i];
        }
    }
}

inline bool bad_dims(int B, int H, int W, int S) { return B <= 0 || B > 65535 || H <= 0 || W <= 0 || S <= 0; }

}  // namespace

extern "C" int e4s_quad_crop_u8(const uint8_t* frames, const double* coeffs, const int32_t* windows, uint8_t* out, float* normalized,
                                int B, int H, int W, int S, void* stream) {
    if (bad_dims(B, H, W, S) || !frames || !coeffs || !windows || !out) return (int)hipErrorInvalidValue;
    const dim3 grid(cdiv(S, TILE), cdiv(S, TILE), B);
    hipLaunchKernelGGL(quad_crop_kernel, grid, dim3(256), 0, as_stream(stream), frames, coeffs, windows, out, normalized, H, W, S);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_perspective_paste_u8(const uint8_t* faces, const uint8_t* frames, const double* coeffs, uint8_t* out, int B, int H,
                                        int W, int S, void* stream) {
    if (bad_dims(B, H, W, S) || !faces || !frames || !coeffs || !out) return (int)hipErrorInvalidValue;
    const dim3 grid(cdiv(W, TILE), cdiv(H, TILE), B);
    hipLaunchKernelGGL(perspective_paste_kernel, grid, dim3(256), 0, as_stream(stream), faces, frames, coeffs, out, H, W, S);
    E4S_CHECK_LAUNCH();
    return 0;
}
