// Pillow's Image.resize of 8-bit RGB images (libImaging/Resample.c, ImagingResample's 8-bit path) on the device, bit for bit:
// a horizontal pass into a uint8 intermediate, then a vertical pass, both in int32 with 22 fractional bits.  The coefficient
// tables (bounds [out,2] = {first input index, number of taps}, kk [out,ksize]) come from the host (e4s_amd/resize.py builds them
// in float64, as Pillow does) and are read from device memory, so a repeated geometry is launches only.
//   value = clamp((2^21 + sum_x pixel[xmin + x] * kk[x]) >> 22, 0, 255)       (arithmetic shift; channels independent)
// 255 * sum|kk| stays below 2^31 for every filter (the taps sum to 2^22, LANCZOS' absolute sum is below 1.5 x 2^22).
//
//   e4s_pil_resample_h_u8   one block = RH input rows x TX output pixels.  The span of input pixels those TX outputs read is
//                           staged into LDS row by row with 16-byte loads (the chunks at either end of the tensor byte by
//                           byte), then a thread makes 4 adjacent output pixels from LDS bytes and stores 12 bytes as three dwords.
//                           Only the output columns of the window and the input rows the vertical pass will read are made.
//   e4s_pil_resample_v_u8   a byte-column job: a thread owns 16 consecutive bytes of one output row and walks the taps' rows with
//                           one 16-byte load each (lanes side by side: a wave reads 1 KiB of a row); the row is wave-uniform, so
//                           its bounds and taps are scalar loads.  The intermediate's pitch is a multiple of 16 bytes.
// Whatever the tables hold, no access leaves the buffers: per output pixel the tap range is clipped to what was staged (h) or to
// the rows of the intermediate (v).
#include "common.h"

namespace {

constexpr int PX = 4;                       // output pixels per thread (h)
constexpr int RH = 8;                       // rows per block (h)
constexpr int PRECISION_BITS = 32 - 8 - 2;  // Pillow's
constexpr int LDS_LIMIT = 64 * 1024;

struct u32x3 { uint32_t v[3]; };

__device__ __forceinline__ uint32_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// img: [B,H,W,3]; makes dst[b][r][(x - x0) * 3 + c] for rows r = 0 .. rows - 1 (input row ry0 + r) and output columns x0 .. x1 - 1
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ img, int H, int W, const int* __restrict__ bounds,
                                                         const int* __restrict__ kk, int ksize, int x0, int x1, int ry0, int rows,
                                                         uint8_t* __restrict__ dst, int64_t dst_pitch, int64_t dst_bstride, int tx,
                                                         int rh, int span, int lds_pitch, int64_t total_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t tile[];
    const int b = blockIdx.z;
    const int tw = tx / PX;                                       // threads across
    const int xt = x0 + blockIdx.x * tx;                          // first output pixel of the tile
    const int xl = min(xt + tx, x1) - 1;                          // last one
    const int r0 = blockIdx.y * rh;
    const int nthreads = tw * rh;
    // the input pixels [lo, hi) the tile reads; at most `span` of them are staged
    int lo = bounds[2 * xt], hi = bounds[2 * xl] + bounds[2 * xl + 1];
    lo = min(max(lo, 0), W - 1);
    hi = min(min(max(hi, lo + 1), W), lo + span);
    const int nbytes = (hi - lo) * 3;
    const int chunks = lds_pitch >> 4;
    const uintptr_t begin = (uintptr_t)img, end = begin + (uintptr_t)total_bytes;
    for (int i = threadIdx.x; i < rh * chunks; i += nthreads) {
        const int r = i / chunks, c = i - r * chunks;
        if (r0 + r >= rows) continue;
        const uintptr_t g = begin + (uintptr_t)((((int64_t)b * H + ry0 + r0 + r) * W + lo) * 3);
        const uintptr_t a = (g & ~(uintptr_t)15) + (uintptr_t)c * 16;
        if (a >= g + nbytes) continue;
        uint4 v;
        if (a >= begin && a + 16 <= end) {
            v = *reinterpret_cast<const uint4*>(a);
        } else {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (a + j >= begin && a + j < end) w[j >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(a + j) << (8 * (j & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(tile + r * lds_pitch + c * 16) = v;
    }
    __syncthreads();

    const int r = threadIdx.x / tw, x = xt + (threadIdx.x - r * tw) * PX;
    if (r0 + r >= rows || x >= x1) return;
    const uintptr_t g = begin + (uintptr_t)((((int64_t)b * H + ry0 + r0 + r) * W + lo) * 3);
    const uint8_t* row = tile + r * lds_pitch + (int)(g & 15);
    uint32_t px[PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        px[p] = 0u;
        if (x + p >= x1) continue;
        int xmin = bounds[2 * (x + p)], n = bounds[2 * (x + p) + 1];
        xmin = min(max(xmin - lo, 0), hi - lo);                   // clipped to what is staged
        n = min(min(n, ksize), hi - lo - xmin);
        const int* k = kk + (int64_t)(x + p) * ksize;
        const uint8_t* s = row + xmin * 3;
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < n; ++t) {
            const int w = k[t];
            a0 += (int)s[3 * t] * w;
            a1 += (int)s[3 * t + 1] * w;
            a2 += (int)s[3 * t + 2] * w;
        }
        px[p] = clip8(a0) | clip8(a1) << 8 | clip8(a2) << 16;
    }
    uint8_t* o = dst + (int64_t)b * dst_bstride + (int64_t)(r0 + r) * dst_pitch + (int64_t)(x - x0) * 3;
    if (x + PX <= x1 && ((uintptr_t)o & 3) == 0) {
        *reinterpret_cast<u32x3*>(o) = u32x3{{px[0] | px[1] << 24, px[1] >> 8 | px[2] << 16, px[2] >> 16 | px[3] << 8}};
    } else {
#pragma unroll
        for (int i = 0; i < PX * 3; ++i)
            if (x + i / 3 < x1) o[i] = (uint8_t)(px[i / 3] >> (8 * (i % 3)));
    }
}

// src: [B,rows,pitch] bytes (pitch a multiple of 16, base 16-byte aligned) whose row r is row ry0 + r of the horizontally resampled
// image; makes out[b][y - y0][0 .. nbytes) for output rows y0 .. y1 - 1
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ src, int64_t pitch, int rows, int ry0,
                                                         const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int y0,
                                                         int y1, int nbytes, uint8_t* __restrict__ out) {
    const int b = blockIdx.z;
    const int y = __builtin_amdgcn_readfirstlane(y0 + blockIdx.y * 4 + threadIdx.y);
    const int j = (blockIdx.x * 64 + threadIdx.x) * 16;
    if (y >= y1 || j >= nbytes) return;
    int ymin = bounds[2 * y] - ry0, n = bounds[2 * y + 1];
    ymin = min(max(ymin, 0), rows);                               // clipped to the rows that exist
    n = min(min(n, ksize), rows - ymin);
    const int* k = kk + (int64_t)y * ksize;
    const uint8_t* s = src + ((int64_t)b * rows + ymin) * pitch + j;
    int acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 1 << (PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) {
        const int w = k[t];
        const uint4 v = *reinterpret_cast<const uint4*>(s + (int64_t)t * pitch);
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] += (int)(d[i >> 2] >> (8 * (i & 3)) & 0xFFu) * w;
    }
    uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i) d[i >> 2] |= clip8(acc[i]) << (8 * (i & 3));
    uint8_t* o = out + ((int64_t)b * (y1 - y0) + (y - y0)) * nbytes + j;
    if (j + 16 <= nbytes && ((uintptr_t)o & 15) == 0) {
        *reinterpret_cast<uint4*>(o) = make_uint4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (j + i < nbytes) o[i] = (uint8_t)(d[i >> 2] >> (8 * (i & 3)));
    }
}

}  // namespace

extern "C" int e4s_pil_resample_h_u8(const uint8_t* img, int B, int H, int W, const int32_t* bounds, const int32_t* kk, int ksize,
                                     int out_size, int x0, int x1, int ry0, int rows, uint8_t* dst, int64_t dst_pitch,
                                     int64_t dst_bstride, int tx, int rh, int span, void* stream) {
    if (!img || !bounds || !kk || !dst || B <= 0 || B > 65535 || H <= 0 || W <= 0 || ksize <= 0 || out_size <= 0) return (int)hipErrorInvalidValue;
    if (x0 < 0 || x1 <= x0 || x1 > out_size || ry0 < 0 || rows <= 0 || ry0 + rows > H) return (int)hipErrorInvalidValue;
    if (dst_pitch < (int64_t)(x1 - x0) * 3 || dst_bstride < dst_pitch * rows) return (int)hipErrorInvalidValue;
    if (tx < PX || tx > 128 || (tx & (tx - 1)) || (rh != RH && rh != 1) || span <= 0 || span > W) return (int)hipErrorInvalidValue;
    const int64_t lds_pitch = (((int64_t)span * 3 + 15) / 16 + 1) * 16;      // the span plus the up to 15 bytes in front of it
    if (lds_pitch * rh > LDS_LIMIT || cdiv(rows, rh) > 65535) return (int)hipErrorInvalidValue;
    const dim3 grid(cdiv(x1 - x0, tx), cdiv(rows, rh), B);
    hipLaunchKernelGGL(resample_h_kernel, grid, dim3(tx / PX * rh), (size_t)(lds_pitch * rh), as_stream(stream), img, H, W, bounds, kk,
                       ksize, x0, x1, ry0, rows, dst, dst_pitch, dst_bstride, tx, rh, span, (int)lds_pitch, (int64_t)B * H * W * 3);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_pil_resample_v_u8(const uint8_t* src, int64_t pitch, int B, int rows, int ry0, const int32_t* bounds,
                                     const int32_t* kk, int ksize, int out_size, int y0, int y1, int nbytes, uint8_t* out, void* stream) {
    if (!src || !bounds || !kk || !out || B <= 0 || B > 65535 || rows <= 0 || ry0 < 0 || ksize <= 0 || out_size <= 0) return (int)hipErrorInvalidValue;
    if (y0 < 0 || y1 <= y0 || y1 > out_size || nbytes <= 0 || pitch < nbytes || (pitch & 15) || !aligned16(src)) return (int)hipErrorInvalidValue;
    if (cdiv(y1 - y0, 4) > 65535) return (int)hipErrorInvalidValue;
    const dim3 grid(cdiv(nbytes, 64 * 16), cdiv(y1 - y0, 4), B);
    hipLaunchKernelGGL(resample_v_kernel, grid, dim3(64, 4), 0, as_stream(stream), src, pitch, rows, ry0, bounds, kk, ksize, y0, y1,
                       nbytes, out);
    E4S_CHECK_LAUNCH();
    return 0;
}
