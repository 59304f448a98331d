// Face editing (e4s_amd/edit.py): what scripts/face_edit.py and demo/gradio_demo.py do around the network in torch / numpy, each
// as one streaming kernel.
//   e4s_texture_mix_f32       face_edit.py:81-87, gradio_demo.py:165-170   the per-region blend of two sets of texture vectors
//   e4s_labels_to_color_u8    gradio_utils.py:58-73     label map -> the demo's coloured mask (19 colours; 255 and unknown ids black)
//   e4s_color_to_labels_u8    gradio_utils.py:75-84     coloured mask -> label map (exact RGB match; unmatched 0)
//   e4s_mask_brush_u8         gradio_demo.py:126-130    labels[sum(brush rgb) != 0] = comp_idx
// All are a few hundred KB per call and launch-bound; the uint8 ones move whole dwords where the pointers allow it.
#include "common.h"

// The mix restates `(1 - alpha) * src + alpha * ref` of torch: two products and one sum, one rounding each.  hipcc's default
// -ffp-contract=fast-honor-pragmas would fuse them, and the header inlines __fmul_rn / __fadd_rn are plain operators parsed before
// this pragma (stitch.hip has the story): the arithmetic goes through the helpers below it.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

// out[b, r, :] = sel[b, r] ? a0[b, r] * src[b|0, r, :] + a1[b, r] * ref[b|0, r, :] : src[b|0, r, :].  VEC: a thread takes 4 floats
// (C % 4 == 0, 16-byte aligned pointers), else one.
template <int VEC>
__global__ __launch_bounds__(256) void texture_mix_kernel(const float* __restrict__ src, const float* __restrict__ ref,
                                                          const uint8_t* __restrict__ sel, const float* __restrict__ a0,
                                                          const float* __restrict__ a1, float* __restrict__ out, int R, int C,
                                                          int src_b1, int ref_b1, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int per_row = C / VEC;
    const int64_t row = i / per_row;                       // b * R + r
    const int c = (int)(i - row * per_row) * VEC;
    const int r = (int)(row % R);
    const int64_t so = (src_b1 ? (int64_t)r : row) * C + c, ro = (ref_b1 ? (int64_t)r : row) * C + c, oo = row * C + c;
    const bool on = sel[row] != 0;
    if (VEC == 4) {
        f32x4 v = *reinterpret_cast<const f32x4*>(src + so);
        if (on) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(ref + ro);
            const float p = a0[row], q = a1[row];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = add_rn(mul_rn(p, v[e]), mul_rn(q, w[e]));
        }
        *reinterpret_cast<f32x4*>(out + oo) = v;
    } else {
        float v = src[so];
        if (on) v = add_rn(mul_rn(a0[row], v), mul_rn(a1[row], ref[ro]));
        out[oo] = v;
    }
}

// ---- the demo's colour table (gradio_utils.py:35-56), as 0x00BBGGRR --------------------------------------------------------
constexpr int NCOL = 19;
#define E4S_RGB(r, g, b) ((uint32_t)(r) | (uint32_t)(g) << 8 | (uint32_t)(b) << 16)
__device__ __forceinline__ uint32_t comp_color(int id) {
    constexpr uint32_t T[NCOL] = {E4S_RGB(0, 0, 0),       E4S_RGB(204, 0, 0),     E4S_RGB(76, 153, 0),  E4S_RGB(204, 204, 0),
                                  E4S_RGB(51, 51, 255),   E4S_RGB(204, 0, 204),   E4S_RGB(0, 255, 255), E4S_RGB(255, 204, 204),
                                  E4S_RGB(102, 51, 0),    E4S_RGB(255, 0, 0),     E4S_RGB(102, 204, 0), E4S_RGB(255, 255, 0),
                                  E4S_RGB(0, 0, 153),     E4S_RGB(0, 0, 204),     E4S_RGB(255, 51, 153), E4S_RGB(0, 204, 204),
                                  E4S_RGB(0, 51, 0),      E4S_RGB(255, 153, 51),  E4S_RGB(0, 204, 0)};
    uint32_t c = 0;                                        // ids >= 19 (255 among them): black
#pragma unroll
    for (int k = 1; k < NCOL; ++k) c = id == k ? T[k] : c;
    return c;
}
__device__ __forceinline__ uint32_t color_comp(uint32_t rgb) {
    uint32_t id = 0;                                       // the table's colours are distinct: at most one match
#pragma unroll
    for (int k = 1; k < NCOL; ++k) id = rgb == comp_color(k) ? (uint32_t)k : id;
    return id;
}

struct u32x3 { uint32_t v[3]; };                           // 12 bytes, 4-byte aligned: four 24-bit pixels
__device__ __forceinline__ u32x3 pack12(const uint32_t (&p)[4]) {
    return u32x3{{p[0] | p[1] << 24, p[1] >> 8 | p[2] << 16, p[2] >> 16 | p[3] << 8}};
}
__device__ __forceinline__ void unpack12(const u32x3 w, uint32_t (&p)[4]) {
    p[0] = w.v[0] & 0xFFFFFFu;
    p[1] = (w.v[0] >> 24 | w.v[1] << 8) & 0xFFFFFFu;
    p[2] = (w.v[1] >> 16 | w.v[2] << 16) & 0xFFFFFFu;
    p[3] = w.v[2] >> 8;
}

// A thread takes four consecutive pixels: one dword of labels, three of colours (dw: both pointers are 4-byte aligned).
__global__ __launch_bounds__(256) void labels_to_color_kernel(const uint8_t* __restrict__ labels, uint8_t* __restrict__ rgb, int64_t n,
                                                              int dw) {
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= n) return;
    const int cnt = (int)min((int64_t)4, n - p0);
    uint32_t px[4] = {0u, 0u, 0u, 0u};
    if (dw && cnt == 4) {
        const uint32_t l = *reinterpret_cast<const uint32_t*>(labels + p0);
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = comp_color((int)(l >> (8 * q) & 0xFFu));
        *reinterpret_cast<u32x3*>(rgb + p0 * 3) = pack12(px);
    } else {
        for (int q = 0; q < cnt; ++q) {
            const uint32_t c = comp_color(labels[p0 + q]);
            uint8_t* o = rgb + (p0 + q) * 3;
            o[0] = (uint8_t)c;
            o[1] = (uint8_t)(c >> 8);
            o[2] = (uint8_t)(c >> 16);
        }
    }
}

__global__ __launch_bounds__(256) void color_to_labels_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ labels, int64_t n,
                                                              int dw) {
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= n) return;
    const int cnt = (int)min((int64_t)4, n - p0);
    if (dw && cnt == 4) {
        uint32_t px[4];
        unpack12(*reinterpret_cast<const u32x3*>(rgb + p0 * 3), px);
        uint32_t l = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) l |= color_comp(px[q]) << (8 * q);
        *reinterpret_cast<uint32_t*>(labels + p0) = l;
    } else {
        for (int q = 0; q < cnt; ++q) {
            const uint8_t* s = rgb + (p0 + q) * 3;
            labels[p0 + q] = (uint8_t)color_comp(s[0] | s[1] << 8 | (uint32_t)s[2] << 16);
        }
    }
}

// brush: `pix` bytes per pixel (3: RGB, 4: gradio's RGBA sketch), of which the first three are summed.  out may be labels itself:
// a thread reads only the pixels it writes.
__global__ __launch_bounds__(256) void mask_brush_kernel(const uint8_t* labels, const uint8_t* __restrict__ brush, uint8_t* out,
                                                         int64_t n, int pix, int comp, int dw) {
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= n) return;
    const int cnt = (int)min((int64_t)4, n - p0);
    if (dw && cnt == 4) {
        uint32_t l = *reinterpret_cast<const uint32_t*>(labels + p0);
        uint32_t px[4];
        if (pix == 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) px[q] = reinterpret_cast<const uint32_t*>(brush + p0 * 4)[q] & 0xFFFFFFu;
        } else {
            unpack12(*reinterpret_cast<const u32x3*>(brush + p0 * 3), px);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (px[q]) l = (l & ~(0xFFu << (8 * q))) | (uint32_t)comp << (8 * q);      // a sum of three bytes is 0 only if all are
        *reinterpret_cast<uint32_t*>(out + p0) = l;
    } else {
        for (int q = 0; q < cnt; ++q) {
            const uint8_t* s = brush + (p0 + q) * pix;
            const uint8_t l = labels[p0 + q];
            out[p0 + q] = (s[0] | s[1] | s[2]) ? (uint8_t)comp : l;
        }
    }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool quads_fit(int64_t n) { return (n + 3) / 4 + 255 < (1ll << 39); }          // grid.x < 2^31 blocks of 256 threads

}  // namespace

extern "C" int e4s_texture_mix_f32(const float* src, const float* ref, const uint8_t* sel, const float* a0, const float* a1, float* out,
                                   int B, int R, int C, int src_b1, int ref_b1, void* stream) {
    if (!src || !ref || !sel || !a0 || !a1 || !out || B <= 0 || R <= 0 || C <= 0) return (int)hipErrorInvalidValue;
    const bool vec = (C & 3) == 0 && aligned16(src) && aligned16(ref) && aligned16(out);
    const int64_t n = (int64_t)B * R * (vec ? C / 4 : C);
    if ((n + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    if (vec)
        hipLaunchKernelGGL(texture_mix_kernel<4>, grid1(n), dim3(256), 0, as_stream(stream), src, ref, sel, a0, a1, out, R, C,
                           src_b1 ? 1 : 0, ref_b1 ? 1 : 0, n);
    else
        hipLaunchKernelGGL(texture_mix_kernel<1>, grid1(n), dim3(256), 0, as_stream(stream), src, ref, sel, a0, a1, out, R, C,
                           src_b1 ? 1 : 0, ref_b1 ? 1 : 0, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_labels_to_color_u8(const uint8_t* labels, uint8_t* rgb, int64_t n, void* stream) {
    if (!labels || !rgb || n < 0 || !quads_fit(n)) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    hipLaunchKernelGGL(labels_to_color_kernel, grid1((n + 3) / 4), dim3(256), 0, as_stream(stream), labels, rgb, n,
                       aligned4(labels) && aligned4(rgb) ? 1 : 0);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_color_to_labels_u8(const uint8_t* rgb, uint8_t* labels, int64_t n, void* stream) {
    if (!labels || !rgb || n < 0 || !quads_fit(n)) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    hipLaunchKernelGGL(color_to_labels_kernel, grid1((n + 3) / 4), dim3(256), 0, as_stream(stream), rgb, labels, n,
                       aligned4(labels) && aligned4(rgb) ? 1 : 0);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_mask_brush_u8(const uint8_t* labels, const uint8_t* brush, uint8_t* out, int64_t n, int brush_pix, int comp_idx,
                                 void* stream) {
    if (!labels || !brush || !out || n < 0 || !quads_fit(n) || (brush_pix != 3 && brush_pix != 4) || comp_idx < 0 || comp_idx > 255)
        return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    hipLaunchKernelGGL(mask_brush_kernel, grid1((n + 3) / 4), dim3(256), 0, as_stream(stream), labels, brush, out, n, brush_pix, comp_idx,
                       aligned4(labels) && aligned4(brush) && aligned4(out) ? 1 : 0);
    E4S_CHECK_LAUNCH();
    return 0;
}
