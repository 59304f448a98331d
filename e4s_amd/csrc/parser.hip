// BiSeNet face parser glue (e4s_amd/face_parser.py): everything of src/pretrained/face_parsing/ that is not a convolution.
//   preprocess        BicubicDownSample(factor 2) + clamp(0,1) + ImageNet normalise   face_parsing_demo.py:15-73,152-162
//   maxpool3s2p1      nn.MaxPool2d(3, 2, padding 1) of ResNet-18                       resnet.py:62
//   add_relu          relu(shortcut + residual) of a BasicBlock (also a strided copy)   resnet.py:37-48
//   mean_hw / fc      global average pool, then 1x1 conv + folded BN + act             model.py:72-79,107-108,205-212
//   gate_add_up2      nearest x2 of (feat * gate + add)                                 model.py:110-118
//   head              bilinear (align_corners) upsample + argmax (+ 19 -> 12 map, one-hot) of the first head, or NCHW logits
// The convolutions themselves run on the library's conv kernels.  Element-wise arithmetic keeps the reference's operation
// order with one rounding per operation (no FMA contraction).  Every entry point enqueues on `stream` and never synchronises.
#include "common.h"

#pragma clang fp contract(off)

namespace {

struct Taps8 { float k[8]; };

__device__ __forceinline__ int reflect_idx(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

// one thread per output pixel, 3 channels: vertical 8-tap pass at the 8 input columns the horizontal pass needs, then the
// horizontal pass (the order of BicubicDownSample.forward).  Reflect padding 3/3 on both axes, stride 2.
template <bool U8>
__global__ void preprocess_kernel(const void* __restrict__ src, float* __restrict__ dst, int H, int W, int Ho, int Wo, int64_t n,
                                  Taps8 t) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ox = (int)(i % Wo);
    const int oy = (int)((i / Wo) % Ho);
    const int64_t b = i / ((int64_t)Wo * Ho);
    int rows[8], cols[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        rows[j] = reflect_idx(2 * oy - 3 + j, H);
        cols[j] = reflect_idx(2 * ox - 3 + j, W);
    }
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 8; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float px;
                if constexpr (U8) px = (float)static_cast<const uint8_t*>(src)[((b * H + rows[r]) * W + cols[j]) * 3 + c] / 255.f;
                else px = static_cast<const float*>(src)[((b * 3 + c) * H + rows[r]) * W + cols[j]];
                v[c] = v[c] + t.k[r] * px;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + t.k[j] * v[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f;          // model.py:13-14
        const float stdv = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
        dst[i * 3 + c] = (fminf(fmaxf(acc[c], 0.f), 1.f) - mean) / stdv;
    }
}

__global__ void maxpool3s2p1_kernel(const float* __restrict__ x, float* __restrict__ y, int Hi, int Wi, int Ho, int Wo, int C,
                                    int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int c4 = C / 4;
    const int cq = (int)(i % c4);
    const int64_t pix = i / c4;
    const int ox = (int)(pix % Wo);
    const int oy = (int)((pix / Wo) % Ho);
    const int64_t b = pix / ((int64_t)Wo * Ho);
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int dy = -1; dy <= 1; ++dy) {
        const int iy = 2 * oy + dy;
        if (iy < 0 || iy >= Hi) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int ix = 2 * ox + dx;
            if (ix < 0 || ix >= Wi) continue;
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((b * Hi + iy) * Wi + ix) * C + 4 * cq);
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = (v[k] > m[k] || v[k] != v[k]) ? v[k] : m[k];     // NaN propagates (ATen)
        }
    }
    *reinterpret_cast<f32x4*>(y + pix * C + 4 * cq) = m;
}

__global__ void add_relu_kernel(const float* __restrict__ a, const float* __restrict__ r, float* __restrict__ y, int C,
                                int y_cstride, int y_coff, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int c4 = C / 4;
    const int cq = (int)(i % c4);
    const int64_t pix = i / c4;
    f32x4 v = *reinterpret_cast<const f32x4*>(a + 4 * i);
    if (r) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(r + 4 * i);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] + u[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
    *reinterpret_cast<f32x4*>(y + pix * y_cstride + y_coff + 4 * cq) = v;
}

// block (64 channels x 16 waves) per (channel chunk, sample); fixed summation order (deterministic)
__global__ __launch_bounds__(1024) void mean_hw_kernel(const float* __restrict__ x, float* __restrict__ out, int HW, int C) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int b = blockIdx.y;
    float s = 0.f;
    if (c < C) {
        const float* xb = x + (int64_t)b * HW * C + c;
        for (int p = wv; p < HW; p += 16) s += xb[(int64_t)p * C];
    }
    part[wv][lane] = s;
    __syncthreads();
    if (wv == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += part[k][lane];
        out[(int64_t)b * C + c] = t / (float)HW;
    }
}

// one wave per output: out[b,o] = act(sum_i w[o,i] v[b,i] + bias[o]) + offset   (w == NULL: act(v[b,o] + bias[o]) + offset)
__global__ void fc_kernel(const float* __restrict__ v, const float* __restrict__ w, const float* __restrict__ bias,
                          float* __restrict__ out, int Ci, int Co, int act, float offset) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    if (o >= Co) return;
    const float* vb = v + (int64_t)b * Ci;
    float s;
    if (w) {
        s = 0.f;
        const float* wr = w + (int64_t)o * Ci;
        for (int i = lane; i < Ci; i += 64) s += wr[i] * vb[i];
        s = wave_sum(s);
    } else {
        s = vb[o];
    }
    if (lane != 0) return;
    if (bias) s = s + bias[o];
    if (act == 1) s = fmaxf(s, 0.f);
    else if (act == 2) s = 1.f / (1.f + expf(-s));
    out[(int64_t)b * Co + o] = s + offset;
}

// y[b, 2i+di, 2j+dj, c] = x[b,i,j,c] * gate[b,c] + add     (add: [B,C] broadcast, or a map [B,h,w,C])
__global__ void gate_add_up2_kernel(const float* __restrict__ x, const float* __restrict__ gate, const float* __restrict__ add,
                                    int add_map, float* __restrict__ y, int h, int w, int C, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int c4 = C / 4;
    const int cq = (int)(i % c4);
    const int64_t pix = i / c4;
    const int j = (int)(pix % w);
    const int r = (int)((pix / w) % h);
    const int64_t b = pix / ((int64_t)w * h);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + 4 * i);
    const f32x4 g = *reinterpret_cast<const f32x4*>(gate + b * C + 4 * cq);
    const f32x4 a = *reinterpret_cast<const f32x4*>(add_map ? add + 4 * i : add + b * C + 4 * cq);
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = xv[k] * g[k] + a[k];
    const int W2 = 2 * w;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
            *reinterpret_cast<f32x4*>(y + ((b * 2 * h + 2 * r + dy) * W2 + 2 * j + dx) * C + 4 * cq) = v;
}

__constant__ uint8_t kSeg12[19] = {0, 6, 2, 2, 3, 3, 10, 7, 7, 11, 5, 9, 1, 1, 8, 0, 0, 4, 0};   // dataset.py:60-108

constexpr int kMaxCls = 32;

// one thread per output pixel: F.interpolate(bilinear, align_corners=True) of every class at this pixel (ATen's CPU formula),
// then the first maximum (torch.argmax), optionally mapped to the 12 classes and expanded to a one-hot; or the NCHW logits.
__global__ void head_kernel(const float* __restrict__ lg, int h, int w, int ncls, int cstride, int H, int W, float sh, float sw,
                            int seg12, uint8_t* __restrict__ labels, float* __restrict__ onehot, float* __restrict__ nchw,
                            int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ox = (int)(i % W);
    const int oy = (int)((i / W) % H);
    const int64_t b = i / ((int64_t)W * H);
    const float ry = sh * (float)oy, rx = sw * (float)ox;
    const int y0 = (int)ry, x0 = (int)rx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float l1y = ry - (float)y0, l0y = 1.f - l1y;
    const float l1x = rx - (float)x0, l0x = 1.f - l1x;
    const float* p00 = lg + ((b * h + y0) * w + x0) * cstride;
    const float* p01 = lg + ((b * h + y0) * w + x1) * cstride;
    const float* p10 = lg + ((b * h + y1) * w + x0) * cstride;
    const float* p11 = lg + ((b * h + y1) * w + x1) * cstride;
    const int64_t hw = (int64_t)H * W, pix = i - b * hw;
    int best = 0;
    float bv = 0.f;
    for (int c = 0; c < ncls; ++c) {
        const float v = l0y * (l0x * p00[c] + l1x * p01[c]) + l1y * (l0x * p10[c] + l1x * p11[c]);
        if (nchw) nchw[(b * ncls + c) * hw + pix] = v;
        if (c == 0 || v > bv) { bv = v; best = c; }
    }
    if (!labels && !onehot) return;
    const int lab = seg12 ? kSeg12[best] : best;
    if (labels) labels[i] = (uint8_t)lab;
    if (onehot) {
        const int nout = seg12 ? 12 : ncls;
        for (int c = 0; c < nout; ++c) onehot[(b * nout + c) * hw + pix] = c == lab ? 1.f : 0.f;
    }
}

}  // namespace

extern "C" int e4s_parser_preprocess_f32(const void* src, int is_u8, float* dst, int B, int H, int W, const float* taps8,
                                         void* stream) {
    if (B < 1 || H < 4 || W < 4 || (H & 1) || (W & 1) || !taps8) return (int)hipErrorInvalidValue;
    Taps8 t;
    for (int j = 0; j < 8; ++j) t.k[j] = taps8[j];           // host array (kernel argument): capture-safe
    const int Ho = H / 2, Wo = W / 2;
    const int64_t n = (int64_t)B * Ho * Wo;
    if (is_u8) hipLaunchKernelGGL(preprocess_kernel<true>, grid1(n), dim3(256), 0, as_stream(stream), src, dst, H, W, Ho, Wo, n, t);
    else hipLaunchKernelGGL(preprocess_kernel<false>, grid1(n), dim3(256), 0, as_stream(stream), src, dst, H, W, Ho, Wo, n, t);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_maxpool3s2p1_f32(const float* x, float* y, int B, int Hi, int Wi, int C, void* stream) {
    if (C % 4 || Hi < 1 || Wi < 1) return (int)hipErrorInvalidValue;
    const int Ho = (Hi - 1) / 2 + 1, Wo = (Wi - 1) / 2 + 1;
    const int64_t n4 = (int64_t)B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(maxpool3s2p1_kernel, grid1(n4), dim3(256), 0, as_stream(stream), x, y, Hi, Wi, Ho, Wo, C, n4);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_add_relu_f32(const float* a, const float* r, float* y, int64_t npix, int C, int y_cstride, int y_coff,
                                void* stream) {
    if (y_cstride == 0) y_cstride = C;
    if (C % 4 || y_cstride % 4 || y_coff % 4 || y_coff < 0 || y_coff + C > y_cstride) return (int)hipErrorInvalidValue;
    const int64_t n4 = npix * (C / 4);
    hipLaunchKernelGGL(add_relu_kernel, grid1(n4), dim3(256), 0, as_stream(stream), a, r, y, C, y_cstride, y_coff, n4);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_mean_hw_f32(const float* x, float* out, int B, int HW, int C, void* stream) {
    if (B < 1 || HW < 1 || C < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mean_hw_kernel, dim3(cdiv(C, 64), B), dim3(1024), 0, as_stream(stream), x, out, HW, C);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_parser_fc_f32(const float* v, const float* w, const float* bias, float* out, int B, int Ci, int Co, int act,
                                 float offset, void* stream) {
    if (B < 1 || Ci < 1 || Co < 1 || act < 0 || act > 2 || (!w && Ci != Co)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fc_kernel, dim3(cdiv(Co, 4), B), dim3(256), 0, as_stream(stream), v, w, bias, out, Ci, Co, act, offset);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_gate_add_up2_f32(const float* x, const float* gate, const float* add, int add_map, float* y, int B, int h,
                                    int w, int C, void* stream) {
    if (C % 4 || B < 1 || h < 1 || w < 1) return (int)hipErrorInvalidValue;
    const int64_t n4 = (int64_t)B * h * w * (C / 4);
    hipLaunchKernelGGL(gate_add_up2_kernel, grid1(n4), dim3(256), 0, as_stream(stream), x, gate, add, add_map, y, h, w, C, n4);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_parser_head_f32(const float* logits, int B, int h, int w, int ncls, int cstride, int H, int W, int seg12,
                                   uint8_t* labels, float* onehot, float* nchw, void* stream) {
    if (B < 1 || h < 1 || w < 1 || H < 1 || W < 1 || ncls < 1 || ncls > kMaxCls || cstride < ncls) return (int)hipErrorInvalidValue;
    if (seg12 && ncls != 19) return (int)hipErrorInvalidValue;
    const float sh = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    const float sw = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const int64_t n = (int64_t)B * H * W;
    hipLaunchKernelGGL(head_kernel, grid1(n), dim3(256), 0, as_stream(stream), logits, h, w, ncls, cstride, H, W, sh, sw, seg12,
                       labels, onehot, nchw, n);
    E4S_CHECK_LAUNCH();
    return 0;
}
