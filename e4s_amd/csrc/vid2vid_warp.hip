// face-vid2vid's dense motion and 3-D feature warp (e4s_amd/reenact_warp.py; src/pretrained/face_vid2vid/modules/dense_motion.py,
// generator.py:211-246): the streaming kernels around the 3-D convs of vid2vid.hip.  Volumes are channels-last fp32 [B,D,H,W,C].
//
// Coordinates.  make_coordinate_grid gives voxel i of n the coordinate 2 (i / (n - 1)) - 1 (an align_corners=True grid); F.grid_sample
// is called with its default align_corners=False, so coordinate g of an axis of n voxels reads index ((g + 1) n - 1) / 2: the
// reference's "identity" grid does not sample voxel centres, and that is kept.  Samples are trilinear with zero padding: a corner
// outside the volume contributes zero.  The corners are added in the order (z0, z1) x (y0, y1) x (x0, x1), x fastest.
// Sparse motions (create_sparse_motions): grid 0 is the coordinate grid; grid k + 1 is J_k (grid - kp_driving_k) + kp_source_k, J_k =
// J_source_k inverse(J_driving_k) (e4s_kp_jacobian_f32, by cofactors) or the identity without jacobians.  They are recomputed from
// the keypoints wherever they are needed and never stored.
// Sums: the soft-max and the deformation run over k in rising order; the occlusion head's order is fixed by (kernel, D, C) alone
// (thread t adds items t, t + 256, ... in rising order, then wave_sum and the four waves in rising order).  Nothing depends on the
// batch or on the position.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAXG = 32;                                        // keypoints + 1 a thread keeps in registers

// grid_sample's source index of coordinate g on an axis of n voxels (align_corners=False), clamped to [-2, n + 1]: every index
// below -1 or above n samples nothing but padding, so the clamp changes no result and keeps the integer conversion in range
__device__ __forceinline__ float unnormalize(float g, int n) {
    const float i = ((g + 1.f) * (float)n - 1.f) * 0.5f;
    return fminf(fmaxf(i, -2.f), (float)n + 1.f);
}

struct Kp {
    const float* src;                                           // [K][3] of this sample
    const float* drv;                                           // [K][3]
    const float* jac;                                           // [K][9] or nullptr
};

// sparse motion g (0: the grid itself) at grid point c
__device__ __forceinline__ void sparse_motion(const Kp& kp, int g, const float (&c)[3], float (&m)[3]) {
    if (g == 0) {
        m[0] = c[0], m[1] = c[1], m[2] = c[2];
        return;
    }
    const int k = g - 1;
    float d[3] = {c[0] - kp.drv[k * 3], c[1] - kp.drv[k * 3 + 1], c[2] - kp.drv[k * 3 + 2]};
    if (kp.jac) {
        const float* J = kp.jac + k * 9;
        const float e0 = (J[0] * d[0] + J[1] * d[1]) + J[2] * d[2];
        const float e1 = (J[3] * d[0] + J[4] * d[1]) + J[5] * d[2];
        const float e2 = (J[6] * d[0] + J[7] * d[1]) + J[8] * d[2];
        d[0] = e0, d[1] = e1, d[2] = e2;
    }
    m[0] = d[0] + kp.src[k * 3], m[1] = d[1] + kp.src[k * 3 + 1], m[2] = d[2] + kp.src[k * 3 + 2];
}

// trilinear sample of four channels at v (+ element strides sd, sy, sx) under the coordinates m (x, y, z)
__device__ __forceinline__ f32x4 sample4(const float* v, int64_t sd, int64_t sy, int64_t sx, int D, int H, int W, const float (&m)[3]) {
    const float fx = unnormalize(m[0], W), fy = unnormalize(m[1], H), fz = unnormalize(m[2], D);
    const float x0f = floorf(fx), y0f = floorf(fy), z0f = floorf(fz);
    const int x0 = (int)x0f, y0 = (int)y0f, z0 = (int)z0f;
    const float tx = fx - x0f, ty = fy - y0f, tz = fz - z0f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int dz = c >> 2, dy = (c >> 1) & 1, dx = c & 1;
        const int z = z0 + dz, y = y0 + dy, x = x0 + dx;
        if ((unsigned)z >= (unsigned)D || (unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) continue;
        const float wgt = ((dz ? tz : 1.f - tz) * (dy ? ty : 1.f - ty)) * (dx ? tx : 1.f - tx);
        acc += *reinterpret_cast<const f32x4*>(v + z * sd + y * sy + x * sx) * wgt;
    }
    return acc;
}

__device__ __forceinline__ void voxel_coord(int64_t v, int D, int H, int W, float (&c)[3]) {
    const int x = (int)(v % W);
    const int64_t t = v / W;
    c[0] = grid_coord(x, W), c[1] = grid_coord((int)(t % H), H), c[2] = grid_coord((int)(t / H), D);
}

// ---- y = relu(x * scale[c] + shift[c]): ResBlock3d's norm1 + ReLU in front of its zero-padded conv ----
__global__ __launch_bounds__(256) void bnrelu_kernel(const float* __restrict__ x, int64_t xb, int64_t xd, int64_t xy, int64_t xx,
                                                     const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ y,
                                                     int D, int H, int W, int C4, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C4);
    int64_t t = i / C4;
    const int ox = (int)(t % W);
    t /= W;
    const int oy = (int)(t % H);
    t /= H;
    const int od = (int)(t % D);
    const int64_t b = t / D;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + b * xb + od * xd + oy * xy + ox * xx + c * 4);
    const f32x4 s = reinterpret_cast<const f32x4*>(scale)[c], h = reinterpret_cast<const f32x4*>(shift)[c];
    f32x4 r = v * s + h;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = r[e] > 0.f ? r[e] : 0.f;
    reinterpret_cast<f32x4*>(y)[i] = r;
}

// ---- out[n][k] = Js[n or 0][k] inverse(Jd[n][k]) ----
__global__ __launch_bounds__(64) void kp_jacobian_kernel(const float* __restrict__ js, int js_batch, const float* __restrict__ jd,
                                                         float* __restrict__ out, int K, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* a = jd + (int64_t)i * 9;
    const float* s = js + (int64_t)(js_batch == 1 ? i % K : i) * 9;
    const float c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const float det = (a[0] * c00 + a[1] * c01) + a[2] * c02;
    const float inv[9] = {c00 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
                          c01 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
                          c02 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(int64_t)i * 9 + r * 3 + c] = (s[r * 3] * inv[c] + s[r * 3 + 1] * inv[3 + c]) + s[r * 3 + 2] * inv[6 + c];
}

// ---- the hourglass input: per (sample, voxel, grid g) channels 5 g .. 5 g + 4 = [heat-map difference, the four compressed features
// sampled under sparse motion g] ----
__global__ __launch_bounds__(256) void sparse_warp_kernel(const float* __restrict__ feat, int feat_batch, const float* __restrict__ kps,
                                                          int kp_batch, const float* __restrict__ kpd, const float* __restrict__ jac,
                                                          float* __restrict__ y, int y_cstride, int K, int D, int H, int W, float variance,
                                                          int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int G = K + 1;
    const int g = (int)(i % G);
    const int64_t V = (int64_t)D * H * W;
    const int64_t nv = i / G, b = nv / V, v = nv % V;
    const Kp kp = {kps + (kp_batch == 1 ? 0 : b) * K * 3, kpd + b * K * 3, jac ? jac + b * K * 9 : nullptr};
    float c[3], m[3];
    voxel_coord(v, D, H, W, c);
    sparse_motion(kp, g, c, m);
    const float* vol = feat + (feat_batch == 1 ? 0 : b) * V * 4;
    const f32x4 s = sample4(vol, (int64_t)H * W * 4, (int64_t)W * 4, 4, D, H, W, m);
    float heat = 0.f;
    if (g > 0) {
        const int k = g - 1;
        const float dx = c[0] - kp.drv[k * 3], dy = c[1] - kp.drv[k * 3 + 1], dz = c[2] - kp.drv[k * 3 + 2];
        const float sx = c[0] - kp.src[k * 3], sy = c[1] - kp.src[k * 3 + 1], sz = c[2] - kp.src[k * 3 + 2];
        heat = expf(-0.5f * ((dx * dx + dy * dy) + dz * dz) / variance) - expf(-0.5f * ((sx * sx + sy * sy) + sz * sz) / variance);
    }
    float* dst = y + nv * y_cstride + g * 5;
    dst[0] = heat, dst[1] = s[0], dst[2] = s[1], dst[3] = s[2], dst[4] = s[3];
}

// ---- mask = softmax over the K + 1 logits of a voxel; deformation = sum_g mask_g * sparse motion g ----
__global__ __launch_bounds__(256) void motion_combine_kernel(const float* __restrict__ logits, int l_cstride, const float* __restrict__ kps,
                                                             int kp_batch, const float* __restrict__ kpd, const float* __restrict__ jac,
                                                             float* __restrict__ mask, float* __restrict__ deform, int K, int D, int H, int W,
                                                             int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int G = K + 1;
    const int64_t V = (int64_t)D * H * W;
    const int64_t b = i / V, v = i % V;
    const Kp kp = {kps + (kp_batch == 1 ? 0 : b) * K * 3, kpd + b * K * 3, jac ? jac + b * K * 9 : nullptr};
    const float* lg = logits + i * l_cstride;
    float e[MAXG];
    float mx = lg[0];
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
        e[g] = g < G ? lg[g] : -INFINITY;
        mx = fmaxf(mx, e[g]);
    }
    float sum = 0.f;
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
        e[g] = g < G ? expf(e[g] - mx) : 0.f;
        sum += e[g];
    }
    float c[3], dsum[3] = {0.f, 0.f, 0.f};
    voxel_coord(v, D, H, W, c);
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
        if (g >= G) break;
        const float wgt = e[g] / sum;
        float m[3];
        sparse_motion(kp, g, c, m);
        mask[i * G + g] = wgt;
        dsum[0] += wgt * m[0], dsum[1] += wgt * m[1], dsum[2] += wgt * m[2];
    }
    deform[i * 3] = dsum[0], deform[i * 3 + 1] = dsum[1], deform[i * 3 + 2] = dsum[2];
}

// ---- the final warp: y[n][y][x][d C + c] = trilinear sample of the (batch-1, broadcast) volume under deformation[n][d][y][x] ----
__global__ __launch_bounds__(256) void warp3d_kernel(const float* __restrict__ vol, int64_t sd, int64_t sy, int64_t sx,
                                                     const float* __restrict__ deform, float* __restrict__ y, int D, int H, int W, int C4,
                                                     int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C4);
    int64_t t = i / C4;                                         // (sample, d, y, x)
    const float* df = deform + t * 3;
    const float m[3] = {df[0], df[1], df[2]};
    const f32x4 s = sample4(vol + c * 4, sd, sy, sx, D, H, W, m);
    const int ox = (int)(t % W);
    t /= W;
    const int oy = (int)(t % H);
    t /= H;
    const int od = (int)(t % D);
    const int64_t b = t / D;
    reinterpret_cast<f32x4*>(y)[(((b * H + oy) * W + ox) * D + od) * C4 + c] = s;
}

// ---- occlusion head: sigmoid of a ks x ks zero-padded conv of the (D C)-channel map to ONE channel; a block per output pixel ----
__global__ __launch_bounds__(256) void occlusion_kernel(const float* __restrict__ x, int x_cstride, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ out, int D, int H, int W, int C4,
                                                        int ks) {
    __shared__ float s_part[4];
    const int tid = threadIdx.x;
    const int64_t pix = blockIdx.x;
    const int ox = (int)(pix % W), oy = (int)((pix / W) % H);
    const int64_t b = pix / ((int64_t)W * H);
    const int per_tap = D * C4, items = ks * ks * per_tap, pad = ks / 2;
    float acc = 0.f;
    for (int it = tid; it < items; it += 256) {
        const int tap = it / per_tap, r = it - tap * per_tap;
        const int d = r / C4, c = r - d * C4;
        const int iy = oy + tap / ks - pad, ix = ox + tap % ks - pad;
        if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (((b * D + d) * H + iy) * W + ix) * x_cstride + c * 4);
        const f32x4 wv = reinterpret_cast<const f32x4*>(w)[it];
        acc += ((xv[0] * wv[0] + xv[1] * wv[1]) + xv[2] * wv[2]) + xv[3] * wv[3];
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        const float v = (((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]) + (bias ? bias[0] : 0.f);
        out[pix] = 1.f / (1.f + expf(-v));
    }
}

// ---- y[r][c] *= m[r] ----
__global__ __launch_bounds__(256) void scale_rows_kernel(float* __restrict__ y, const float* __restrict__ m, int C4, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    reinterpret_cast<f32x4*>(y)[i] = reinterpret_cast<f32x4*>(y)[i] * m[i / C4];
}

inline bool grid_ok(int64_t n) { return n >= 1 && (n + 255) / 256 < (1ll << 31); }
inline bool volume_ok(int B, int D, int H, int W) { return B >= 1 && D >= 1 && H >= 1 && W >= 1 && (int64_t)B * D * H * W < (1ll << 31); }

}  // namespace

extern "C" int e4s_bnrelu3d_f32(const float* x, int64_t x_bstride, int64_t x_dstride, int64_t x_ystride, int64_t x_xstride,
                                const float* scale, const float* shift, float* y, int B, int D, int H, int W, int C, void* stream) {
    if (!x || !scale || !shift || !y || !volume_ok(B, D, H, W) || C < 4 || C % 4) return (int)hipErrorInvalidValue;
    if (x_bstride < 0 || x_dstride < 0 || x_ystride < 0 || x_xstride < C) return (int)hipErrorInvalidValue;
    if (x_bstride % 4 || x_dstride % 4 || x_ystride % 4 || x_xstride % 4) return (int)hipErrorInvalidValue;
    if (!aligned16(x) || !aligned16(scale) || !aligned16(shift) || !aligned16(y)) return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)B * D * H * W * (C / 4);
    if (!grid_ok(n)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(bnrelu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, x_bstride, x_dstride, x_ystride,
                       x_xstride, scale, shift, y, D, H, W, C / 4, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_kp_jacobian_f32(const float* j_source, int source_batch, const float* j_driving, float* out, int N, int K, void* stream) {
    if (!j_source || !j_driving || !out || N < 1 || K < 1 || (source_batch != 1 && source_batch != N)) return (int)hipErrorInvalidValue;
    if ((int64_t)N * K >= (1ll << 30)) return (int)hipErrorInvalidValue;
    const int n = N * K;
    hipLaunchKernelGGL(kp_jacobian_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, as_stream(stream), j_source, source_batch, j_driving,
                       out, K, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_sparse_warp_f32(const float* feat, int feat_batch, const float* kp_source, int kp_batch, const float* kp_driving,
                                   const float* jac, float* y, int y_cstride, int N, int K, int D, int H, int W, int C, float variance,
                                   void* stream) {
    if (!feat || !kp_source || !kp_driving || !y || !volume_ok(N, D, H, W) || K < 1 || K + 1 > MAXG) return (int)hipErrorInvalidValue;
    if (C != 4 || y_cstride < 5 * (K + 1) || !(variance > 0.f) || !aligned16(feat)) return (int)hipErrorInvalidValue;
    if ((feat_batch != 1 && feat_batch != N) || (kp_batch != 1 && kp_batch != N)) return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)N * D * H * W * (K + 1);
    if (!grid_ok(n)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sparse_warp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), feat, feat_batch, kp_source,
                       kp_batch, kp_driving, jac, y, y_cstride, K, D, H, W, variance, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_motion_combine_f32(const float* logits, int l_cstride, const float* kp_source, int kp_batch, const float* kp_driving,
                                      const float* jac, float* mask, float* deformation, int N, int K, int D, int H, int W, void* stream) {
    if (!logits || !kp_source || !kp_driving || !mask || !deformation || !volume_ok(N, D, H, W)) return (int)hipErrorInvalidValue;
    if (K < 1 || K + 1 > MAXG || l_cstride < K + 1 || (kp_batch != 1 && kp_batch != N)) return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)N * D * H * W;
    hipLaunchKernelGGL(motion_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), logits, l_cstride, kp_source,
                       kp_batch, kp_driving, jac, mask, deformation, K, D, H, W, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_warp3d_f32(const float* vol, int64_t v_dstride, int64_t v_ystride, int64_t v_xstride, const float* deformation, float* y,
                              int N, int D, int H, int W, int C, void* stream) {
    if (!vol || !deformation || !y || !volume_ok(N, D, H, W) || C < 4 || C % 4 || !aligned16(vol) || !aligned16(y)) return (int)hipErrorInvalidValue;
    if (v_dstride < 0 || v_ystride < 0 || v_xstride < C || v_dstride % 4 || v_ystride % 4 || v_xstride % 4) return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)N * D * H * W * (C / 4);
    if (!grid_ok(n)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(warp3d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), vol, v_dstride, v_ystride, v_xstride,
                       deformation, y, D, H, W, C / 4, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_occlusion_f32(const float* x, int x_cstride, const float* w, const float* bias, float* out, int N, int D, int H, int W,
                                 int C, int ksize, void* stream) {
    if (!x || !w || !out || !volume_ok(N, D, H, W) || C < 4 || C % 4 || x_cstride < C || x_cstride % 4) return (int)hipErrorInvalidValue;
    if (ksize < 1 || !(ksize & 1) || ksize > 15 || !aligned16(x) || !aligned16(w)) return (int)hipErrorInvalidValue;
    if ((int64_t)ksize * ksize * D * (C / 4) >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(occlusion_kernel, dim3((unsigned)((int64_t)N * H * W)), dim3(256), 0, as_stream(stream), x, x_cstride, w, bias, out, D, H,
                       W, C / 4, ksize);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_scale_rows_f32(float* y, const float* m, int64_t rows, int C, void* stream) {
    if (!y || !m || rows < 1 || C < 4 || C % 4 || !aligned16(y)) return (int)hipErrorInvalidValue;
    const int64_t n = rows * (C / 4);
    if (!grid_ok(n)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), y, m, C / 4, n);
    E4S_CHECK_LAUNCH();
    return 0;
}
