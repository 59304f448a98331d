// Latent optimisation (scripts/optimization.py:125-161, 209-232): the two optimisers of `setup_W_optimizer` that had no fused form --
// torch.optim.SGD (with and without momentum) and torch.optim.Adamax -- as multi-tensor capturable steps in the calling convention of
// adam_multi_kernel (optim.hip): pointers BY VALUE in the kernel arguments, 48 tensors per launch, the learning rate in a device double,
// Adamax's step counts in device int64s (already advanced); and the script's `loss_dict` as one small launch that files up to 16 device
// scalars under the step's row of a device log.  Streaming kernels: 16 bytes per lane where every pointer of a tensor is 16-byte aligned
// and the block's 4096 elements are all there, one element per lane otherwise (unaligned views, tensor tails).
#include "common.h"

// one rounding per operation, as the chains of ATen launches these kernels stand for (no FMA contraction in this file)
#pragma clang fp contract(off)

namespace {

constexpr int MT = 48;          // tensors per launch (optim.hip)
constexpr int MT_ELEMS = 4096;  // elements per block

struct SgdChunk {
    float* p[MT];
    const float* g[MT];
    float* buf[MT];             // all NULL when momentum == 0
    int64_t n[MT];
    int blk0[MT + 1];
};
struct AdamaxChunk {
    float* p[MT];
    const float* g[MT];
    float* m[MT];
    float* u[MT];
    const int64_t* step[MT];
    int64_t n[MT];
    int blk0[MT + 1];
};
struct LogSrc {
    const float* src[16];
};

__device__ __forceinline__ int mt_find(const int* blk0, int cnt, int b) {
    int lo = 0, hi = cnt;                                       // blk0[lo] <= b < blk0[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk0[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// torch.optim.SGD (nesterov=False, maximize=False), _single_tensor_sgd:
//   g += wd * p;  buf = buf * momentum + omd * g;  p += neg_lr * buf            (momentum == 0: p += neg_lr * g, no buffer)
// The buffer starts as zeros: momentum * 0 + 1 * g is g exactly, torch's first-step clone (with dampening != 0 torch's first buffer is g
// and this one (1 - dampening) g: the one documented difference).
struct SgdCoef { float neg_lr, momentum, omd, wd; };

template <bool MOM>
__device__ __forceinline__ void sgd_elem(const SgdCoef& c, float& pv, float g, float& b) {
    if (c.wd != 0.f) g = g + c.wd * pv;
    if (MOM) {
        b = b * c.momentum + c.omd * g;
        g = b;
    }
    pv = pv + c.neg_lr * g;
}

template <bool MOM>
__global__ __launch_bounds__(256) void sgd_multi_kernel(const SgdChunk c, int cnt, double lr, const double* __restrict__ lr_dev, float momentum,
                                                        float omd, float wd) {
    const int t = mt_find(c.blk0, cnt, blockIdx.x);
    const int64_t base = (int64_t)(blockIdx.x - c.blk0[t]) * MT_ELEMS, n = c.n[t];
    float* __restrict__ p = c.p[t];
    const float* __restrict__ g = c.g[t];
    float* __restrict__ buf = MOM ? c.buf[t] : nullptr;
    if (lr_dev) lr = *lr_dev;
    const SgdCoef k = {(float)(-lr), momentum, omd, wd};
    const bool al = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)buf)) & 15) == 0;
    if (al && base + MT_ELEMS <= n) {
#pragma unroll
        for (int j = 0; j < MT_ELEMS / 1024; ++j) {
            const int64_t i = base + j * 1024 + threadIdx.x * 4;
            f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (MOM) bv = *reinterpret_cast<const f32x4*>(buf + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pv[e], be = bv[e];
                sgd_elem<MOM>(k, pe, gv[e], be);
                pv[e] = pe, bv[e] = be;
            }
            if (MOM) *reinterpret_cast<f32x4*>(buf + i) = bv;
            *reinterpret_cast<f32x4*>(p + i) = pv;
        }
        return;
    }
    for (int64_t i = base + threadIdx.x; i < min(base + (int64_t)MT_ELEMS, n); i += 256) {
        float pv = p[i], b = MOM ? buf[i] : 0.f;
        sgd_elem<MOM>(k, pv, g[i], b);
        if (MOM) buf[i] = b;
        p[i] = pv;
    }
}

// torch.optim.Adamax, _single_tensor_adamax on its non-capturable path:
//   g += wd * p;  m.lerp_(g, 1 - b1);  u = max(u * b2, |g| + eps);  p.addcdiv_(m, u, value = -(lr / (1 - b1^t)))
// b1^t in double from the DEVICE step count, once per thread.  u >= eps > 0 whatever g is: no division by zero.
struct AdamaxCoef { float neg_clr, w, omw, b2, eps, wd; };

__device__ __forceinline__ AdamaxCoef adamax_coef(double lr, const double* lr_dev, double beta1, double beta2, float eps, float wd,
                                                  const int64_t* step) {
    const double t = (double)*step;
    if (lr_dev) lr = *lr_dev;
    AdamaxCoef c;
    c.neg_clr = (float)(-(lr / (1.0 - pow(beta1, t))));
    c.w = (float)(1.0 - beta1), c.omw = 1.f - c.w;
    c.b2 = (float)beta2, c.eps = eps, c.wd = wd;
    return c;
}

__device__ __forceinline__ void adamax_elem(const AdamaxCoef& c, float& pv, float g, float& m, float& u) {
    if (c.wd != 0.f) g = g + c.wd * pv;
    const float d = g - m;
    m = c.w < 0.5f ? m + c.w * d : g - d * c.omw;               // at::lerp's two branches
    u = fmaxf(u * c.b2, fabsf(g) + c.eps);
    pv = pv + c.neg_clr * (m / u);
}

__global__ __launch_bounds__(256) void adamax_multi_kernel(const AdamaxChunk c, int cnt, double lr, const double* __restrict__ lr_dev, double beta1,
                                                           double beta2, float eps, float wd) {
    const int t = mt_find(c.blk0, cnt, blockIdx.x);
    const int64_t base = (int64_t)(blockIdx.x - c.blk0[t]) * MT_ELEMS, n = c.n[t];
    float* __restrict__ p = c.p[t];
    const float* __restrict__ g = c.g[t];
    float* __restrict__ m = c.m[t];
    float* __restrict__ u = c.u[t];
    if (*c.step[t] < 1) return;                                 // a count that was never advanced: 1 - b1^0 = 0
    const AdamaxCoef k = adamax_coef(lr, lr_dev, beta1, beta2, eps, wd, c.step[t]);
    const bool al = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)u)) & 15) == 0;
    if (al && base + MT_ELEMS <= n) {
#pragma unroll
        for (int j = 0; j < MT_ELEMS / 1024; ++j) {
            const int64_t i = base + j * 1024 + threadIdx.x * 4;
            f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
            f32x4 mv = *reinterpret_cast<const f32x4*>(m + i), uv = *reinterpret_cast<const f32x4*>(u + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pv[e], me = mv[e], ue = uv[e];
                adamax_elem(k, pe, gv[e], me, ue);
                pv[e] = pe, mv[e] = me, uv[e] = ue;
            }
            *reinterpret_cast<f32x4*>(m + i) = mv;
            *reinterpret_cast<f32x4*>(u + i) = uv;
            *reinterpret_cast<f32x4*>(p + i) = pv;
        }
        return;
    }
    for (int64_t i = base + threadIdx.x; i < min(base + (int64_t)MT_ELEMS, n); i += 256) {
        float pv = p[i], mi = m[i], ui = u[i];
        adamax_elem(k, pv, g[i], mi, ui);
        m[i] = mi;
        u[i] = ui;
        p[i] = pv;
    }
}

// log[(t - 1) * count + j] = *src[j] for t = *step; nothing is written for t < 1 or t - 1 >= rows
__global__ void scalar_log_kernel(const LogSrc s, int count, const int64_t* __restrict__ step, float* __restrict__ log, int64_t rows) {
    const int j = threadIdx.x;
    if (j >= count) return;
    const int64_t t = *step;
    if (t < 1 || t - 1 >= rows) return;
    log[(t - 1) * count + j] = *s.src[j];
}

}  // namespace

extern "C" int e4s_sgd_multi_dev_f32(int count, float* const* p, const float* const* grad, float* const* buf, const int64_t* n, double lr,
                                     const double* lr_dev, double momentum, double dampening, double weight_decay, void* stream) {
    const bool mom = momentum != 0.0;
    if (count < 0 || (count && (!p || !grad || !n || (mom && !buf)))) return (int)hipErrorInvalidValue;
    hipStream_t st = as_stream(stream);
    int i = 0;
    while (i < count) {
        SgdChunk c;
        int cnt = 0;
        int64_t blocks = 0;
        c.blk0[0] = 0;
        while (i < count && cnt < MT) {
            if (n[i] > 0) {
                if (!p[i] || !grad[i] || (mom && !buf[i])) return (int)hipErrorInvalidValue;
                const int64_t nb = (n[i] + MT_ELEMS - 1) / MT_ELEMS;
                if (blocks + nb > 0x7fffffff) { if (cnt) break; return (int)hipErrorInvalidValue; }
                c.p[cnt] = p[i], c.g[cnt] = grad[i], c.buf[cnt] = mom ? buf[i] : nullptr, c.n[cnt] = n[i];
                blocks += nb;
                c.blk0[++cnt] = (int)blocks;
            }
            ++i;
        }
        if (!cnt) continue;
        if (mom)
            hipLaunchKernelGGL(sgd_multi_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, c, cnt, lr, lr_dev, (float)momentum,
                               (float)(1.0 - dampening), (float)weight_decay);
        else
            hipLaunchKernelGGL(sgd_multi_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, c, cnt, lr, lr_dev, 0.f, 1.f,
                               (float)weight_decay);
        E4S_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int e4s_adamax_multi_dev_f32(int count, float* const* p, const float* const* grad, float* const* m, float* const* u, const int64_t* n,
                                        const int64_t* const* step, double lr, const double* lr_dev, double beta1, double beta2, double eps,
                                        double weight_decay, void* stream) {
    if (count < 0 || (count && (!p || !grad || !m || !u || !n || !step))) return (int)hipErrorInvalidValue;
    hipStream_t st = as_stream(stream);
    int i = 0;
    while (i < count) {
        AdamaxChunk c;
        int cnt = 0;
        int64_t blocks = 0;
        c.blk0[0] = 0;
        while (i < count && cnt < MT) {
            if (n[i] > 0) {
                if (!p[i] || !grad[i] || !m[i] || !u[i] || !step[i]) return (int)hipErrorInvalidValue;
                const int64_t nb = (n[i] + MT_ELEMS - 1) / MT_ELEMS;
                if (blocks + nb > 0x7fffffff) { if (cnt) break; return (int)hipErrorInvalidValue; }
                c.p[cnt] = p[i], c.g[cnt] = grad[i], c.m[cnt] = m[i], c.u[cnt] = u[i], c.step[cnt] = step[i], c.n[cnt] = n[i];
                blocks += nb;
                c.blk0[++cnt] = (int)blocks;
            }
            ++i;
        }
        if (!cnt) continue;
        hipLaunchKernelGGL(adamax_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, st, c, cnt, lr, lr_dev, beta1, beta2, (float)eps,
                           (float)weight_decay);
        E4S_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int e4s_scalar_log_f32(int count, const float* const* src, const int64_t* step_dev, float* log, int64_t rows, void* stream) {
    if (count < 0 || count > 16 || rows < 0 || (count && (!src || !step_dev || !log))) return (int)hipErrorInvalidValue;
    if (count == 0 || rows == 0) return 0;
    LogSrc s;
    for (int j = 0; j < 16; ++j) {
        if (j < count && !src[j]) return (int)hipErrorInvalidValue;
        s.src[j] = j < count ? src[j] : nullptr;
    }
    hipLaunchKernelGGL(scalar_log_kernel, dim3(1), dim3(64), 0, as_stream(stream), s, count, step_dev, log, rows);
    E4S_CHECK_LAUNCH();
    return 0;
}
