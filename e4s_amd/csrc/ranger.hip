// Ranger (RAdam + Lookahead + gradient centralisation, src/training/ranger.py:78-164) as a multi-tensor, capturable step in the style of
// adam_multi_kernel (optim.hip): pointers BY VALUE in the kernel arguments, step counts and learning rate in device memory.  What Ranger
// adds to Adam: a per-row sum of the gradient BEFORE the update (the centralisation subtracts each row's mean) and two data-dependent
// branches -- RAdam's rectification test and Lookahead's `step % k` -- which are decided in the kernel from the device step count, so
// a replayed HIP graph takes the right one on every step.
//
// Two phases per launch chunk of RG_MT tensors:
//   (a) ranger_rowsum_kernel   ws[off + row * nseg + seg] = sum of segment `seg` (RG_ELEMS elements) of row `row` of g, for the centralised
//                              tensors only.  A row of <= RG_ELEMS elements is ONE segment summed by one wave; a longer row is cut into
//                              nseg = ceil(L / RG_ELEMS) segments, one block each (four waves x 1024 elements, added in wave order).
//   (b) ranger_update_kernel   the fused update of p, m, v (and slow on Lookahead steps), RG_ELEMS elements per block.  It subtracts the row
//                              mean as it reads g: the centralised gradient never goes to memory and p.grad is left as it was.  A block of
//                              a long-row tensor touches at most two rows and adds their nseg segment sums itself, in a fixed order.
// Order of every row sum (no floating-point atomics; the same bits on every run, with any launch-mates and for any alignment): inside a
// wave's range lane l accumulates the four elements 256 j + 4 l .. + 3 separately over j, adds them as (a0 + a1) + (a2 + a3), and the lanes
// are added by the xor butterfly of wave_sum; waves, and the per-thread strides over the segment sums, are added in index order.
// Traffic per element and step: 32 B for a centralised tensor (g twice; p, m, v read and written), 28 B otherwise, + 8 B for slow on
// a Lookahead step.
#include "common.h"

namespace {

constexpr int RG_MT = 40;           // tensors per launch: 80 B each in the arguments (AdamChunk's 52 B allow 48)
constexpr int RG_ELEMS = 4096;      // elements per update block == elements per row segment

struct RangerChunk {
    float* p[RG_MT];
    const float* g[RG_MT];
    float* m[RG_MT];
    float* v[RG_MT];
    float* slow[RG_MT];
    const int64_t* step[RG_MT];
    int64_t n[RG_MT];
    int64_t row_len[RG_MT];         // 0: not centralised
    int64_t ws_off[RG_MT];          // first float of the tensor's segment sums in the workspace
    int blk0[RG_MT + 1];            // update blocks
    int blk0a[RG_MT + 1];           // row-sum blocks (none for a tensor that is not centralised)
};
// the kernel-argument segment is 4 KiB; the scalars behind the struct and the hidden arguments of the code object need ~350 B of it
static_assert(sizeof(RangerChunk) <= 3584, "RangerChunk must leave room in the 4 KiB kernel-argument segment");

__device__ __forceinline__ int rg_find(const int* blk0, int cnt, int b) {
    int lo = 0, hi = cnt;                                       // blk0[lo] <= b < blk0[hi]  (an empty range is never the answer)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk0[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// elements q[0 .. min(rem, 4)) and zeros behind them; `vec`: q is 16-byte aligned
__device__ __forceinline__ f32x4 rg_load4(const float* __restrict__ q, int64_t rem, bool vec) {
    if (vec && rem >= 4) return *reinterpret_cast<const f32x4*>(q);
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (rem > 0) r[0] = q[0];
    if (rem > 1) r[1] = q[1];
    if (rem > 2) r[2] = q[2];
    if (rem > 3) r[3] = q[3];
    return r;
}

// sum of q[0 .. len) by one wave, the same bits on every lane (the order is the one in the header of this file, whatever the alignment)
__device__ __forceinline__ float rg_wave_range_sum(const float* __restrict__ q, int64_t len, int lane) {
    const bool vec = (((uintptr_t)q) & 15) == 0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = lane * 4; i < len; i += 256) acc += rg_load4(q + i, len - i, vec);
    return wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
}

__global__ __launch_bounds__(256) void ranger_rowsum_kernel(const RangerChunk c, int cnt, float* __restrict__ ws) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int t = rg_find(c.blk0a, cnt, blockIdx.x);
    const int64_t L = c.row_len[t], rows = c.n[t] / L;
    const int64_t lb = (int64_t)blockIdx.x - c.blk0a[t];
    const float* __restrict__ g = c.g[t];
    float* __restrict__ out = ws + c.ws_off[t];
    if (L <= RG_ELEMS) {                                        // four rows per block, a wave each
        const int64_t row = lb * 4 + wv;
        if (row < rows) {
            const float s = rg_wave_range_sum(g + row * L, L, lane);
            if (lane == 0) out[row] = s;
        }
        return;
    }
    const int64_t nseg = (L + RG_ELEMS - 1) / RG_ELEMS;
    const int64_t row = lb / nseg, seg = lb - row * nseg;
    const int64_t s0 = seg * RG_ELEMS + wv * 1024;              // this wave's quarter of the segment
    const int64_t len = min((int64_t)1024, L - s0);             // (<= 0: the row ends before it)
    const float s = rg_wave_range_sum(g + row * L + s0, len, lane);
    if (lane == 0) red[wv] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[lb] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct RangerCoef {
    float b1, b2, omb1, omb2, eps, alpha;
    float neg_step;                 // -(step_size * lr), the product formed in double
    float wdlr;                     // -(weight_decay * lr), likewise; 0: no decay
    int adaptive, look, live;
};

// src/training/ranger.py:127-143,146,151-153,159 for the step count in device memory, in double as Python evaluates it
__device__ __forceinline__ RangerCoef ranger_coef(const int64_t* step, double lr, const double* lr_dev, double beta1, double beta2, float eps,
                                                  double wd, float alpha, int k, double thr) {
    RangerCoef c;
    const int64_t ts = *step;
    if (lr_dev) lr = *lr_dev;
    const double t = (double)ts;
    const double beta2_t = pow(beta2, t);
    const double nmax = 2.0 / (1.0 - beta2) - 1.0;
    const double nsma = nmax - 2.0 * t * beta2_t / (1.0 - beta2_t);
    const double bc1 = 1.0 - pow(beta1, t);
    c.adaptive = nsma > thr;
    double step_size;
    if (c.adaptive)
        step_size = sqrt((1.0 - beta2_t) * (nsma - 4.0) / (nmax - 4.0) * (nsma - 2.0) / nsma * nmax / (nmax - 2.0)) / bc1;
    else
        step_size = 1.0 / bc1;
    c.neg_step = (float)(-step_size * lr);
    c.wdlr = wd != 0.0 ? (float)(-wd * lr) : 0.f;
    c.b1 = (float)beta1, c.b2 = (float)beta2, c.omb1 = (float)(1.0 - beta1), c.omb2 = (float)(1.0 - beta2), c.eps = eps, c.alpha = alpha;
    c.look = ts % k == 0;
    c.live = ts >= 1;               // a count that was not advanced: the tensor is left alone
    return c;
}

// one element; `g` is the centralised gradient.  Every product-sum is an explicit fma, so the scalar and the 16-byte path round alike.
__device__ __forceinline__ void ranger_elem(const RangerCoef& c, float& p, float g, float& m, float& v) {
    v = __fmaf_rn(c.omb2 * g, g, v * c.b2);                      // exp_avg_sq.mul_(beta2).addcmul_(1 - beta2, grad, grad)
    m = __fmaf_rn(c.omb1, g, m * c.b1);                          // exp_avg.mul_(beta1).add_(1 - beta1, grad)
    if (c.wdlr != 0.f) p = __fmaf_rn(c.wdlr, p, p);              // p.add_(-wd * lr, p)
    if (c.adaptive) p = __fmaf_rn(c.neg_step, m / (sqrtf(v) + c.eps), p);      // p.addcdiv_(-step_size * lr, exp_avg, sqrt(v) + eps)
    else p = __fmaf_rn(c.neg_step, m, p);                        // p.add_(-step_size * lr, exp_avg)
}

// ordered sum of the nseg segment sums of one row by the whole block; every thread returns the same bits
__device__ __forceinline__ float rg_block_row_sum(const float* __restrict__ part, int64_t nseg, float* red) {
    float a = 0.f;
    for (int64_t j = threadIdx.x; j < nseg; j += 256) a += part[j];
    a = wave_sum(a);
    __syncthreads();                                            // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void ranger_update_kernel(const RangerChunk c, int cnt, const float* __restrict__ ws, double lr,
                                                            const double* __restrict__ lr_dev, double beta1, double beta2, float eps, double wd,
                                                            float alpha, int k, double thr) {
    __shared__ RangerCoef coef;
    __shared__ float red[4];
    const int t = rg_find(c.blk0, cnt, blockIdx.x);
    if (threadIdx.x == 0) coef = ranger_coef(c.step[t], lr, lr_dev, beta1, beta2, eps, wd, alpha, k, thr);
    __syncthreads();
    RangerCoef q = coef;
    q.adaptive = __builtin_amdgcn_readfirstlane(q.adaptive);     // block-uniform: scalar branches
    q.look = __builtin_amdgcn_readfirstlane(q.look);
    if (!__builtin_amdgcn_readfirstlane(q.live)) return;
    const int64_t base = (int64_t)(blockIdx.x - c.blk0[t]) * RG_ELEMS, n = c.n[t];
    float* __restrict__ p = c.p[t];
    const float* __restrict__ g = c.g[t];
    float* __restrict__ m = c.m[t];
    float* __restrict__ v = c.v[t];
    float* __restrict__ slow = c.slow[t];
    // the row mean of element base + j:  mode 0 none;  mode 1 (rows of <= RG_ELEMS elements) ws[row] / L with row = row0 + (rem0 + j) / L;
    // mode 2 (longer rows: at most two in a block) mean0 for j < edge, mean1 behind it
    const int64_t L = c.row_len[t];
    const int mode = L == 0 ? 0 : (L <= RG_ELEMS ? 1 : 2);
    const float* __restrict__ rs = ws + c.ws_off[t];
    const float Lf = (float)L;
    uint32_t L32 = 1, rem0 = 0;
    int64_t row0 = 0;
    int edge = RG_ELEMS;
    float mean0 = 0.f, mean1 = 0.f;
    if (mode) {
        row0 = base / L;
        const int64_t r0 = base - row0 * L;
        if (mode == 1) {
            L32 = (uint32_t)L, rem0 = (uint32_t)r0;
        } else {
            const int64_t nseg = (L + RG_ELEMS - 1) / RG_ELEMS;
            mean0 = rg_block_row_sum(rs + row0 * nseg, nseg, red) / Lf;
            if (L - r0 < RG_ELEMS) {
                edge = (int)(L - r0);
                if (base + edge < n) mean1 = rg_block_row_sum(rs + (row0 + 1) * nseg, nseg, red) / Lf;
            }
        }
    }
    const bool al = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)slow)) & 15) == 0;
    if (al && base + RG_ELEMS <= n) {
#pragma unroll
        for (int jj = 0; jj < RG_ELEMS / 1024; ++jj) {
            const int j = jj * 1024 + threadIdx.x * 4;
            const int64_t i = base + j;
            f32x4 pv = *reinterpret_cast<const f32x4*>(p + i), gv = *reinterpret_cast<const f32x4*>(g + i);
            f32x4 mv = *reinterpret_cast<const f32x4*>(m + i), vv = *reinterpret_cast<const f32x4*>(v + i);
            if (mode == 1) {
                uint32_t row = (rem0 + (uint32_t)j) / L32, r = (rem0 + (uint32_t)j) - row * L32;
                float mean = rs[row0 + row] / Lf;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (r >= L32) { r = 0; ++row; mean = rs[row0 + row] / Lf; }
                    gv[e] -= mean;
                    ++r;
                }
            } else if (mode == 2) {
#pragma unroll
                for (int e = 0; e < 4; ++e) gv[e] -= j + e < edge ? mean0 : mean1;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pv[e], me = mv[e], ve = vv[e];
                ranger_elem(q, pe, gv[e], me, ve);
                pv[e] = pe, mv[e] = me, vv[e] = ve;
            }
            *reinterpret_cast<f32x4*>(m + i) = mv;
            *reinterpret_cast<f32x4*>(v + i) = vv;
            if (q.look) {                                       // slow += alpha (p - slow); p = slow
                f32x4 sv = *reinterpret_cast<const f32x4*>(slow + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) sv[e] = __fmaf_rn(q.alpha, pv[e] - sv[e], sv[e]);
                *reinterpret_cast<f32x4*>(slow + i) = sv;
                pv = sv;
            }
            *reinterpret_cast<f32x4*>(p + i) = pv;
        }
        return;
    }
    const int jend = (int)min((int64_t)RG_ELEMS, n - base);
    for (int j = threadIdx.x; j < jend; j += 256) {
        const int64_t i = base + j;
        float gi = g[i];
        if (mode == 1) gi -= rs[row0 + (rem0 + (uint32_t)j) / L32] / Lf;
        else if (mode == 2) gi -= j < edge ? mean0 : mean1;
        float pe = p[i], me = m[i], ve = v[i];
        ranger_elem(q, pe, gi, me, ve);
        m[i] = me;
        v[i] = ve;
        if (q.look) {
            const float se = slow[i];
            pe = __fmaf_rn(q.alpha, pe - se, se);
            slow[i] = pe;
        }
        p[i] = pe;
    }
}

// floats of segment sums of one tensor (0: not centralised)
inline int64_t rg_ws_floats(int64_t n, int64_t row_len) {
    if (n <= 0 || row_len <= 0) return 0;
    return n / row_len * ((row_len + RG_ELEMS - 1) / RG_ELEMS);
}

}  // namespace

extern "C" int64_t e4s_ranger_multi_ws_floats(int count, const int64_t* n, const int64_t* row_len) {
    if (count < 0 || (count && (!n || !row_len))) return -1;
    int64_t total = 0;
    for (int i = 0; i < count; ++i) {
        if (n[i] > 0 && (row_len[i] < 0 || (row_len[i] > 0 && n[i] % row_len[i]))) return -1;
        total += rg_ws_floats(n[i], row_len[i]);
    }
    return total;
}

extern "C" int e4s_ranger_multi_dev_f32(int count, float* const* p, const float* const* grad, float* const* m, float* const* v, float* const* slow,
                                        const int64_t* n, const int64_t* row_len, const int64_t* const* step, float* ws, int64_t ws_floats,
                                        double lr, const double* lr_dev, double beta1, double beta2, double eps, double weight_decay, double alpha,
                                        int k, double nsma_threshold, void* stream) {
    if (count < 0 || (count && (!p || !grad || !m || !v || !slow || !n || !row_len || !step)) || k < 1) return (int)hipErrorInvalidValue;
    const int64_t need = e4s_ranger_multi_ws_floats(count, n, row_len);
    if (need < 0 || need > ws_floats || (need > 0 && !ws)) return (int)hipErrorInvalidValue;
    for (int i = 0; i < count; ++i)
        if (n[i] > 0 && (!p[i] || !grad[i] || !m[i] || !v[i] || !slow[i] || !step[i])) return (int)hipErrorInvalidValue;
    hipStream_t st = as_stream(stream);
    int64_t off = 0;
    int i = 0;
    while (i < count) {
        RangerChunk c;
        int cnt = 0;
        int64_t blocks = 0, blocks_a = 0;
        c.blk0[0] = 0, c.blk0a[0] = 0;
        while (i < count && cnt < RG_MT) {
            if (n[i] > 0) {
                const int64_t L = row_len[i], nb = (n[i] + RG_ELEMS - 1) / RG_ELEMS;
                const int64_t parts = rg_ws_floats(n[i], L);
                const int64_t na = L == 0 ? 0 : (L <= RG_ELEMS ? (n[i] / L + 3) / 4 : parts);
                if (blocks + nb > 0x7fffffff || blocks_a + na > 0x7fffffff) { if (cnt) break; return (int)hipErrorInvalidValue; }
                c.p[cnt] = p[i], c.g[cnt] = grad[i], c.m[cnt] = m[i], c.v[cnt] = v[i], c.slow[cnt] = slow[i], c.step[cnt] = step[i];
                c.n[cnt] = n[i], c.row_len[cnt] = L, c.ws_off[cnt] = off;
                off += parts;
                blocks += nb, blocks_a += na;
                ++cnt;
                c.blk0[cnt] = (int)blocks, c.blk0a[cnt] = (int)blocks_a;
            }
            ++i;
        }
        if (!cnt) continue;
        if (blocks_a > 0) {
            hipLaunchKernelGGL(ranger_rowsum_kernel, dim3((unsigned)blocks_a), dim3(256), 0, st, c, cnt, ws);
            E4S_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(ranger_update_kernel, dim3((unsigned)blocks), dim3(256), 0, st, c, cnt, (const float*)ws, lr, lr_dev, beta1, beta2,
                           (float)eps, weight_decay, (float)alpha, k, nsma_threshold);
        E4S_CHECK_LAUNCH();
    }
    return 0;
}
