// RetinaFace-R50 (e4s_amd/retinaface.py; src/pretrained/gpen/face_detect/): the zero-padded conv family of the whole network, the
// frame preparation, the fused heads with prior + decode, and the selection + greedy NMS.
//
// Conv family (e4s_rconv_f32): 1x1 and 3x3, stride 1 and 2, zero padding k / 2, NHWC fp32, Cin a multiple of 32, Cout of 64, ANY
// H and W: Ho = (H + 2 pad - k) / s + 1 (ceil(H / 2) at stride 2).  It is an implicit GEMM over the flattened output pixels M = B Ho
// Wo on the tile of gather_gemm.h (RconvGather, RconvEpi below): a block computes 128 pixels x BN output channels (BN = 128 when Cout
// allows, else 64), so the input is staged once per 128 (64) output channels, not once per 32 -- the 1x1 convs that read up to 2048
// channels dominate the network.  The gathered pixel rows are zero where the tap leaves the image or the row is past M; the weight
// rows are pre-packed by e4s_rconv_pack_f32 in row blocks of 64 channels.  Arithmetic: split-bf16 or exact fp32 from the same tile
// code.  The summation order of an output is (tap, chunk, k-step) whatever the batch or the tile's place.
//   epilogue  v = acc + bias[c] (eval BatchNorm folded on the host); r0_mode 1: v += r0; act: v = v > 0 ? v : v * slope (slope 0 is
//             ReLU); r0_mode 2: v += r0.  r0 is an NHWC map at the output resolution, or, with r0_H / r0_W set, a smaller map read
//             through a nearest upsampling to Ho x Wo (source index min(floor(dst * (float(in) / float(out))), in - 1), ATen's own
//             float arithmetic): the upsampled map is never written.  The result lands at channel offset y_coff of a wider buffer.
// Prep:   uint8 BGR HWC -> fp32 NHWC minus (104, 117, 123), optionally through a bilinear shrink with half-pixel centres.
// Head:   per pyramid level the three 1x1 heads (256 -> 2 anchors x (4 loc + 2 conf + 10 landmarks) = 32 columns) in one pass, the
//         2-class softmax, the cell's prior computed from (i, j, step, min_size, image size) as prior_box.py:21-28 does (in double,
//         rounded to float: no prior table), decode / decode_landm with variances (0.1, 0.2) and the scaling to pixels.
// Select: score > threshold on the score-sorted list (ties: lower prior index first, from a stable sort), the top_k cut, greedy NMS
//         as py_cpu_nms.py:18-36 (+ 1 areas, suppression when not ovr <= thresh), keep_top_k, the landmark re-layout to five x then
//         five y and the final / ss.  One block per image; fixed-capacity outputs and a device count.
#include "gather_gemm.h"                                        // the conv family's tile (gather_gemm_kernel) and its weight packer

#pragma clang fp contract(off)

namespace {

// Gather of gather_gemm.h: output pixel m = (b, oy, ox) of [B,Ho,Wo] reads input pixel (oy stride - pad + ky, ox stride - pad + kx),
// k and stride at run time; a tap that leaves the image is not live.
struct RconvGather {
    const float* x;
    int Hi, Wi, x_cstride, k, stride, Ho, Wo;
    struct Item { int b, y, x, c; bool live; };
    struct Tap { int ky, kx; };
    __device__ __forceinline__ int ntaps() const { return k * k; }
    __device__ __forceinline__ Item item(int m, bool live, int q) const {
        const int pad = k >> 1;
        const int mm = live ? m : 0;
        const int ox = mm % Wo, t = mm / Wo;
        return Item{t / Ho, (t % Ho) * stride - pad, ox * stride - pad, q * 8, live};
    }
    __device__ __forceinline__ Tap tap(int t) const {
        const int ky = t / k;
        return Tap{ky, t - ky * k};
    }
    __device__ __forceinline__ bool src(const Item& it, const Tap& t, int chunk, const float*& ptr) const {
        const int iy = it.y + t.ky, ix = it.x + t.kx;
        const bool ok = it.live && (unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi;
        ptr = x + (((size_t)it.b * Hi + (ok ? iy : 0)) * Wi + (ok ? ix : 0)) * x_cstride + chunk * KC + it.c;
        return ok;
    }
};

// Epi of gather_gemm.h: the epilogue of the file header (bias, r0 before or after the activation, r0 through the nearest upsampling)
struct RconvEpi {
    const float* bias_p;                                        // bias [Cout] or null
    const float* r0;
    float* y;
    int Ho, Wo, y_cstride, y_coff, r0_cstride, r0_H, r0_W, r0_mode, act;
    float slope;
    __device__ __forceinline__ float bias(int c) const { return bias_p ? bias_p[c] : 0.f; }
    __device__ __forceinline__ void store(int pix, int c, f32x4 v) const {
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (r0) {
            size_t rpix = (size_t)pix;
            if (r0_H > 0) {
                const int ox = pix % Wo, t = pix / Wo;
                const int oy = t % Ho, b = t / Ho;
                rpix = ((size_t)b * r0_H + nearest_src(oy, r0_H, Ho)) * r0_W + nearest_src(ox, r0_W, Wo);
            }
            r = *reinterpret_cast<const f32x4*>(r0 + rpix * r0_cstride + c);
        }
        if (r0_mode == 1) v = v + r;
        if (act) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * slope;
        }
        if (r0_mode == 2) v = v + r;
        *reinterpret_cast<f32x4*>(y + (size_t)pix * y_cstride + y_coff + c) = v;
    }
};

// ---- prep: uint8 BGR HWC -> fp32 NHWC minus the channel means, optionally through a half-pixel bilinear shrink ----
__global__ __launch_bounds__(256) void prep_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int H, int W, int Hd, int Wd,
                                                   int shrink, double scale, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % Wd), y = (int)((i / Wd) % Hd);
    const int64_t b = i / ((int64_t)Wd * Hd);
    const float mean[3] = {104.f, 117.f, 123.f};
    const uint8_t* img = src + b * H * W * 3;
    float v[3];
    if (!shrink) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)img[((int64_t)y * W + x) * 3 + c];
    } else {
        const double sy = ((double)y + 0.5) * scale - 0.5, sx = ((double)x + 0.5) * scale - 0.5;
        int y0 = (int)floor(sy), x0 = (int)floor(sx);
        float fy = (float)(sy - (double)y0), fx = (float)(sx - (double)x0);
        if (y0 < 0) { y0 = 0; fy = 0.f; }
        if (x0 < 0) { x0 = 0; fx = 0.f; }
        if (y0 >= H - 1) { y0 = H - 1; fy = 0.f; }
        if (x0 >= W - 1) { x0 = W - 1; fx = 0.f; }
        const int y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p00 = (float)img[((int64_t)y0 * W + x0) * 3 + c], p01 = (float)img[((int64_t)y0 * W + x1) * 3 + c];
            const float p10 = (float)img[((int64_t)y1 * W + x0) * 3 + c], p11 = (float)img[((int64_t)y1 * W + x1) * 3 + c];
            const float top = p00 * (1.f - fx) + p01 * fx, bot = p10 * (1.f - fx) + p11 * fx;
            v[c] = top * (1.f - fy) + bot * fy;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[i * 3 + c] = v[c] - mean[c];
}

// ---- priors and decode ----
struct Prior { float cx, cy, w, h; };

// prior_box.py:21-28 for one (level row i, column j, min_size): Python doubles, rounded to float by torch.Tensor(anchors)
__device__ __forceinline__ Prior make_prior(int i, int j, int step, float min_size, int imH, int imW) {
    Prior q;
    q.cx = (float)(((double)j + 0.5) * (double)step / (double)imW);
    q.cy = (float)(((double)i + 0.5) * (double)step / (double)imH);
    q.w = (float)((double)min_size / (double)imW);
    q.h = (float)((double)min_size / (double)imH);
    return q;
}

// box_utils.py decode / decode_landm with variances (0.1, 0.2), then * (W, H, ...) / resize (retinaface_detection.py:85-94)
__device__ __forceinline__ void decode_store(const float* loc, const float* lm, float score, const Prior q, const e4s_retina_geom& g,
                                             int64_t n, float* __restrict__ boxes, float* __restrict__ scores, float* __restrict__ landms) {
    const float W = (float)g.imW, H = (float)g.imH;
    const float cx = q.cx + loc[0] * 0.1f * q.w, cy = q.cy + loc[1] * 0.1f * q.h;
    const float bw = q.w * expf(loc[2] * 0.2f), bh = q.h * expf(loc[3] * 0.2f);
    const float x1 = cx - bw / 2.f, y1 = cy - bh / 2.f;
    const float x2 = bw + x1, y2 = bh + y1;
    *reinterpret_cast<f32x4*>(boxes + n * 4) = f32x4{x1 * W / g.resize, y1 * H / g.resize, x2 * W / g.resize, y2 * H / g.resize};
    scores[n] = score;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        landms[n * 10 + 2 * k] = (q.cx + lm[2 * k] * 0.1f * q.w) * W / g.resize;
        landms[n * 10 + 2 * k + 1] = (q.cy + lm[2 * k + 1] * 0.1f * q.h) * H / g.resize;
    }
}

// F.softmax over two classes, the second one's probability
__device__ __forceinline__ void softmax2(float a, float b, float& pa, float& pb) {
    const float m = fmaxf(a, b);
    const float ea = expf(a - m), eb = expf(b - m);
    const float s = ea + eb;
    pa = ea / s;
    pb = eb / s;
}

constexpr int HC = 256, HCELLS = 8;                             // head: 256 input channels, 8 cells x 32 columns per block

// column o = anchor * 16 + t: t 0..3 loc, 4..5 conf, 6..15 landmarks.  wp [256][32], bias [32].
__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ x, int x_cs, const float* __restrict__ wp,
                                                   const float* __restrict__ bias, const e4s_retina_geom g, int level, int64_t ncell,
                                                   float* __restrict__ boxes, float* __restrict__ scores, float* __restrict__ landms,
                                                   float* __restrict__ raw_loc, float* __restrict__ raw_conf, float* __restrict__ raw_lm) {
    __shared__ __attribute__((aligned(16))) float s_x[HCELLS][HC];
    __shared__ float s_raw[HCELLS][32];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * HCELLS;
    for (int k = tid; k < HCELLS * HC / 4; k += 256) {
        const int cell = k / (HC / 4), c4 = k % (HC / 4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c0 + cell < ncell) v = *reinterpret_cast<const f32x4*>(x + (c0 + cell) * x_cs + c4 * 4);
        *reinterpret_cast<f32x4*>(&s_x[cell][c4 * 4]) = v;
    }
    __syncthreads();
    const int cell = tid >> 5, o = tid & 31;
    float acc = 0.f;
#pragma unroll 8
    for (int c = 0; c < HC; ++c) acc = fmaf(s_x[cell][c], wp[c * 32 + o], acc);
    s_raw[cell][o] = acc + bias[o];
    __syncthreads();
    if (o >= 2 || c0 + cell >= ncell) return;
    const int a = o;
    const float* r = &s_raw[cell][a * 16];
    const int64_t gc = c0 + cell;
    const int lh = g.lh[level], lw = g.lw[level];
    const int j = (int)(gc % lw), i = (int)((gc / lw) % lh);
    const int64_t b = gc / ((int64_t)lw * lh);
    const int64_t n = b * g.N + g.base[level] + ((int64_t)i * lw + j) * 2 + a;
    float loc[4], lm[10], pa, pb;
#pragma unroll
    for (int k = 0; k < 4; ++k) loc[k] = r[k];
#pragma unroll
    for (int k = 0; k < 10; ++k) lm[k] = r[6 + k];
    softmax2(r[4], r[5], pa, pb);
    if (raw_loc) {
#pragma unroll
        for (int k = 0; k < 4; ++k) raw_loc[n * 4 + k] = loc[k];
        raw_conf[n * 2] = pa;
        raw_conf[n * 2 + 1] = pb;
#pragma unroll
        for (int k = 0; k < 10; ++k) raw_lm[n * 10 + k] = lm[k];
    }
    decode_store(loc, lm, pb, make_prior(i, j, g.step[level], g.min_size[level][a], g.imH, g.imW), g, n, boxes, scores, landms);
}

// the same decode from the network's raw outputs (loc [B,N,4], conf [B,N,2] after the softmax, landms [B,N,10])
__global__ __launch_bounds__(256) void decode_kernel(const float* __restrict__ rloc, const float* __restrict__ rconf,
                                                     const float* __restrict__ rlm, const e4s_retina_geom g, int64_t total,
                                                     float* __restrict__ boxes, float* __restrict__ scores, float* __restrict__ landms) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= total) return;
    const int pi = (int)(n % g.N);
    int level = 0;
    if (g.nlevel > 1 && pi >= g.base[1]) level = 1;
    if (g.nlevel > 2 && pi >= g.base[2]) level = 2;
    const int rel = pi - g.base[level];
    const int a = rel & 1, cellidx = rel >> 1;
    const int j = cellidx % g.lw[level], i = cellidx / g.lw[level];
    float loc[4], lm[10];
#pragma unroll
    for (int k = 0; k < 4; ++k) loc[k] = rloc[n * 4 + k];
#pragma unroll
    for (int k = 0; k < 10; ++k) lm[k] = rlm[n * 10 + k];
    decode_store(loc, lm, rconf[n * 2 + 1], make_prior(i, j, g.step[level], g.min_size[level][a], g.imH, g.imW), g, n, boxes, scores,
                 landms);
}

// ---- selection + greedy NMS: one block per image ----
// skeys / sidx [B,N]: the scores sorted descending (stable: equal scores keep the lower prior index first) and their prior indices.
__global__ __launch_bounds__(256) void select_kernel(const float* __restrict__ boxes, const float* __restrict__ landms,
                                                     const float* __restrict__ skeys, const int64_t* __restrict__ sidx, int N, float conf_thr,
                                                     float nms_thr, int top_k, int K, float ss, float* __restrict__ dets,
                                                     float* __restrict__ lm_out, int* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    int* s_keep = reinterpret_cast<int*>(s_dyn);                // [K]
    unsigned char* s_supp = s_dyn + (size_t)K * 4;              // [min(top_k, N)]
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* keys = skeys + (size_t)b * N;
    const int64_t* idx = sidx + (size_t)b * N;
    const float* bx = boxes + (size_t)b * N * 4;
    // number of scores above the threshold: the first position of the descending list that is not (every thread, the same search)
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] > conf_thr) lo = mid + 1; else hi = mid;
    }
    const int n = lo < top_k ? lo : top_k;
    for (int j = tid; j < n; j += 256) s_supp[j] = 0;
    __syncthreads();
    int nk = 0;
    for (int i = 0; i < n && nk < K; ++i) {
        if (s_supp[i]) continue;                                // written before the last barrier: every thread sees the same
        if (tid == 0) s_keep[nk] = i;
        ++nk;
        const f32x4 bi = *reinterpret_cast<const f32x4*>(bx + idx[i] * 4);
        const float area_i = (bi[2] - bi[0] + 1.f) * (bi[3] - bi[1] + 1.f);
        for (int j = i + 1 + tid; j < n; j += 256) {
            if (s_supp[j]) continue;
            const f32x4 bj = *reinterpret_cast<const f32x4*>(bx + idx[j] * 4);
            const float area_j = (bj[2] - bj[0] + 1.f) * (bj[3] - bj[1] + 1.f);
            const float xx1 = fmaxf(bi[0], bj[0]), yy1 = fmaxf(bi[1], bj[1]);
            const float xx2 = fminf(bi[2], bj[2]), yy2 = fminf(bi[3], bj[3]);
            const float w = fmaxf(0.f, xx2 - xx1 + 1.f), h = fmaxf(0.f, yy2 - yy1 + 1.f);
            const float inter = w * h;
            const float ovr = inter / (area_i + area_j - inter);
            if (!(ovr <= nms_thr)) s_supp[j] = 1;
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) counts[b] = nk;
    for (int t = tid; t < K * 15; t += 256) {
        const int r = t / 15, c = t - r * 15;
        float v = 0.f;
        if (r < nk) {
            const int i = s_keep[r];
            const int64_t pi = idx[i];
            if (c < 4) v = bx[pi * 4 + c] / ss;
            else if (c == 4) v = keys[i] / ss;
            else {
                const int q = c - 5;                            // five x, then five y
                v = landms[((size_t)b * N + pi) * 10 + (q < 5 ? 2 * q : 2 * (q - 5) + 1)] / ss;
            }
        }
        if (c < 5) dets[((size_t)b * K + r) * 5 + c] = v;
        else lm_out[((size_t)b * K + r) * 10 + (c - 5)] = v;
    }
}

int rconv_out(int n, int k, int stride) { return (n + 2 * (k / 2) - k) / stride + 1; }

template <int F32, int BN>
int launch_rconv(const e4s_rconv_params& p, int Ho, int Wo, int M, hipStream_t st) {
    const RconvGather g = {p.x, p.Hi, p.Wi, p.x_cstride, p.k, p.stride, Ho, Wo};
    const RconvEpi epi = {p.bias, p.r0, p.y, Ho, Wo, p.y_cstride, p.y_coff, p.r0_cstride, p.r0_H, p.r0_W, p.r0_mode, p.act, p.slope};
    hipLaunchKernelGGL((gg::gather_gemm_kernel<F32, BN, RconvGather, RconvEpi>), dim3((unsigned)((M + gg::BM - 1) / gg::BM), (unsigned)(p.Cout / BN)),
                       dim3(gg::NTHR), 0, st, g, epi, p.w, p.Cin / KC, M);
    E4S_CHECK_LAUNCH();
    return 0;
}

bool geom_ok(const e4s_retina_geom& g) {
    if (g.imH < 1 || g.imW < 1 || g.nlevel < 1 || g.nlevel > 3 || g.N < 1 || !(g.resize > 0.f)) return false;
    int base = 0;
    for (int l = 0; l < g.nlevel; ++l) {
        if (g.lh[l] < 1 || g.lw[l] < 1 || g.step[l] < 1 || g.base[l] != base) return false;
        if ((int64_t)base + (int64_t)g.lh[l] * g.lw[l] * 2 > (int64_t)g.N) return false;
        base += g.lh[l] * g.lw[l] * 2;
    }
    return base == g.N;
}

}  // namespace

extern "C" int e4s_rconv_f32(const e4s_rconv_params* pp, void* stream) {
    const e4s_rconv_params& p = *pp;
    if (!p.x || !p.w || !p.y || p.B < 1 || p.Hi < 1 || p.Wi < 1) return (int)hipErrorInvalidValue;
    if (p.Cin < KC || p.Cin % KC || p.Cout < 64 || p.Cout % 64) return (int)hipErrorInvalidValue;
    if ((p.k != 1 && p.k != 3) || (p.stride != 1 && p.stride != 2)) return (int)hipErrorInvalidValue;
    if (p.x_cstride < p.Cin || p.x_cstride % 4 || p.y_coff < 0 || p.y_coff % 4 || p.y_cstride < p.y_coff + p.Cout || p.y_cstride % 4)
        return (int)hipErrorInvalidValue;
    if ((p.act != 0 && p.act != 1) || (p.precision != 0 && p.precision != 1) || p.r0_mode < 0 || p.r0_mode > 2)
        return (int)hipErrorInvalidValue;
    if ((p.r0 != nullptr) != (p.r0_mode != 0)) return (int)hipErrorInvalidValue;
    if (!aligned16(p.x) || !aligned16(p.w) || !aligned16(p.y)) return (int)hipErrorInvalidValue;
    if (p.r0 && (!aligned16(p.r0) || p.r0_cstride < p.Cout || p.r0_cstride % 4 || p.r0_H < 0 || p.r0_W < 0 || (p.r0_H > 0) != (p.r0_W > 0)))
        return (int)hipErrorInvalidValue;
    const int Ho = rconv_out(p.Hi, p.k, p.stride), Wo = rconv_out(p.Wi, p.k, p.stride);
    if (Ho < 1 || Wo < 1) return (int)hipErrorInvalidValue;
    if ((int64_t)p.B * Ho * Wo >= (1ll << 31) - gg::BM || (int64_t)p.B * p.Hi * p.Wi >= (1ll << 31)) return (int)hipErrorInvalidValue;
    {
        const uintptr_t xa = reinterpret_cast<uintptr_t>(p.x), ya = reinterpret_cast<uintptr_t>(p.y);
        const uintptr_t xe = xa + (size_t)p.B * p.Hi * p.Wi * p.x_cstride * 4, ye = ya + (size_t)p.B * Ho * Wo * p.y_cstride * 4;
        if (xa < ye && ya < xe) return (int)hipErrorInvalidValue;               // y must not overlap x: its pixels are other blocks' input
    }
    const int M = p.B * Ho * Wo;
    if (p.Cout / 64 > 65535) return (int)hipErrorInvalidValue;
    hipStream_t st = as_stream(stream);
    if (p.Cout % 128 == 0) return p.precision == 1 ? launch_rconv<1, 128>(p, Ho, Wo, M, st) : launch_rconv<0, 128>(p, Ho, Wo, M, st);
    return p.precision == 1 ? launch_rconv<1, 64>(p, Ho, Wo, M, st) : launch_rconv<0, 64>(p, Ho, Wo, M, st);
}

extern "C" int64_t e4s_rconv_pack_bytes(int Cin, int Cout, int k) {
    return Cin >= KC && Cin % KC == 0 && Cout >= 64 && Cout % 64 == 0 && (k == 1 || k == 3) ? (int64_t)Cout * Cin * k * k * 4 : 0;
}

extern "C" int e4s_rconv_pack_f32(const float* w, void* out, int Cin, int Cout, int k, int split, void* stream) {
    if (!w || !out || !aligned16(out) || e4s_rconv_pack_bytes(Cin, Cout, k) == 0) return (int)hipErrorInvalidValue;
    gg::gather_gemm_pack<64>(w, out, Cin, Cout, k * k, (int64_t)Cout * Cin * k * k, split, as_stream(stream));
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_retina_prep_f32(const uint8_t* src, float* dst, int B, int H, int W, int Hd, int Wd, double scale, void* stream) {
    if (!src || !dst || B < 1 || H < 1 || W < 1 || Hd < 1 || Wd < 1) return (int)hipErrorInvalidValue;
    const int shrink = !(Hd == H && Wd == W);
    if (shrink && !(scale > 0.0)) return (int)hipErrorInvalidValue;
    const int64_t n = (int64_t)B * Hd * Wd;
    if ((n + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), src, dst, H, W, Hd, Wd, shrink, scale, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_retina_head_f32(const float* x, int x_cstride, const float* wp, const float* bias, const e4s_retina_geom* g, int level,
                                   int B, float* boxes, float* scores, float* landms, float* raw_loc, float* raw_conf, float* raw_lm,
                                   void* stream) {
    if (!x || !wp || !bias || !g || !boxes || !scores || !landms || B < 1 || !geom_ok(*g) || level < 0 || level >= g->nlevel)
        return (int)hipErrorInvalidValue;
    if (x_cstride < HC || x_cstride % 4 || !aligned16(x) || !aligned16(boxes)) return (int)hipErrorInvalidValue;
    if ((raw_loc != nullptr) != (raw_conf != nullptr) || (raw_loc != nullptr) != (raw_lm != nullptr)) return (int)hipErrorInvalidValue;
    const int64_t ncell = (int64_t)B * g->lh[level] * g->lw[level];
    if ((ncell + HCELLS - 1) / HCELLS >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(head_kernel, dim3((unsigned)((ncell + HCELLS - 1) / HCELLS)), dim3(256), 0, as_stream(stream), x, x_cstride, wp, bias,
                       *g, level, ncell, boxes, scores, landms, raw_loc, raw_conf, raw_lm);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_retina_decode_f32(const float* loc, const float* conf, const float* lm, const e4s_retina_geom* g, int B, float* boxes,
                                     float* scores, float* landms, void* stream) {
    if (!loc || !conf || !lm || !g || !boxes || !scores || !landms || B < 1 || !geom_ok(*g) || !aligned16(boxes)) return (int)hipErrorInvalidValue;
    const int64_t total = (int64_t)B * g->N;
    if ((total + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), loc, conf, lm, *g, total, boxes,
                       scores, landms);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_retina_select_f32(const float* boxes, const float* landms, const float* sorted_scores, const int64_t* sorted_idx, int B,
                                     int N, float conf_thr, float nms_thr, int top_k, int keep_top_k, float ss, float* dets, float* lm_out,
                                     int* counts, void* stream) {
    if (!boxes || !landms || !sorted_scores || !sorted_idx || !dets || !lm_out || !counts) return (int)hipErrorInvalidValue;
    if (B < 1 || N < 1 || top_k < 1 || keep_top_k < 1 || !(ss > 0.f) || !aligned16(boxes)) return (int)hipErrorInvalidValue;
    const int64_t smem = (int64_t)keep_top_k * 4 + (top_k < N ? top_k : N);
    if (smem > 60 * 1024) return (int)hipErrorInvalidValue;     // the candidate flags and the kept list live in LDS
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)B), dim3(256), (size_t)smem, as_stream(stream), boxes, landms, sorted_scores, sorted_idx,
                       N, conf_thr, nms_thr, top_k, keep_top_k, ss, dets, lm_out, counts);
    E4S_CHECK_LAUNCH();
    return 0;
}
