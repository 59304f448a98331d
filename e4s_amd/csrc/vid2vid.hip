// face-vid2vid's pose front end (e4s_amd/reenact.py; src/pretrained/face_vid2vid/): the 3-D conv of the keypoint detector's
// up-sampling blocks and heads, the soft-argmax head, the anti-alias down-sampling, the 2x2 average pool and the pose kernel.
//
// 3-D conv (e4s_conv3d_f32): zero-padded 3x3x3, stride 1, channels-last fp32, Cin a multiple of 32, ANY Cout, D, H and W.  It is a
// private copy of the tile of gather_gemm.h (e4s_rconv_f32's), not a user of halo_conv3x3.h: the shipped volumes start
// at 16 x 4 x 4 and 16 x 8 x 8, where a 16 x 16 halo tile is mostly overhang, and the reshaped input is not plane-contiguous (it
// arrives through strides).  An implicit GEMM over the
// flattened output voxels M = B D Ho Wo: a block computes 128 voxels x BN output channels, BN = 128 / 64 / 32 by the padded Cout
// (the packer pads Cout to a multiple of 32 with zero rows; padded channels are computed and never stored).  Four waves of 32 x 32
// MFMA tiles, as 2 x 2 (BN >= 64) or 4 x 1 (BN = 32).  K runs over (tap = (kd, ky, kx), 32-channel chunk): per step the 128 gathered
// voxel rows (zero where the tap leaves the volume or the row is past M) and the BN weight rows are staged in LDS as 128-byte rows with
// the 16-byte granule XOR-swizzled (mfma_rows.h), while the next step's global loads are in flight in registers.
//   up2       the grid the conv runs on is the nearest (1, 2, 2) up-sampling of x: grid position (d, gy, gx) reads source (d, gy >> 1,
//             gx >> 1); the padding applies on the grid; the up-sampled volume is never written
//   x         addressed through element strides (batch, depth, row, column), channels contiguous: a contiguous NDHWC volume, or the
//             NHWC output [B,h,w,depth * C] of the 1x1 conv in front read as [B,depth,h,w,C] (strides h w depth C, C, w depth C, depth C)
//   epilogue  v = acc + bias[c] (eval BatchNorm3d folded on the host), ReLU with relu
// Arithmetic: split-bf16 (rows hold [32 hi | 32 lo] bf16; three v_mfma_f32_32x32x16_bf16 per product, lo x hi first, then hi x lo,
// then hi x hi, fp32 accumulate) or exact fp32 (v_mfma_f32_32x32x2_f32) from the same tile code.  The summation order of an output is
// (tap kd-major then ky then kx, 32-channel chunk, k-step) whatever the batch, the voxel's position or the tile's place: a tap that
// leaves the volume contributes exact zeros in its turn.
//
// The family (e4s_conv3dx_f32, ABI v23; the dense motion network and the ResBlock3d stack of reenact_warp.py) is the same tile code
// with the kernel's edge KS = 1, 3 or 7 as a template parameter (KS = 3 is the kernel above, instruction for instruction) and a
// residual read through its own strides in the epilogue (v = acc + bias + res, then the ReLU).  Channel-slice outputs are y advanced
// to the slice with the buffer's y_cstride; Cin 80 and 112 are a padded channel stride whose pad channels hold zeros, with zero
// weight columns; x_bstride = 0 broadcasts a batch-1 input.  KS = 7 (Cin 112 -> 16 on a 16-deep volume): a tile skips the kd planes
// that leave the volume for all of its voxels; their steps would add exact zeros to accumulators that are never -0, so the order of
// the in-range steps, and every bit, stays (test_new_convs_batch_and_position_do_not_change_the_bits).  Cout = 16 runs the BN = 32
// tile with half of its columns idle.
//
// Soft-argmax head: one block per (sample, keypoint).  m = max logit / T; every thread adds exp(logit / T - m) times (1, x, y, z, the
// nine jacobian maps) over voxels tid, tid + 256, ... in rising order, then a fixed binary tree over the 256 partials; value = sums /
// sum.  The order depends on (D, H, W) only.
// Pose: one block per frame.  Global average pool (per channel, pixels in rising order), the five linear heads (per output a lane-
// strided dot and wave_sum), the three 66-bin softmax expectations, the rotation matrix and the keypoint transformation.
#include "gather_gemm.h"                                        // the weight packer (gg::gather_gemm_pack)

#pragma clang fp contract(off)

namespace {

constexpr int BM = 128, NTHR = 256, YLD = 36;
constexpr int A_BYTES = BM * ROWB;                                              // 16 384

// F32: 1 = exact fp32 MFMA, 0 = split-bf16; BN: output channels per block (32, 64 or 128); UP2: the (1, 2, 2) nearest up-sampling
// KS: the kernel's edge (1, 3 or 7; padding KS / 2)
template <int F32, int BN, int UP2, int KS>
__global__ __launch_bounds__(NTHR) void conv3d_kernel(const e4s_conv3dx_params p, const int Ho, const int Wo, const int M) {
    constexpr int PAD = KS / 2, NTAP = KS * KS * KS;
    constexpr int WN = BN >= 64 ? 2 : 1, WM = 4 / WN;           // waves along the channels / the voxels
    constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);     // 32 x 32 tiles per wave
    constexpr int BPIECES = BN * 8;                             // 16-byte weight pieces per step
    constexpr int BJ = BPIECES / NTHR;
    static_assert(BPIECES % NTHR == 0, "thread layout");
    constexpr int B_BYTES = BN * ROWB;
    static_assert(4 * 32 * YLD * 4 <= A_BYTES + B_BYTES, "the output staging tiles alias the operand buffers");
    __shared__ __attribute__((aligned(16))) unsigned char smem[A_BYTES + B_BYTES];
    __shared__ int s_out[BM];
    unsigned char* sA = smem;                                   // [128 voxels][ROWB]
    unsigned char* sB = smem + A_BYTES;                         // [BN channels][ROWB]
    float* sY = reinterpret_cast<float*>(smem);                 // [4 waves][32][YLD] output staging (aliases the operands)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int wm = wave % WM, wn = wave / WM;
    const int m0 = blockIdx.x * BM;
    const int nchunk = p.Cin / KC;
    const int nstep = NTAP * nchunk;
    const int Hg = UP2 ? 2 * p.Hi : p.Hi, Wg = UP2 ? 2 * p.Wi : p.Wi;          // the grid the padding applies on (= Ho x Wo)

    // this thread's two gathered items: (voxel row m, 8-channel group q)
    int a_d[2], a_y[2], a_x[2];
    int64_t a_base[2];
    bool a_live[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int item = tid + NTHR * j;
        const int m = m0 + (item >> 2);
        a_live[j] = m < M;
        const int mm = a_live[j] ? m : 0;
        const int ox = mm % Wo;
        int t = mm / Wo;
        a_x[j] = ox - PAD;
        a_y[j] = t % Ho - PAD;
        t /= Ho;
        a_d[j] = t % p.D - PAD;
        a_base[j] = (int64_t)(t / p.D) * p.x_bstride + (item & 3) * 8;
    }
    const f32x8 zero8 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x8 ra[2];
    f32x4 rb[BJ];
    const unsigned char* wbase = reinterpret_cast<const unsigned char*>(p.w);
    auto fetch = [&](int step) {
        const int tap = step / nchunk, chunk = step - tap * nchunk;
        const int kd = tap / (KS * KS), ky = (tap - kd * (KS * KS)) / KS, kx = tap % KS;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int id = a_d[j] + kd, gy = a_y[j] + ky, gx = a_x[j] + kx;
            const bool ok = a_live[j] && (unsigned)id < (unsigned)p.D && (unsigned)gy < (unsigned)Hg && (unsigned)gx < (unsigned)Wg;
            const int iy = UP2 ? gy >> 1 : gy, ix = UP2 ? gx >> 1 : gx;
            const int64_t off = a_base[j] + (int64_t)id * p.x_dstride + (int64_t)iy * p.x_ystride + (int64_t)ix * p.x_xstride + chunk * KC;
            ra[j] = ok ? load8(p.x + off) : zero8;
        }
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
            const int i = tid + NTHR * j;
            const int row = i >> 3;
            const int cb32 = blockIdx.y * (BN / 32) + (row >> 5);
            const unsigned char* wb = wbase + (((size_t)cb32 * NTAP + tap) * nchunk + chunk) * (32 * ROWB) + (size_t)(row & 31) * ROWB + (i & 7) * 16;
            rb[j] = *reinterpret_cast<const f32x4*>(wb);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int item = tid + NTHR * j;
            const int m = item >> 2, q = item & 3;
            if (F32) {
                *reinterpret_cast<f32x4*>(sA + swz(m, 2 * q)) = f32x4{ra[j][0], ra[j][1], ra[j][2], ra[j][3]};
                *reinterpret_cast<f32x4*>(sA + swz(m, 2 * q + 1)) = f32x4{ra[j][4], ra[j][5], ra[j][6], ra[j][7]};
            } else {
                split_store(sA, swz(m, q), ra[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
            const int i = tid + NTHR * j;
            *reinterpret_cast<f32x4*>(sB + swz(i >> 3, i & 7)) = rb[j];
        }
    };

    if (tid < BM) s_out[tid] = m0 + tid < M ? m0 + tid : -1;
    int aro[TM], bro[TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) aro[tm] = swz(wm * (32 * TM) + tm * 32 + li, kh);
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) bro[tn] = swz(wn * (32 * TN) + tn * 32 + li, kh);

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    // KS = 7: the kd planes that leave the volume for EVERY voxel of the tile are skipped.  Each of their steps would add exact zeros to
    // accumulators that are never -0, so the in-range steps, still in rising order, give the same bits.
    int step_lo = 0, step_hi = nstep;
    if (KS == 7) {
        const int per = Ho * Wo;
        const int v0 = m0 / per, v1 = (m0 + BM - 1 < M ? m0 + BM - 1 : M - 1) / per;
        const bool one = v0 / p.D == v1 / p.D;                 // the tile lies in one sample
        const int dlo = one ? v0 % p.D : 0, dhi = one ? v1 % p.D : p.D - 1;
        const int kd_lo = PAD - dhi > 0 ? PAD - dhi : 0, kd_hi = p.D - 1 + PAD - dlo < KS - 1 ? p.D - 1 + PAD - dlo : KS - 1;
        step_lo = kd_lo * KS * KS * nchunk;
        step_hi = (kd_hi + 1) * KS * KS * nchunk;
    }
    fetch(step_lo);
    for (int step = step_lo; step < step_hi; ++step) {
        __syncthreads();                                        // every reader of the previous step's LDS image is done
        stage();
        if (step + 1 < step_hi) fetch(step + 1);
        __syncthreads();
        if (F32) {
            // lane (li, kh) holds channels 4 (2 gp + kh) + s of its row, for A and B alike
#pragma unroll
            for (int gp = 0; gp < 4; ++gp) {
                f32x4 a4[TM], b4[TN];
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) a4[tm] = *reinterpret_cast<const f32x4*>(sA + (aro[tm] ^ (gp * 32)));
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) b4[tn] = *reinterpret_cast<const f32x4*>(sB + (bro[tn] ^ (gp * 32)));
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                        for (int tn = 0; tn < TN; ++tn)
                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tm][s], b4[tn][s], acc[tm][tn], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    ah[tm] = *reinterpret_cast<const bf16x8*>(sA + (aro[tm] ^ (kk * 32)));
                    al[tm] = *reinterpret_cast<const bf16x8*>(sA + (aro[tm] ^ (kk * 32) ^ LO));
                }
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    bh[tn] = *reinterpret_cast<const bf16x8*>(sB + (bro[tn] ^ (kk * 32)));
                    bl[tn] = *reinterpret_cast<const bf16x8*>(sB + (bro[tn] ^ (kk * 32) ^ LO));
                }
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) {
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[tm], bh[tn], acc[tm][tn], 0, 0, 0);
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[tm], bl[tn], acc[tm][tn], 0, 0, 0);
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[tm], bh[tn], acc[tm][tn], 0, 0, 0);
                    }
            }
        }
    }

    // ---- epilogue: one 32 x 32 tile per wave and pass through the LDS staging tile; 16-byte stores where the output's channel count
    // and stride allow them, else one guarded 4-byte store per live channel (the 15- and 135-channel heads) ----
    const bool vec = (p.Cout & 3) == 0 && (p.y_cstride & 3) == 0;
    float* myY = sY + wave * 32 * YLD;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int co = blockIdx.y * BN + wn * (32 * TN) + tn * 32;
            const float bsv = (p.bias && co + li < p.Cout) ? p.bias[co + li] : 0.f;
            __syncthreads();                                    // the operands (or the previous pass's tile) are read
#pragma unroll
            for (int r = 0; r < 16; ++r) myY[((r & 3) + 8 * (r >> 2) + 4 * kh) * YLD + li] = acc[tm][tn][r] + bsv;
            __syncthreads();
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) {
                const int row = ps * 8 + (lane >> 3), c4 = lane & 7;
                const int pix = s_out[wm * (32 * TM) + tm * 32 + row];
                const int c = co + c4 * 4;
                if (pix < 0 || c >= p.Cout) continue;
                f32x4 v = *reinterpret_cast<const f32x4*>(myY + row * YLD + c4 * 4);
                if (p.res) {
                    const int ox = pix % Wo;
                    int t = pix / Wo;
                    const int oy = t % Ho;
                    t /= Ho;
                    const float* rs = p.res + (int64_t)(t / p.D) * p.r_bstride + (int64_t)(t % p.D) * p.r_dstride + (int64_t)oy * p.r_ystride +
                                      (int64_t)ox * p.r_xstride + c;
                    if (vec) {
                        v += *reinterpret_cast<const f32x4*>(rs);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (c + e < p.Cout) v[e] += rs[e];
                    }
                }
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
                }
                float* dst = p.y + (size_t)pix * p.y_cstride + c;
                if (vec) {
                    *reinterpret_cast<f32x4*>(dst) = v;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < p.Cout) dst[e] = v[e];
                }
            }
        }
}

template <int F32, int BN>
int launch_conv3d(const e4s_conv3dx_params& p, int Ho, int Wo, int M, int cout_pad, hipStream_t st) {
    const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)(cout_pad / BN));
    if (p.ksize == 7) hipLaunchKernelGGL((conv3d_kernel<F32, BN, 0, 7>), grid, dim3(NTHR), 0, st, p, Ho, Wo, M);
    else if (p.ksize == 1) hipLaunchKernelGGL((conv3d_kernel<F32, BN, 0, 1>), grid, dim3(NTHR), 0, st, p, Ho, Wo, M);
    else if (p.up2) hipLaunchKernelGGL((conv3d_kernel<F32, BN, 1, 3>), grid, dim3(NTHR), 0, st, p, Ho, Wo, M);
    else hipLaunchKernelGGL((conv3d_kernel<F32, BN, 0, 3>), grid, dim3(NTHR), 0, st, p, Ho, Wo, M);
    E4S_CHECK_LAUNCH();
    return 0;
}

// ---- soft-argmax head ----
constexpr int SA_N = 13;                                        // sum, x, y, z and nine jacobian entries

__global__ __launch_bounds__(256) void softargmax_kernel(const float* __restrict__ logits, int64_t l_bstride, int64_t l_kstride,
                                                         int64_t l_vstride, const float* __restrict__ jac, int64_t j_bstride,
                                                         int64_t j_cstride, int64_t j_vstride, int njmaps, int K, int D, int H, int W,
                                                         float temperature, float* __restrict__ value, float* __restrict__ jacobian) {
    __shared__ float s_red[256];
    __shared__ float s_sum[SA_N][256];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / K, k = blockIdx.x % K;
    const int V = D * H * W;
    const float* lg = logits + (int64_t)b * l_bstride + (int64_t)k * l_kstride;
    const float* jm = jac ? jac + (int64_t)b * j_bstride + (int64_t)(njmaps == 1 ? 0 : k) * 9 * j_cstride : nullptr;

    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256) mx = fmaxf(mx, lg[(int64_t)v * l_vstride] / temperature);
    s_red[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] = fmaxf(s_red[tid], s_red[tid + o]);
        __syncthreads();
    }
    mx = s_red[0];

    float part[SA_N];
#pragma unroll
    for (int e = 0; e < SA_N; ++e) part[e] = 0.f;
    for (int v = tid; v < V; v += 256) {
        const float ev = expf(lg[(int64_t)v * l_vstride] / temperature - mx);
        const int x = v % W, t = v / W;
        const int y = t % H, z = t / H;
        part[0] += ev;
        part[1] += ev * grid_coord(x, W);
        part[2] += ev * grid_coord(y, H);
        part[3] += ev * grid_coord(z, D);
        if (jm) {
#pragma unroll
            for (int e = 0; e < 9; ++e) part[4 + e] += ev * jm[(int64_t)e * j_cstride + (int64_t)v * j_vstride];
        }
    }
#pragma unroll
    for (int e = 0; e < SA_N; ++e) s_sum[e][tid] = part[e];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int e = 0; e < SA_N; ++e) s_sum[e][tid] += s_sum[e][tid + o];
        }
        __syncthreads();
    }
    const float total = s_sum[0][0];
    if (tid < 3) value[((int64_t)b * K + k) * 3 + tid] = s_sum[1 + tid][0] / total;
    if (jacobian && tid < 9) jacobian[((int64_t)b * K + k) * 9 + tid] = s_sum[4 + tid][0] / total;
}

// ---- anti-alias down-sampling: out(oy, ox) = sum_ky t[ky] sum_kx t[kx] in(oy step + ky - ka, ox step + kx - ka), zero outside ----
__global__ __launch_bounds__(256) void aa_down_kernel(const void* __restrict__ src, int is_u8, float* __restrict__ dst, int H, int W, int Ho,
                                                      int Wo, const float* __restrict__ taps, int ntaps, int step, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % 3);
    int64_t t = i / 3;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const int64_t b = t / Ho;
    const int ka = ntaps / 2;
    const uint8_t* s8 = static_cast<const uint8_t*>(src) + b * H * W * 3;
    const float* sf = static_cast<const float*>(src) + b * H * W * 3;
    float acc = 0.f;
    for (int ky = 0; ky < ntaps; ++ky) {
        const int iy = oy * step + ky - ka;
        if ((unsigned)iy >= (unsigned)H) continue;
        float row = 0.f;
        for (int kx = 0; kx < ntaps; ++kx) {
            const int ix = ox * step + kx - ka;
            if ((unsigned)ix >= (unsigned)W) continue;
            const int64_t o = ((int64_t)iy * W + ix) * 3 + c;
            const float v = is_u8 ? (float)s8[o] / 255.f : sf[o];
            row += taps[kx] * v;
        }
        acc += taps[ky] * row;
    }
    dst[i] = acc;
}

// ---- nn.AvgPool2d(2) on NHWC: Ho = Hi / 2, Wo = Wi / 2 (odd sizes drop their last row / column) ----
__global__ __launch_bounds__(256) void avgpool2_kernel(const float* __restrict__ x, float* __restrict__ y, int Hi, int Wi, int Ho, int Wo,
                                                       int C4, int XS4, int YS4, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C4);
    int64_t t = i / C4;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const int64_t b = t / Ho;
    const f32x4* src = reinterpret_cast<const f32x4*>(x) + ((b * Hi + 2 * oy) * Wi + 2 * ox) * XS4 + c;
    const f32x4 s = ((src[0] + src[XS4]) + src[(int64_t)Wi * XS4]) + src[(int64_t)Wi * XS4 + XS4];
    reinterpret_cast<f32x4*>(y)[((b * Ho + oy) * Wo + ox) * YS4 + c] = s * 0.25f;
}

// ---- pose ----
constexpr int POSE_MAXC = 2048, POSE_MAXO = 512;

// headpose_pred_to_degree of one row of nbins logits in LDS: softmax, sum p idx, * 3 - 99 (one thread)
__device__ float bins_to_degree(const float* z, int nbins) {
    float m = z[0];
    for (int i = 1; i < nbins; ++i) m = fmaxf(m, z[i]);
    float s = 0.f;
    for (int i = 0; i < nbins; ++i) s += expf(z[i] - m);
    float d = 0.f;
    for (int i = 0; i < nbins; ++i) d += expf(z[i] - m) / s * (float)i;
    return d * 3.f - 99.f;
}

__global__ __launch_bounds__(256) void pose_kernel(const e4s_pose_params p) {
    __shared__ float s_f[POSE_MAXC];
    __shared__ float s_o[POSE_MAXO];
    __shared__ float s_rot[9];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int nout = 3 * p.nbins + 3 + 3 * p.K;
    const float* x = p.x + (int64_t)b * p.HW * p.x_cstride;
    const float inv = 1.f / (float)p.HW;
    for (int c = tid; c < p.C; c += 256) {
        float s = 0.f;
        for (int i = 0; i < p.HW; ++i) s += x[(int64_t)i * p.x_cstride + c];
        s_f[c] = s * inv;
    }
    __syncthreads();
    for (int o = wave; o < nout; o += 4) {
        const float* w = p.w + (int64_t)o * p.C;
        float s = 0.f;
        for (int c = lane; c < p.C; c += 64) s += w[c] * s_f[c];
        s = wave_sum(s);
        if (lane == 0) s_o[o] = s + p.bias[o];
    }
    __syncthreads();
    // rows of s_o: yaw (fc_roll), pitch (fc_pitch), roll (fc_yaw), t, exp
    for (int o = tid; o < nout; o += 256) p.raw[(int64_t)b * nout + o] = s_o[o];
    if (tid < 3) {
        const float fixed = tid == 0 ? p.yaw : (tid == 1 ? p.pitch : p.roll);
        const float deg = bins_to_degree(s_o + tid * p.nbins, p.nbins);
        p.degrees[b * 3 + tid] = deg;
        s_f[tid] = ((p.fixed_mask >> tid) & 1) ? fixed : deg;   // s_f is free again: the heads are done
    }
    __syncthreads();
    if (tid == 0) {
        // get_rotation_matrix: angle / 180 * 3.14 (the reference's pi), pitch about x, yaw about y, roll about z; R = Rp Ry Rr
        const float yaw = s_f[0] / 180.f * 3.14f, pitch = s_f[1] / 180.f * 3.14f, roll = s_f[2] / 180.f * 3.14f;
        const float cp = cosf(pitch), sp = sinf(pitch), cy = cosf(yaw), sy = sinf(yaw), cr = cosf(roll), sr = sinf(roll);
        const float P[9] = {1.f, 0.f, 0.f, 0.f, cp, -sp, 0.f, sp, cp};
        const float Y[9] = {cy, 0.f, sy, 0.f, 1.f, 0.f, -sy, 0.f, cy};
        const float R[9] = {cr, -sr, 0.f, sr, cr, 0.f, 0.f, 0.f, 1.f};
        float PY[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                float s = 0.f;
                for (int k = 0; k < 3; ++k) s += P[i * 3 + k] * Y[k * 3 + j];
                PY[i * 3 + j] = s;
            }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                float s = 0.f;
                for (int k = 0; k < 3; ++k) s += PY[i * 3 + k] * R[k * 3 + j];
                s_rot[i * 3 + j] = s;
                p.rot[b * 9 + i * 3 + j] = s;
            }
    }
    __syncthreads();
    if (!p.kp_value) return;
    const float* kp = p.kp_value + (int64_t)(p.kp_batch == 1 ? 0 : b) * p.K * 3;
    const float* tt = s_o + 3 * p.nbins;
    const float* ex = tt + 3;
    for (int i = tid; i < p.K * 3; i += 256) {
        const int k = i / 3, m = i % 3;
        float s = 0.f;
        for (int q = 0; q < 3; ++q) s += s_rot[m * 3 + q] * kp[k * 3 + q];
        p.value[((int64_t)b * p.K + k) * 3 + m] = s + tt[m] + ex[k * 3 + m];
    }
    if (p.kp_jacobian && p.jacobian) {
        const float* kj = p.kp_jacobian + (int64_t)(p.kp_batch == 1 ? 0 : b) * p.K * 9;
        for (int i = tid; i < p.K * 9; i += 256) {
            const int k = i / 9, m = (i % 9) / 3, s3 = i % 3;
            float s = 0.f;
            for (int q = 0; q < 3; ++q) s += s_rot[m * 3 + q] * kj[k * 9 + q * 3 + s3];
            p.jacobian[(int64_t)b * p.K * 9 + i] = s;
        }
    }
}

}  // namespace

static bool conv3d_ksize_ok(int k) { return k == 1 || k == 3 || k == 7; }

extern "C" int64_t e4s_conv3dx_pack_bytes(int Cin, int Cout, int ksize) {
    return conv3d_ksize_ok(ksize) && Cin >= KC && Cin % KC == 0 && Cout >= 1
               ? (int64_t)((Cout + 31) / 32) * (ksize * ksize * ksize) * (Cin / KC) * 32 * ROWB
               : 0;
}

extern "C" int64_t e4s_conv3d_pack_bytes(int Cin, int Cout) { return e4s_conv3dx_pack_bytes(Cin, Cout, 3); }

extern "C" int e4s_conv3dx_pack_f32(const float* w, void* out, int Cin, int Cout, int ksize, int split, void* stream) {
    const int64_t bytes = e4s_conv3dx_pack_bytes(Cin, Cout, ksize);
    if (!w || !out || !aligned16(out) || bytes == 0) return (int)hipErrorInvalidValue;
    const int64_t n = bytes / ROWB * 32;
    if ((n + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    gg::gather_gemm_pack<32>(w, out, Cin, Cout, ksize * ksize * ksize, n, split, as_stream(stream));    // nn.Conv3d's [Cout][Cin][ntap], row blocks of 32
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_conv3d_pack_f32(const float* w, void* out, int Cin, int Cout, int split, void* stream) {
    return e4s_conv3dx_pack_f32(w, out, Cin, Cout, 3, split, stream);
}

extern "C" int e4s_conv3dx_f32(const e4s_conv3dx_params* pp, void* stream) {
    const e4s_conv3dx_params& p = *pp;
    if (!p.x || !p.w || !p.y || p.B < 1 || p.D < 1 || p.Hi < 1 || p.Wi < 1) return (int)hipErrorInvalidValue;
    if (p.Cin < KC || p.Cin % KC || p.Cout < 1 || p.y_cstride < p.Cout) return (int)hipErrorInvalidValue;
    if ((p.up2 != 0 && p.up2 != 1) || (p.relu != 0 && p.relu != 1) || (p.precision != 0 && p.precision != 1)) return (int)hipErrorInvalidValue;
    if (!conv3d_ksize_ok(p.ksize) || (p.up2 && p.ksize != 3)) return (int)hipErrorInvalidValue;
    if (p.x_bstride < 0 || p.x_dstride < 0 || p.x_ystride < 0 || p.x_xstride < p.Cin) return (int)hipErrorInvalidValue;
    if (p.x_bstride % 4 || p.x_dstride % 4 || p.x_ystride % 4 || p.x_xstride % 4) return (int)hipErrorInvalidValue;
    if (!aligned16(p.x) || !aligned16(p.w) || !aligned16(p.y)) return (int)hipErrorInvalidValue;
    if (p.res) {
        if (p.r_bstride < 0 || p.r_dstride < 0 || p.r_ystride < 0 || p.r_xstride < p.Cout) return (int)hipErrorInvalidValue;
        if (p.r_bstride % 4 || p.r_dstride % 4 || p.r_ystride % 4 || p.r_xstride % 4 || !aligned16(p.res)) return (int)hipErrorInvalidValue;
    }
    const int Ho = p.up2 ? 2 * p.Hi : p.Hi, Wo = p.up2 ? 2 * p.Wi : p.Wi;
    const int64_t M = (int64_t)p.B * p.D * Ho * Wo;
    if (M >= (1ll << 31) - BM) return (int)hipErrorInvalidValue;
    const int cout_pad = (p.Cout + 31) / 32 * 32;
    if (cout_pad / 32 > 65535) return (int)hipErrorInvalidValue;
    hipStream_t st = as_stream(stream);
    if (cout_pad % 128 == 0)
        return p.precision == 1 ? launch_conv3d<1, 128>(p, Ho, Wo, (int)M, cout_pad, st) : launch_conv3d<0, 128>(p, Ho, Wo, (int)M, cout_pad, st);
    if (cout_pad % 64 == 0)
        return p.precision == 1 ? launch_conv3d<1, 64>(p, Ho, Wo, (int)M, cout_pad, st) : launch_conv3d<0, 64>(p, Ho, Wo, (int)M, cout_pad, st);
    return p.precision == 1 ? launch_conv3d<1, 32>(p, Ho, Wo, (int)M, cout_pad, st) : launch_conv3d<0, 32>(p, Ho, Wo, (int)M, cout_pad, st);
}

extern "C" int e4s_conv3d_f32(const e4s_conv3d_params* pp, void* stream) {
    if (!pp) return (int)hipErrorInvalidValue;
    e4s_conv3dx_params q = {};
    q.x = pp->x, q.w = pp->w, q.bias = pp->bias, q.y = pp->y;
    q.x_bstride = pp->x_bstride, q.x_dstride = pp->x_dstride, q.x_ystride = pp->x_ystride, q.x_xstride = pp->x_xstride;
    q.B = pp->B, q.D = pp->D, q.Hi = pp->Hi, q.Wi = pp->Wi, q.Cin = pp->Cin, q.Cout = pp->Cout;
    q.y_cstride = pp->y_cstride, q.ksize = 3, q.up2 = pp->up2, q.relu = pp->relu, q.precision = pp->precision;
    return e4s_conv3dx_f32(&q, stream);
}

extern "C" int e4s_softargmax3d_f32(const float* logits, int64_t l_bstride, int64_t l_kstride, int64_t l_vstride, const float* jac,
                                    int64_t j_bstride, int64_t j_cstride, int64_t j_vstride, int njmaps, int B, int K, int D, int H, int W,
                                    float temperature, float* value, float* jacobian, void* stream) {
    if (!logits || !value || B < 1 || K < 1 || D < 1 || H < 1 || W < 1 || !(temperature > 0.f)) return (int)hipErrorInvalidValue;
    if ((jac != nullptr) != (jacobian != nullptr) || (jac && njmaps != 1 && njmaps != K)) return (int)hipErrorInvalidValue;
    if ((int64_t)D * H * W >= (1ll << 31) || (int64_t)B * K >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(softargmax_kernel, dim3((unsigned)(B * K)), dim3(256), 0, as_stream(stream), logits, l_bstride, l_kstride, l_vstride,
                       jac, j_bstride, j_cstride, j_vstride, njmaps, K, D, H, W, temperature, value, jacobian);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_aa_down_f32(const void* src, int is_u8, float* dst, int B, int H, int W, const float* taps, int ntaps, int step,
                               void* stream) {
    if (!src || !dst || !taps || B < 1 || H < 1 || W < 1 || ntaps < 1 || !(ntaps & 1) || step < 1) return (int)hipErrorInvalidValue;
    const int Ho = (H + step - 1) / step, Wo = (W + step - 1) / step;
    const int64_t n = (int64_t)B * Ho * Wo * 3;
    if ((n + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(aa_down_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), src, is_u8, dst, H, W, Ho, Wo, taps,
                       ntaps, step, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_avgpool2s_f32(const float* x, float* y, int B, int Hi, int Wi, int C, int x_cstride, int y_cstride, void* stream) {
    if (!x || !y || B < 1 || Hi < 2 || Wi < 2 || C < 4 || C % 4 || !aligned16(x) || !aligned16(y)) return (int)hipErrorInvalidValue;
    if (x_cstride < C || y_cstride < C || x_cstride % 4 || y_cstride % 4) return (int)hipErrorInvalidValue;
    const int Ho = Hi / 2, Wo = Wi / 2;
    const int64_t n = (int64_t)B * Ho * Wo * (C / 4);
    if ((n + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(avgpool2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, y, Hi, Wi, Ho, Wo, C / 4,
                       x_cstride / 4, y_cstride / 4, n);
    E4S_CHECK_LAUNCH();
    return 0;
}

extern "C" int e4s_avgpool2_f32(const float* x, float* y, int B, int Hi, int Wi, int C, void* stream) {
    return e4s_avgpool2s_f32(x, y, B, Hi, Wi, C, C, C, stream);
}

extern "C" int e4s_pose_f32(const e4s_pose_params* pp, void* stream) {
    const e4s_pose_params& p = *pp;
    if (!p.x || !p.w || !p.bias || !p.raw || !p.degrees || !p.rot || p.B < 1 || p.HW < 1) return (int)hipErrorInvalidValue;
    if (p.C < 1 || p.C > POSE_MAXC || p.x_cstride < p.C || p.nbins < 1 || p.K < 1 || 3 * p.nbins + 3 + 3 * p.K > POSE_MAXO)
        return (int)hipErrorInvalidValue;
    if (p.fixed_mask < 0 || p.fixed_mask > 7) return (int)hipErrorInvalidValue;
    if (p.kp_value && (!p.value || (p.kp_batch != 1 && p.kp_batch != p.B))) return (int)hipErrorInvalidValue;
    if (p.kp_jacobian && !p.kp_value) return (int)hipErrorInvalidValue;
    if ((p.kp_jacobian != nullptr) != (p.jacobian != nullptr)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pose_kernel, dim3((unsigned)p.B), dim3(256), 0, as_stream(stream), p);
    E4S_CHECK_LAUNCH();
    return 0;
}
