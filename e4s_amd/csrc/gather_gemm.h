// The gather-GEMM conv tile (namespace gg): RetinaFace's zero-padded 2-D conv family (retinaface.hip) runs on it.  face-vid2vid's 3-D conv
// family (vid2vid.hip) shares the weight packer only and keeps a private copy of the tile (DESIGN 3.19 says why), so what only that
// family needs -- a BN = 32 wave grid, row blocks of 32, a per-tile step range -- is not here.
// An implicit GEMM over M flattened output positions (rows): a block computes 128 rows x BN output channels, four waves of 32 x 32 MFMA
// tiles as 2 x 2.  K runs over (tap, 32-channel chunk): per step the 128 gathered source rows (zero where Gather says the tap is not
// live) and the BN weight rows (pre-packed by gather_gemm_pack_kernel<SPLIT, 64>) are staged in LDS as 128-byte rows with the 16-byte
// granule XOR-swizzled (mfma_rows.h), while the next step's global loads are in flight in registers.  Arithmetic: split-bf16 (rows hold
// [32 hi | 32 lo] bf16; three v_mfma_f32_32x32x16_bf16 per product, lo x hi first, then hi x lo, then hi x hi, fp32 accumulate) or exact
// fp32 (v_mfma_f32_32x32x2_f32) from the same tile code.  The summation order of an output is (tap, chunk, k-step) whatever the batch
// or the tile's place (tests/test_gpu_gather_conv_bits.py holds it to the bit).  Rows past M are masked at the store.
//   Gather   how a row index becomes a source address (passed by value in the kernel arguments):
//              int ntaps()                              taps of the kernel window
//              Item item(m, live, q)                    this thread's gathered item: row m (live: m < M), 8-channel group q
//              Tap tap(t)                               tap index t decoded once per step
//              bool src(item, tap, chunk, ptr&)         is (item, tap) read at all, and from where (8 floats of the chunk)
//   Epi      what happens to a 4-channel group on its way out (passed by value in the kernel arguments):
//              float bias(c)                            added to channel c's accumulators before the staging tile
//              void store(row, c, v)                    output row `row`, channels c .. c + 3 of the conv's own
#pragma once
#include "mfma_rows.h"

// Intended to hold for the rest of the including file too: an Epi policy reproduces its net's arithmetic operation for operation only
// without fused multiply-adds, so every includer is compiled under it (both set it themselves as well, as with halo_conv3x3.h).
#pragma clang fp contract(off)

namespace gg {
namespace {

constexpr int BM = 128, NTHR = 256, YLD = 36;
constexpr int A_BYTES = BM * ROWB;                                              // 16 384

// F32: 1 = exact fp32 MFMA, 0 = split-bf16; BN: output channels per block (64 or 128); w: gridDim.y BN / RB row blocks of
// [ntaps][nchunk][RB][ROWB]
template <int F32, int BN, class Gather, class Epi>
__global__ __launch_bounds__(NTHR) void gather_gemm_kernel(const Gather g, const Epi epi, const float* w, const int nchunk,
                                                           const int M) {
    constexpr int RB = 64;                                      // output channels per row block of the weight image
    constexpr int WN = 2, WM = 2;                               // waves along the channels / the rows
    constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);     // 32 x 32 tiles per wave
    constexpr int BPIECES = BN * 8;                             // 16-byte weight pieces per step
    constexpr int BJ = BPIECES / NTHR;
    static_assert((BN == 64 || BN == 128) && BPIECES % NTHR == 0 && BN % RB == 0, "thread layout");
    constexpr int B_BYTES = BN * ROWB;
    static_assert(4 * 32 * YLD * 4 <= A_BYTES + B_BYTES, "the output staging tiles alias the operand buffers");
    __shared__ __attribute__((aligned(16))) unsigned char smem[A_BYTES + B_BYTES];
    __shared__ int s_out[BM];
    unsigned char* sA = smem;                                   // [128 rows][ROWB]
    unsigned char* sB = smem + A_BYTES;                         // [BN channels][ROWB]
    float* sY = reinterpret_cast<float*>(smem);                 // [4 waves][32][YLD] output staging (aliases the operands)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int wm = wave % WM, wn = wave / WM;
    const int m0 = blockIdx.x * BM;
    const int ntaps = g.ntaps();

    // this thread's two gathered items: (row m, 8-channel group q)
    typename Gather::Item it[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int item = tid + NTHR * j;
        const int m = m0 + (item >> 2);
        it[j] = g.item(m, m < M, item & 3);
    }
    const f32x8 zero8 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x8 ra[2];
    f32x4 rb[BJ];
    const unsigned char* wbase = reinterpret_cast<const unsigned char*>(w);
    auto fetch = [&](int step) {
        const int tap = step / nchunk, chunk = step - tap * nchunk;
        const typename Gather::Tap t = g.tap(tap);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float* src;
            const bool ok = g.src(it[j], t, chunk, src);
            ra[j] = ok ? load8(src) : zero8;
        }
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
            const int i = tid + NTHR * j;
            const int row = i >> 3;
            const int cb = blockIdx.y * (BN / RB) + row / RB;
            const unsigned char* wb = wbase + (((size_t)cb * ntaps + tap) * nchunk + chunk) * (RB * ROWB) + (size_t)(row % RB) * ROWB + (i & 7) * 16;
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

    const int nstep = ntaps * nchunk;
    fetch(0);
    for (int step = 0; step < nstep; ++step) {
        __syncthreads();                                        // every reader of the previous step's LDS image is done
        stage();
        if (step + 1 < nstep) fetch(step + 1);
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

    // ---- epilogue: one 32 x 32 tile per wave and pass through the LDS staging tile, then one Epi::store per 4-channel group ----
    float* myY = sY + wave * 32 * YLD;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int co = blockIdx.y * BN + wn * (32 * TN) + tn * 32;
            const float bsv = epi.bias(co + li);
            __syncthreads();                                    // the operands (or the previous pass's tile) are read
#pragma unroll
            for (int r = 0; r < 16; ++r) myY[((r & 3) + 8 * (r >> 2) + 4 * kh) * YLD + li] = acc[tm][tn][r] + bsv;
            __syncthreads();
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) {
                const int row = ps * 8 + (lane >> 3), c4 = lane & 7;
                const int pix = s_out[wm * (32 * TM) + tm * 32 + row];
                if (pix < 0) continue;
                epi.store(pix, co + c4 * 4, *reinterpret_cast<const f32x4*>(myY + row * YLD + c4 * 4));
            }
        }
}

// w [Cout][Cin][ntap] -> [ceil(Cout / RB)][ntap][Cin / 32][RB co][128 bytes]: 32 floats (SPLIT = 0) or [32 hi | 32 lo] bf16 (SPLIT = 1);
// rows of channels past Cout are zero.  n: elements of the image
template <int SPLIT, int RB>
__global__ void gather_gemm_pack_kernel(const float* __restrict__ w, unsigned char* __restrict__ out, int Cin, int Cout, int ntap, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ci = (int)(i & 31), co = (int)((i >> 5) % RB);
    int64_t rest = i / (32 * RB);
    const int nchunk = Cin / KC;
    const int chunk = (int)(rest % nchunk);
    rest /= nchunk;
    const int tap = (int)(rest % ntap);
    const int c = (int)(rest / ntap) * RB + co;
    const float v = c < Cout ? w[((size_t)c * Cin + chunk * KC + ci) * ntap + tap] : 0.f;
    pack_row_store<SPLIT>(out + (size_t)(i >> 5) * ROWB, ci, v);
}

template <int RB>
void gather_gemm_pack(const float* w, void* out, int Cin, int Cout, int ntap, int64_t n, int split, hipStream_t st) {
    const dim3 grid((unsigned)((n + 255) / 256));
    unsigned char* o = static_cast<unsigned char*>(out);
    if (split) hipLaunchKernelGGL((gather_gemm_pack_kernel<1, RB>), grid, dim3(256), 0, st, w, o, Cin, Cout, ntap, n);
    else hipLaunchKernelGGL((gather_gemm_pack_kernel<0, RB>), grid, dim3(256), 0, st, w, o, Cin, Cout, ntap, n);
}

}  // namespace
}  // namespace gg
