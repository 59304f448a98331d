// Shared helpers for the gfx950 kernels of libe4s_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "e4s_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define E4S_CHECK_LAUNCH()                         \
    do {                                           \
        hipError_t e__ = hipGetLastError();        \
        if (e__ != hipSuccess) return (int)e__;    \
    } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// a * b rounded on its own: the product carries no `contract` flag, so no later add can fuse with it under hipcc's default
// -ffp-contract=fast-honor-pragmas (__fmul_rn is a plain operator in this ROCm's headers and does fuse; stitch.hip has the story).
// The per-channel noise term noise_w * noise[pix][co] of the conv epilogues: the per-pixel term is such a product too, rounded by
// its trip through the tile's row table.
__device__ __forceinline__ float e4s_mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// wave64 all-lanes sum
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// wave64 sums of N values per lane at once (N a power of two <= 64): a butterfly that halves the set at every step -- the lane keeps
// the half its lane bit selects and adds the partner's copy of it -- then finishes the single survivor like wave_sum.  N - 1 + (6 -
// log2 N) shuffles in place of 6 N.  Afterwards v[0] is the complete sum of value (lane >> (6 - log2 N)), on every lane of that group.
// Each value goes through wave_sum's additions (offsets 32, 16, ..., 1; a + b == b + a), so it has wave_sum's bits.
template <int N, int CNT, int O>
__device__ __forceinline__ void packed_wave_sum_step(float (&v)[N], const int lane) {      // every index a compile-time constant
    if constexpr (O > 0) {
        if constexpr (CNT > 1) {
            constexpr int H = CNT / 2;
            const bool up = lane & O;
#pragma unroll
            for (int i = 0; i < H; ++i) {
                const float keep = up ? v[i + H] : v[i], send = up ? v[i] : v[i + H];
                v[i] = keep + __shfl_xor(send, O, 64);
            }
            packed_wave_sum_step<N, H, O / 2>(v, lane);
        } else {
            v[0] += __shfl_xor(v[0], O, 64);
            packed_wave_sum_step<N, 1, O / 2>(v, lane);
        }
    }
}

template <int N>
__device__ __forceinline__ void packed_wave_sum(float (&v)[N], const int lane) {
    static_assert(N >= 1 && N <= 64 && (N & (N - 1)) == 0, "N: a power of two <= 64");
    packed_wave_sum_step<N, N, 32>(v, lane);
}

// 4x4 transpose inside each quad of lanes (two DPP quad_perm exchanges): in: a_i = M[i][lane & 3]; out: a_k = M[lane & 3][k].
// MFMA 32x32 accumulators hold one COLUMN per lane and rows (r & 3) + 8 (r >> 2) + 4 kh in register r: transposing registers
// 4g .. 4g+3 across the quad gives each lane four consecutive columns of ONE row -- a 16-byte NHWC store instead of four 4-byte
// ones.  (Stores straight from the accumulators are store-ISSUE bound on gfx950: ~70 cycles per store instruction whatever its
// width; measured on conv_c32.hip: 128 -> 32 store instructions per tile = 0.86 -> 0.70 ms.)
__device__ __forceinline__ float e4s_dpp_f32(float v, const int ctrl_b1_or_4e) {
    return ctrl_b1_or_4e == 0xB1
               ? __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true))     // quad_perm [1,0,3,2]
               : __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
}

__device__ __forceinline__ void quad_transpose4(float& a0, float& a1, float& a2, float& a3, const int lane) {
    const bool odd = lane & 1, hi = lane & 2;
    const float r01 = e4s_dpp_f32(odd ? a0 : a1, 0xB1), r23 = e4s_dpp_f32(odd ? a2 : a3, 0xB1);
    if (odd) { a0 = r01; a2 = r23; } else { a1 = r01; a3 = r23; }
    const float ra = e4s_dpp_f32(hi ? a0 : a2, 0x4E), rb = e4s_dpp_f32(hi ? a1 : a3, 0x4E);
    if (hi) { a0 = ra; a1 = rb; } else { a2 = ra; a3 = rb; }
}

// XCD-aware bijective remap of a 1-D block id: consecutive logical ids land on the same XCD
// (hardware places block b on XCD b % 8), so tiles that share an A panel share an L2.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = bid & 7, slot = bid >> 3;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + slot;
}

// Kernels that need more than 64 KB of dynamic LDS must raise hipFuncAttributeMaxDynamicSharedMemorySize first.  The
// attribute belongs to the function as loaded on ONE device, so it is set once per (kernel, device): `mask` (one static
// per launch site) has a bit per device ordinal; atomics keep concurrent host threads safe.
static inline int e4s_ensure_dyn_smem(const void* fn, int bytes, std::atomic<uint64_t>& mask) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    const uint64_t bit = 1ull << (dev & 63);
    if (mask.load(std::memory_order_acquire) & bit) return 0;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    mask.fetch_or(bit, std::memory_order_release);
    return 0;
}

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// grid of 256-thread blocks over n items
inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// 8 consecutive floats as two 16-byte loads
__device__ __forceinline__ f32x8 load8(const float* src) {
    const f32x4 lo4 = *reinterpret_cast<const f32x4*>(src);
    const f32x4 hi4 = *reinterpret_cast<const f32x4*>(src + 4);
    return f32x8{lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
}

// The reference's label lookup (F.interpolate(mode='nearest'), model.py:391) = ATen's legacy nearest source index (UpSample.h
// nearest_neighbor_compute_source_index): float scale, floorf, clamp.  The masked forward, its backward, the plan and ToRGB must agree
// on it bit for bit: this is the only definition.
__device__ __forceinline__ int nearest_src(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}

// LDS-only workgroup barrier: every LDS access of this wave issued so far has completed (lgkmcnt(0)); global loads stay in flight
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// make_coordinate_grid's coordinate of index i of n: 2 (i / (n - 1)) - 1 in float (n = 1: 0 / 0, NaN, as the reference); the product and
// the difference stay two operations, as in the translation units that use it (they are under `fp contract(off)` as a whole)
__device__ __forceinline__ float grid_coord(int i, int n) {
#pragma clang fp contract(off)
    return 2.f * ((float)i / (float)(n - 1)) - 1.f;
}
