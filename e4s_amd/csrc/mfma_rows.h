// The 128-byte swizzled LDS row that the 32-channel-chunk MFMA convs share (conv_c32.hip, halo_conv3x3.h, gather_gemm.h): one
// 32-channel chunk of a pixel (or of a weight row) per row, as [32 hi | 32 lo] bf16 (split-bf16) or as 32 floats (exact fp32).
#pragma once
#include "common.h"

namespace {

constexpr int KC = 32, ROWB = 128, LO = 64;                                     // channels per chunk, bytes per row, offset of the lo halves

// byte offset of 16-byte granule g (0..7) of row r.  split-bf16: granules 0..3 hold 8 hi channels each, g + 4 (the same offset ^ 64)
// their lo halves, the second k-step is ^ 32; fp32: granule g holds channels 4 g .. 4 g + 3.
// A ds_read_b128 is served in groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...) that must hit 16 different 16-byte
// slots of the 256-byte bank line.  Weights (swz): a group reads 16 rows of one tap at one logical granule; rows of one parity share a
// 128-byte half and have eight different (r >> 1) & 7 -- conflict free.  Halo (swz_halo): a group's pixels are columns x0 .. x0 + 15
// of TWO image rows ({0-3, 12-15} of one, {4-11} of the next), so the swizzle keys on the halo COLUMN hx = h % HALO_W (the row pitch
// of an 18-wide halo is even: a row's parity is its column's): (hx & 1, (hx >> 1) & 7) takes 16 different values -- conflict free
// (keyed on the row itself, like the 144-byte padded rows of round 3, every group was 2-way: the 30.9 % of conflict cycles in r04f's
// counters of conv_c32.hip).  The halo argument holds for HALO_W = 18 only: the stride-2 tile of halo_conv3x3.h (HALO_W = 33, an odd
// pitch, fragment columns two apart) uses the same key, and its conflicts are neither analysed nor measured.
__device__ __forceinline__ int swz(int r, int g) { return r * ROWB + ((g ^ ((r >> 1) & 7)) << 4); }
template <int HALO_W>
__device__ __forceinline__ int swz_halo(int h, int g) { return h * ROWB + ((g ^ (((h % HALO_W) >> 1) & 7)) << 4); }

// 8 floats -> 8 hi bf16 at off and the 8 lo bf16 (of the remainders) at off ^ LO
__device__ __forceinline__ void split_store(unsigned char* base, int off, const f32x8 v) {
    const bf16x8 h = __builtin_convertvector(v, bf16x8);
    const f32x8 r = v - __builtin_convertvector(h, f32x8);
    const bf16x8 l = __builtin_convertvector(r, bf16x8);
    *reinterpret_cast<bf16x8*>(base + off) = h;
    *reinterpret_cast<bf16x8*>(base + (off ^ LO)) = l;
}

// element ci of a packed (unswizzled, global-memory) weight row: 32 floats (SPLIT = 0) or [32 hi | 32 lo] bf16 (SPLIT = 1)
template <int SPLIT>
__device__ __forceinline__ void pack_row_store(unsigned char* row, int ci, float v) {
    if (SPLIT) {
        const __bf16 h = (__bf16)v;
        const __bf16 l = (__bf16)(v - (float)h);
        reinterpret_cast<__bf16*>(row)[ci] = h;
        reinterpret_cast<__bf16*>(row + LO)[ci] = l;
    } else {
        reinterpret_cast<float*>(row)[ci] = v;
    }
}

}  // namespace
