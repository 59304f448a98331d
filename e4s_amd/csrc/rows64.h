// The 64-byte swizzled LDS row of the 16-channel-chunk MFMA convs (conv_region.hip, conv_region1w.hip through region_rows.h; conv_wino.hip,
// conv_wino1w.hip): one 16-channel chunk of a pixel (or of a weight row) per row, as [16 hi | 16 lo] bf16, UNPADDED.
// Not to be confused with the 128-byte row of the 32-channel-chunk convs (mfma_rows.h), which has the same three names in the file-local
// namespace: everything here lives in namespace rows64 and a file says `using rows64::swz;` for what it takes, so a file that included
// both headers would not compile instead of picking one of them silently.
// Plain C++ outside __HIPCC__, so the host tests compile it as it is.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define E4S_R64_HD __host__ __device__ __forceinline__
#else
#define E4S_R64_HD inline
#endif

namespace rows64 {

constexpr int KC = 16, ROWB = 64;         // channels per chunk, bytes per row; the lo half of a 16-byte granule is at offset ^ 32

// byte offset of 16-byte granule g (0, 1: the hi halves of channels 0-7, 8-15; 2, 3: their lo halves) of a row: the granule index is XORed
// with (row >> 2) & 3 (round 4; the 80-byte padded rows of round 3 ran at 37-39 % bank-conflict cycles).  The 256-byte bank line holds
// four rows of four granules, so for one logical granule the 16-byte slot hit is a bijection of row & 15: a ds_read_b128 group of 16
// lanes is conflict free when its rows have 16 different residues mod 16 (tests/region_rows_main.cpp walks that for the masked convs'
// tile).
E4S_R64_HD int swz(int row, int g) { return row * ROWB + ((g ^ ((row >> 2) & 3)) << 4); }

}  // namespace rows64
