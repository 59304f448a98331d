// LDS addressing of conv_gather1w_kernel (conv_gather1w.hip): a stage is 256 rows (the tile's pixels) of 144 bytes [32 hi bf16 | 32 lo bf16 | 16 pad].
//   * Fragment reads (ds_read_b128, served in four groups of 16 lanes, 16-byte slot = (a / 16) mod 16 of the 256-byte bank row): lane l reads row
//     32 g + (l & 31) at + 16 (l >> 5); a group's lanes ({0-3, 12-15, 20-27}, ...) cover sixteen rows that differ mod 16 and 9 r mod 16 is a
//     bijection on the slots: conflict free.
//   * Staging stores (ds_write_b128, served in eight groups of 8 consecutive lanes, slot = (a / 16) mod 8 of the 128-byte write row): thread t stores
//     the 8-channel group t & 3 of rows stage_row(t >> 2) + 64 j.  stage_row swaps bits 0 and 2 of its argument, so a group's two rows are r and
//     r + 4: 64 bytes apart in the write row, eight different slots.  (Rows r and r + 1, the 8-wave kernel's deal, overlap in three of the four.)
// Plain C++ with no device code: tests/gather1w_rows_main.cpp checks both claims for every lane group on the host.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define E4S_G1W_HD __host__ __device__ inline
#else
#define E4S_G1W_HD inline
#endif

namespace e4s_gather1w {

constexpr int kRows = 256, kRowBytes = 144, kLo = 64;       // rows per stage, bytes per row, offset of the lo halves

// the first of the four rows thread t stages (the others: + 64, + 128, + 192); q = t >> 2 in [0, 64)
E4S_G1W_HD int stage_row(int q) { return (q & ~5) | ((q & 1) << 2) | ((q >> 2) & 1); }
// byte offset inside a stage of the hi half of 8-channel group aq of row r (lo: + kLo)
E4S_G1W_HD int stage_dst(int r, int aq) { return r * kRowBytes + aq * 16; }
// byte offset of lane `lane`'s hi fragment of 32-row group g, k-step kk (lo: + kLo)
E4S_G1W_HD int frag_src(int g, int lane, int kk) { return (g * 32 + (lane & 31)) * kRowBytes + (lane >> 5) * 16 + kk * 32; }

}  // namespace e4s_gather1w
