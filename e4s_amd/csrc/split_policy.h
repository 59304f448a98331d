// Every K-split rule of the split-bf16 conv family, once: pure functions of integers, plain C++17 with no device code (the host tests compile
// this file as it is: tests/split_policy_main.cpp).  A rule answers (ksplit, cper): split ks contracts the input-channel chunks
// [ks cper, min(nchunk, (ks + 1) cper)).  Every rule guarantees ksplit cper >= nchunk > (ksplit - 1) cper: no split is empty, every chunk
// is in exactly one.  (e4s_conv_mfma_f32's f32_split reads the launch parameters and is a different rule: conv_mfma.hip.)
#pragma once

namespace e4s_split {

constexpr int kBlocks = 256;        // blocks a launch should reach: one per CU
constexpr int kChunk = 32;          // input channels per chunk of the plain / masked / gather rules (the Winograd kernels count 16s)

// few tiles (<= kBlocks / 2, so that two K halves still fit one round of blocks; >= 4 chunks): ceil(kBlocks / tiles) splits, at most
// nchunk / 2 of them.  The splits before the last hold cper >= 2 chunks; the LAST may hold one (nchunk 16, 6 wanted: 3 3 3 3 3 1).
inline void few_tiles_split(long long tiles, int nchunk, int& ksplit, int& cper) {
    ksplit = 1;
    cper = nchunk;
    if (tiles < 1 || tiles > kBlocks / 2 || nchunk < 4) return;
    long long want = (kBlocks + tiles - 1) / tiles;
    if (want > nchunk / 2) want = nchunk / 2;
    if (want < 2) return;
    cper = (nchunk + (int)want - 1) / (int)want;
    ksplit = (nchunk + cper - 1) / cper;
}

// the Winograd kernels' form: few_tiles_split, but a split whose last part would hold ONE chunk is refused (the launch stays whole), so
// every split holds >= 2 chunks
inline void few_tiles_split_guarded(long long tiles, int nchunk, int& ksplit, int& cper) {
    few_tiles_split(tiles, nchunk, ksplit, cper);
    if (ksplit > 1 && nchunk - (ksplit - 1) * cper < 2) ksplit = 1, cper = nchunk;
}

// strided gather kernel: only the 3x3 launches that leave three quarters of the chip idle AND are deep enough that a split still runs >= 18
// stages -- few_tiles_split on <= kBlocks / 4 tiles and >= 8 chunks.  (Cin < 256 stays whole: those launches keep their fused epilogue
// statistics, and their 36 / 72 stages are no longer than one split of the deep ones.)
inline void gather_split(long long tiles, int cin, int ntaps, int& ksplit, int& cper) {
    ksplit = 1;
    cper = cin / kChunk;
    if (ntaps != 9 || cin < 8 * kChunk || cin % kChunk || tiles < 1 || tiles > kBlocks / 4) return;
    few_tiles_split(tiles, cin / kChunk, ksplit, cper);
}

// packed small-map masked launch of `tiles` blocks (all classes and column tiles, few_tile_geom.h): as many splits as still fit ONE round of
// kBlocks blocks (a launch just past 256 blocks would run two rounds), down to one chunk per block
inline void pack_split(long long tiles, int nchunk, int& ksplit, int& cper) {
    ksplit = 1;
    cper = nchunk;
    if (tiles < 1 || nchunk < 2) return;
    long long want = kBlocks / tiles;
    if (want > nchunk) want = nchunk;
    if (want < 2) return;
    cper = (nchunk + (int)want - 1) / (int)want;
    ksplit = (nchunk + cper - 1) / cper;
}

}  // namespace e4s_split
