// Stand-alone check of csrc/split_policy.h (built and run by tests/test_few_tile_host.py with -fsanitize=address,undefined): every K-split
// rule over tiles 1..300 x chunks 1..128.  The splits are walked as the kernels walk them -- split ks takes the chunks
// [ks cper, min(nchunk, (ks + 1) cper)) -- and every chunk must lie in exactly one non-empty split; ksplit cper >= nchunk > (ksplit - 1) cper;
// the Winograd form never leaves a last split of one chunk.  Prints one row "rule tiles nchunk ksplit cper" per pair (the Python side
// compares every row with its own restatement of the rule) and exits non-zero on the first violated property.
#include <cstdio>
#include <vector>

#include "split_policy.h"

using namespace e4s_split;

static bool walk(const char* rule, long long tiles, int nchunk, int ksplit, int cper, bool guarded) {
    bool ok = ksplit >= 1 && cper >= 1 && (long long)ksplit * cper >= nchunk && (long long)(ksplit - 1) * cper < nchunk;
    if (ok) {
        std::vector<int> seen((size_t)nchunk, 0);
        for (int ks = 0; ks < ksplit; ++ks) {
            const int lo = ks * cper, hi = lo + cper < nchunk ? lo + cper : nchunk;
            ok &= hi > lo;                                             // no empty split
            for (int c = lo; c < hi; ++c) ++seen.at((size_t)c);
        }
        for (int c = 0; c < nchunk; ++c) ok &= seen[(size_t)c] == 1;
        if (guarded && ksplit > 1) ok &= nchunk - (ksplit - 1) * cper >= 2;
    }
    if (!ok) std::printf("FAILED %s(%lld, %d) = %d x %d\n", rule, tiles, nchunk, ksplit, cper);
    else std::printf("%s %lld %d %d %d\n", rule, tiles, nchunk, ksplit, cper);
    return ok;
}

int main() {
    for (long long tiles = 1; tiles <= 300; ++tiles)
        for (int nchunk = 1; nchunk <= 128; ++nchunk) {
            int k, c;
            few_tiles_split(tiles, nchunk, k, c);
            if (!walk("few", tiles, nchunk, k, c, false)) return 1;
            few_tiles_split_guarded(tiles, nchunk, k, c);
            if (!walk("wino", tiles, nchunk, k, c, true)) return 1;
            gather_split(tiles, nchunk * kChunk, 9, k, c);
            if (!walk("gather", tiles, nchunk, k, c, false)) return 1;
            gather_split(tiles, nchunk * kChunk, 1, k, c);
            if (!walk("gather1x1", tiles, nchunk, k, c, false) || k != 1) return 1;
            pack_split(tiles, nchunk, k, c);
            if (!walk("pack", tiles, nchunk, k, c, false) || (k > 1 && tiles * k > kBlocks)) return 1;
        }
    std::printf("OK\n");
    return 0;
}
