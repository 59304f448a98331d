// Stand-alone check of csrc/gather1w_rows.h (built and run by tests/test_gather1w_rows_host.py with -fsanitize=address,undefined): the LDS
// stage of conv_gather1w_kernel is written and read exactly as the kernel does it, lane group by lane group.
//   * every (row, 16-byte granule) of a stage's hi and lo halves is stored exactly once by the 256 threads x 4 items, inside the stage;
//   * every ds_write_b128 service group (8 consecutive lanes) hits 8 different 16-byte slots of the 128-byte write row;
//   * every ds_read_b128 service group (16 lanes: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, the same + 32) hits 16 different slots of the
//     256-byte bank row, for every 32-row group, k-step and half; and every fragment read lands on bytes that were stored.
// Prints the 64 values of stage_row (the Python side compares them with its restatement), then OK; exits non-zero on the first violation.
#include <cstdio>
#include <vector>

#include "gather1w_rows.h"

using namespace e4s_gather1w;

#define REQUIRE(c)                                           \
    do {                                                     \
        if (!(c)) {                                          \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__); \
            return 1;                                        \
        }                                                    \
    } while (0)

int main() {
    const int stage_bytes = kRows * kRowBytes;
    std::vector<int> written(stage_bytes / 16, 0);
    // staging stores: thread t, item j, half (hi | lo)
    for (int half = 0; half < 2; ++half)
        for (int j = 0; j < 4; ++j)
            for (int t0 = 0; t0 < 256; t0 += 8) {
                unsigned slots = 0;
                for (int t = t0; t < t0 + 8; ++t) {
                    const int q = t >> 2, aq = t & 3;
                    REQUIRE(stage_row(q) >= 0 && stage_row(q) < 64);
                    const int a = stage_dst(stage_row(q) + 64 * j, aq) + half * kLo;
                    REQUIRE(a >= 0 && a % 16 == 0 && a + 16 <= stage_bytes);
                    ++written.at(a / 16);
                    const unsigned bit = 1u << ((a / 16) % 8);
                    REQUIRE(!(slots & bit));              // ds_write_b128: 8 lanes, 8 different slots of the 128-byte row
                    slots |= bit;
                }
            }
    for (int r = 0; r < kRows; ++r)
        for (int gq = 0; gq < 9; ++gq) REQUIRE(written.at((r * kRowBytes) / 16 + gq) == (gq < 8 ? 1 : 0));      // each granule once, the pad never
    // fragment reads
    static const int groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                      {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                      {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    for (int g = 0; g < kRows / 32; ++g)
        for (int kk = 0; kk < 2; ++kk)
            for (int half = 0; half < 2; ++half)
                for (int sg = 0; sg < 4; ++sg) {
                    unsigned slots = 0;
                    for (int i = 0; i < 16; ++i) {
                        const int a = frag_src(g, groups[sg][i], kk) + half * kLo;
                        REQUIRE(a >= 0 && a % 16 == 0 && a + 16 <= stage_bytes);
                        REQUIRE(written.at(a / 16) == 1);
                        const unsigned bit = 1u << ((a / 16) % 16);
                        REQUIRE(!(slots & bit));          // ds_read_b128: 16 lanes, 16 different slots of the 256-byte row
                        slots |= bit;
                    }
                }
    for (int q = 0; q < 64; ++q) std::printf("%d\n", stage_row(q));
    std::printf("OK\n");
    return 0;
}
