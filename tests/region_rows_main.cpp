// Stand-alone check of the layout part of csrc/region_rows.h and csrc/rows64.h (built and run by tests/test_region_rows_host.py with
// -fsanitize=address,undefined; the headers are plain C++ outside __HIPCC__):
//   1. halo_row(h), h < HALO, and var_row(v), v < VMAX, are NROW distinct rows in [0, NROW): halo and variant rows partition the buffer;
//   2. own-row fragment reads are free of LDS bank conflicts: a ds_read_b128 is served in groups of 16 lanes -- {0-3, 12-15, 20-27} and
//      {4-11, 16-19, 28-31} of each half wave (mfma_rows.h) -- and for every 32-pixel MFMA row tile of the 16 x 16 tile, every one of the
//      nine tap shifts, both k-halves and the hi and the lo granule, the 16 lanes of a group hit 16 different 16-byte slots of the
//      256-byte bank line.
// Prints one line per violated case and "OK <rows> <groups>" at the end; exit status 1 if anything failed.
#include <cstdio>
#include <vector>

#include "region_rows.h"

using namespace region_rows;

int main() {
    int bad = 0;
    std::vector<int> seen(NROW, 0);
    for (int h = 0; h < HALO; ++h) {
        const int r = halo_row(h);
        if (r < 0 || r >= NROW) { std::printf("FAILED halo_row(%d) = %d out of range\n", h, r); return 1; }
        ++seen[r];
    }
    for (int v = 0; v < VMAX; ++v) {
        const int r = var_row(v);
        if (r < 0 || r >= NROW) { std::printf("FAILED var_row(%d) = %d out of range\n", v, r); return 1; }
        ++seen[r];
    }
    for (int r = 0; r < NROW; ++r)
        if (seen[r] != 1) { std::printf("FAILED row %d used %d times\n", r, seen[r]); ++bad; }
    // every byte of a row is reached exactly once through its four granules
    for (int r = 0; r < NROW; ++r) {
        unsigned mask = 0;
        for (int g = 0; g < 4; ++g) {
            const int off = swz(r, g);
            if (off / ROWB != r || off % 16) { std::printf("FAILED swz(%d, %d) = %d leaves the row\n", r, g, off); ++bad; }
            mask |= 1u << (off % ROWB / 16);
        }
        if (mask != 15u) { std::printf("FAILED granules of row %d overlap\n", r); ++bad; }
    }

    static const int group_lanes[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                           {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
    int groups = 0;
    for (int tile = 0; tile < BM / 32; ++tile)                      // 32-pixel MFMA row tile: pixels of two image rows
        for (int tap = 0; tap < 9; ++tap)
            for (int kh = 0; kh < 2; ++kh)                          // lanes 32-63 read the second k-half
                for (int lo = 0; lo < 2; ++lo)                      // the lo granule is at offset ^ 32
                    for (int grp = 0; grp < 2; ++grp) {
                        unsigned slots = 0;
                        for (int i = 0; i < 16; ++i) {
                            const int m = tile * 32 + group_lanes[grp][i];
                            const int my = m / TW, mx = m % TW;
                            const int h = (my + tap / 3) * HALO_W + mx + tap % 3;
                            const int off = swz(halo_row(h), kh) ^ (lo ? 32 : 0);
                            slots |= 1u << (off % 256 / 16);
                        }
                        ++groups;
                        if (slots != 0xFFFFu) {
                            std::printf("FAILED conflict: row tile %d tap %d k-half %d %s lanes %d: slots %04x\n", tile, tap, kh, lo ? "lo" : "hi",
                                        group_lanes[grp][0], slots);
                            ++bad;
                        }
                    }
    if (bad) return 1;
    std::printf("OK %d %d\n", NROW, groups);
    return 0;
}
