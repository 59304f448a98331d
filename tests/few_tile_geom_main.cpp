// Stand-alone check of csrc/few_tile_geom.h (built and run by tests/test_few_tile_host.py with -fsanitize=address,undefined): the packed
// tiles are walked exactly as conv_bf16x3_region_kernel walks them -- halo array of 324 slots filled slot by slot from pack_slot, rows read
// through pack_arow + pack_tap -- for every eligible map and every batch from 1 to 2 n_img + 1.  Prints one line per eligible map
// "h w n_img" (the Python side compares the list with its own restatement) and exits non-zero on the first violated property.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "few_tile_geom.h"

using namespace e4s_few_tile;

#define REQUIRE(c)                                                                                    \
    do {                                                                                              \
        if (!(c)) {                                                                                   \
            std::printf("FAILED %s (h %d w %d batch %d tile %d)\n", #c, h, w, batch, t);              \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

int main() {
    int eligible = 0;
    for (int h = 1; h <= 18; ++h)
        for (int w = 1; w <= 18; ++w) {
            int batch = 0, t = 0;
            const PackGeom g = pack_geom(h, w);
            const int by_halo = kHalo / ((h + 2) * (w + 2)), by_rows = kRows / (h * w);
            const int want = by_halo < by_rows ? by_halo : by_rows;
            REQUIRE(g.n_img == ((want >= 2 && h <= 16 && w <= 16) ? want : 0));
            if (!g.n_img) continue;
            ++eligible;
            std::printf("%d %d %d\n", h, w, g.n_img);
            REQUIRE(g.n_img * g.hblk <= kHalo && g.n_img * g.npix <= kRows);
            for (batch = 1; batch <= 2 * g.n_img + 1; ++batch) {
                std::vector<int> seen((size_t)batch * h * w, 0);
                const int tiles = pack_tiles(g, batch);
                REQUIRE(tiles == (batch + g.n_img - 1) / g.n_img);
                for (t = 0; t < tiles; ++t) {
                    // the halo array as the kernel stages it: slot -> image * 1e6 + input pixel, -1 zero ring / no image
                    std::vector<int> halo(kHalo, -2);
                    for (int s = 0; s < kHalo; ++s) {
                        const PackSlot ps = pack_slot(g, t, s, batch);
                        const bool inside = ps.image >= 0 && ps.iy >= 0 && ps.iy < h && ps.ix >= 0 && ps.ix < w;
                        if (ps.image >= 0) REQUIRE(ps.image == t * g.n_img + ps.j && ps.iy >= -1 && ps.iy <= h && ps.ix >= -1 && ps.ix <= w);
                        halo[s] = inside ? ps.image * 1000000 + ps.iy * w + ps.ix : -1;
                    }
                    for (int m = 0; m < kRows; ++m) {
                        const PackRow r = pack_row(g, t, m, batch);
                        if (r.image < 0) continue;
                        REQUIRE(r.image < batch && r.image / g.n_img == t && r.j < g.n_img && r.y < h && r.x < w);
                        ++seen[((size_t)r.image * h + r.y) * w + r.x];
                        const int a = pack_arow(g, r.j, r.y, r.x);
                        for (int ty = 0; ty < 3; ++ty)
                            for (int tx = 0; tx < 3; ++tx) {
                                const int s = a + pack_tap(g, ty, tx);
                                REQUIRE(s >= 0 && s < kHalo);
                                REQUIRE(s >= r.j * g.hblk && s < (r.j + 1) * g.hblk);          // its own image's block
                                const int iy = r.y + ty - 1, ix = r.x + tx - 1;
                                const bool inside = iy >= 0 && iy < h && ix >= 0 && ix < w;
                                REQUIRE(halo.at(s) == (inside ? r.image * 1000000 + iy * w + ix : -1));      // that pixel, or the zero ring
                            }
                    }
                }
                t = -1;
                for (size_t i = 0; i < seen.size(); ++i) REQUIRE(seen[i] == 1);      // every (image, y, x) in exactly one live row
            }
        }
    // the K-split rule: every chunk in exactly one non-empty split, one round of blocks where the tiles alone fit one
    for (long long tiles = 1; tiles <= 300; ++tiles)
        for (int nchunk = 1; nchunk <= 32; ++nchunk) {
            int ksplit, cper;
            pack_split(tiles, nchunk, ksplit, cper);
            if (ksplit < 1 || cper < 1 || (long long)ksplit * cper < nchunk || (ksplit - 1) * cper >= nchunk || ksplit > nchunk ||
                (ksplit > 1 && tiles * ksplit > kBlocks)) {
                std::printf("FAILED pack_split(%lld, %d) = %d x %d\n", tiles, nchunk, ksplit, cper);
                return 1;
            }
            std::printf("split %lld %d %d %d\n", tiles, nchunk, ksplit, cper);
        }
    std::printf("OK %d\n", eligible);
    return 0;
}
