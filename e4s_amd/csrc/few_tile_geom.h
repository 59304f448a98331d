// Geometry of the PACKED small-map tiles of conv_bf16x3_region_kernel (conv_bf16x3.hip); the K-split rule of those launches is split_policy.h's pack_split.
//
// The region-select kernel cuts 256-row x 128-column GEMM tiles whose rows are the pixels of ONE 16x16 patch of ONE image: a 4x4 map fills 16
// of the 256 rows, an 8x8 map 64.  A packed tile holds n_img WHOLE images of such a map instead:
//   * GEMM row m = (j, y, x): j = m / (Ha Wa) the image inside the tile, (y, x) its pixel; rows of images past n_img or past the batch are dead;
//   * image j owns the (Ha+2) x (Wa+2) block [j hblk, (j+1) hblk) of the kernel's 324-row halo array, its own zero ring included, so no tap of
//     one image ever reads a pixel of its neighbour;
//   * row m's tap (ty, tx) reads halo slot  j hblk + (y + ty)(Wa+2) + (x + tx).
// n_img = min(324 / ((Ha+2)(Wa+2)), 256 / (Ha Wa)); a map is eligible when n_img >= 2 (9 images at 4x4, 3 at 8x8; 16x16 is not).
// Plain C++ with no device code, so the host tests compile it as it is.
#pragma once
#include "split_policy.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define E4S_FT_HD __host__ __device__ inline
#else
#define E4S_FT_HD inline
#endif

namespace e4s_few_tile {

constexpr int kRows = 256;        // GEMM rows of a tile
constexpr int kHalo = 324;        // halo rows of a tile: (16 + 2)^2
using e4s_split::kBlocks;          // blocks a launch should reach, and the K split of a packed launch: split_policy.h
using e4s_split::pack_split;

struct PackGeom {
    int ha, wa;        // map size
    int npix;          // Ha Wa: GEMM rows per image
    int pitch;         // Wa + 2: halo rows per image row
    int hblk;          // (Ha + 2)(Wa + 2): halo rows per image
    int n_img;         // images per tile (0: the map is not eligible)
};

E4S_FT_HD PackGeom pack_geom(int ha, int wa) {
    PackGeom g = {ha, wa, 0, 0, 0, 0};
    if (ha < 1 || wa < 1 || ha > 16 || wa > 16) return g;
    g.npix = ha * wa;
    g.pitch = wa + 2;
    g.hblk = (ha + 2) * (wa + 2);
    const int by_halo = kHalo / g.hblk, by_rows = kRows / g.npix;
    const int n = by_halo < by_rows ? by_halo : by_rows;
    g.n_img = n >= 2 ? n : 0;
    return g;
}

E4S_FT_HD int pack_tiles(const PackGeom& g, int batch) { return (batch + g.n_img - 1) / g.n_img; }      // tiles per class

struct PackRow {
    int j, y, x;       // image inside the tile, pixel
    int image;         // sample index, -1: dead row
};

// GEMM row m of tile t
E4S_FT_HD PackRow pack_row(const PackGeom& g, int t, int m, int batch) {
    PackRow r;
    r.j = m / g.npix;
    const int rem = m - r.j * g.npix;
    r.y = rem / g.wa;
    r.x = rem - r.y * g.wa;
    const int image = t * g.n_img + r.j;
    r.image = (r.j < g.n_img && image < batch) ? image : -1;
    return r;
}

// halo slot that row (j, y, x) reads through tap (0, 0); tap (ty, tx) adds pack_tap(g, ty, tx)
E4S_FT_HD int pack_arow(const PackGeom& g, int j, int y, int x) { return j * g.hblk + y * g.pitch + x; }
E4S_FT_HD int pack_tap(const PackGeom& g, int ty, int tx) { return ty * g.pitch + tx; }

struct PackSlot {
    int j, iy, ix;     // image inside the tile, INPUT pixel (-1 or Ha / Wa: the zero ring)
    int image;         // sample index, -1: no image behind this slot (it is zero filled)
};

// halo slot h of tile t
E4S_FT_HD PackSlot pack_slot(const PackGeom& g, int t, int h, int batch) {
    PackSlot s;
    s.j = h / g.hblk;
    const int rem = h - s.j * g.hblk;
    const int hy = rem / g.pitch;
    s.iy = hy - 1;
    s.ix = rem - hy * g.pitch - 1;
    const int image = t * g.n_img + s.j;
    s.image = (s.j < g.n_img && image < batch) ? image : -1;
    return s;
}

}  // namespace e4s_few_tile
