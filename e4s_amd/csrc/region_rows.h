// The "variant rows" tile of the masked StyledConv, as conv_region.hip (8 waves) and conv_region1w.hip (one wave per SIMD)
// both mean it: a 16 x 16 pixel tile, its 18 x 18 halo staged once per 16-channel chunk scaled with each halo pixel's OWN region's style,
// plus one variant row per (halo pixel, foreign region that reads it).  Here: the LDS row layout, the tile tables and their analysis
// (label map -> variant rows -> per-lane row table -> staging items), the tile decode and the scale + split of a staged row.
// NOT here, on purpose: step 1 of the analysis (labels, noise and output offsets into the tables).  The 8-wave kernel fetches them with
// branchy loads under exec masks; the one-wave kernel issues ONE straight-line batch of clamped loads and selects afterwards, because
// nothing else runs on its CU while the tile is analysed (measured; comment at its step 1).  The pipelines, wave layouts, K split and
// epilogues are each kernel's own as well.  The one-wave kernel also writes decode_tile, label_at, variant_rows and staging_item out in its
// own body, word for word (it shares the constants, the layout, the tables, tap_row, load8 and scale_split_store): through the functions
// its prologue compiles differently and its polyphase launch measured 0.5-0.8 % slower; change both places together.
// The layout part is plain C++ (the host test tests/region_rows_main.cpp compiles it); what needs device builtins is behind __HIPCC__.
#pragma once
#include "rows64.h"
#ifdef __HIPCC__
#include "common.h"
#endif

namespace region_rows {

using rows64::KC;
using rows64::ROWB;
using rows64::swz;

constexpr int TW = 16, TH = 16, BM = TW * TH, HALO_W = TW + 2, HALO = (TH + 2) * HALO_W;
// A halo pixel (hy, hx) lives in LDS row hy * 32 + hx: the two 16-lane halves of an MFMA row tile (pixels of two image rows) are then 32
// rows apart, so the 16 lanes of every ds_read_b128 group touch 16 different residues mod 16 = 16 different (bank quad, swizzle) pairs
// for any tap shift -- own-row fragment reads are conflict free (rows64.h).  The 14 unused slots of each 32-row stripe hold the variant
// rows: 18 x 14 = 252 of them; a tile that needs more is left to the region-select kernel (flag table + a second, filtered launch).
constexpr int HSTR = 32, VSLOT = HSTR - HALO_W;
constexpr int VMAX = (TH + 2) * VSLOT, NROW = (TH + 2) * HSTR;
constexpr int A_BYTES = NROW * ROWB;      // one buffer of halo + variant rows
constexpr int MAXR = 16;                  // regions: a variant row is (halo pixel << 4) | region, the foreign regions of a pixel one u32 mask
static_assert(HALO + VMAX == NROW, "halo rows and variant rows partition the LDS rows exactly");
static_assert(HALO <= 6 * 64, "the scan of step 3 gives each lane of one wave six halo pixels");

E4S_R64_HD int halo_row(int h) { return (h / HALO_W) * HSTR + h % HALO_W; }          // LDS row of halo pixel h
E4S_R64_HD int var_row(int v) { return (v / VSLOT) * HSTR + HALO_W + v % VSLOT; }    // LDS row of variant row v

// the tile tables, as offsets from a base that each kernel places behind its own buffers
constexpr int TBL_OUT = 0;                                      // int   [BM]    output pixel offset or -1
constexpr int TBL_NZ = TBL_OUT + BM * 4;                        // float [BM]    noise term
constexpr int TBL_NEED = TBL_NZ + BM * 4;                       // u32   [HALO]  bit r: a foreign region r reads this halo pixel
constexpr int TBL_BASE = TBL_NEED + HALO * 4;                   // u16   [HALO]  first variant row of the halo pixel
constexpr int TBL_VAR = TBL_BASE + (HALO * 2 + 15) / 16 * 16;   // u16   [VMAX]  variant row -> (halo pixel << 4) | region
constexpr int TBL_LAB = TBL_VAR + VMAX * 2;                     // u8    [HALO]  own region of the halo pixel, 0xFF outside the image
constexpr int TBL_GRP = TBL_LAB + (HALO + 7) / 8 * 8;           // u8    [BM]    region of the output pixel
constexpr int TBL_MISC = TBL_GRP + BM;                          // int   [4]
constexpr int TBL_BYTES = TBL_MISC + 16;
static_assert(TBL_VAR - TBL_BASE == 656 && TBL_GRP - TBL_LAB == 328 && TBL_MISC % 4 == 0, "table block");

#ifdef __HIPCC__

struct TileTables {
    int* out;
    float* nz;
    unsigned* need;
    unsigned short* base;
    unsigned short* var;
    unsigned char* lab;
    unsigned char* grp;
    int* misc;
};

__device__ __forceinline__ TileTables tile_tables(unsigned char* t) {
    return TileTables{reinterpret_cast<int*>(t + TBL_OUT), reinterpret_cast<float*>(t + TBL_NZ), reinterpret_cast<unsigned*>(t + TBL_NEED),
                      reinterpret_cast<unsigned short*>(t + TBL_BASE), reinterpret_cast<unsigned short*>(t + TBL_VAR), t + TBL_LAB, t + TBL_GRP,
                      reinterpret_cast<int*>(t + TBL_MISC)};
}

// logical block id (after the XCD remap and any K split) -> row tile mt = (class, image, tile row, tile column), column tile nt
struct Tile {
    int mt, nt, cls, tb, tyb, txb, py, px;
};
__device__ __forceinline__ Tile decode_tile(const e4s_conv_params& p, const int logical, const int ntn, const int tx_n, const int per_img,
                                            const int tiles_per_cls) {
    Tile t;
    t.mt = logical / ntn;
    t.nt = logical - t.mt * ntn;
    t.cls = t.mt / tiles_per_cls;
    const int tt = t.mt - t.cls * tiles_per_cls;
    t.tb = tt / per_img;
    const int rem = tt - t.tb * per_img;
    t.tyb = rem / tx_n;
    t.txb = rem - t.tyb * tx_n;
    t.py = (p.ncls == 4) ? (t.cls >> 1) : 0;
    t.px = (p.ncls == 4) ? (t.cls & 1) : 0;
    return t;
}

// legacy-nearest label of an OUTPUT pixel of image tb (F.interpolate 'nearest', model.py:391)
__device__ __forceinline__ int label_at(const e4s_conv_params& p, const int tb, const int oy, const int ox) {
    return p.labels[((size_t)tb * p.Hm + nearest_src(oy, p.Hm, p.Ho)) * p.Wm + nearest_src(ox, p.Wm, p.Wo)];
}

// a = x * s as hi + lo bf16: hi = rne(x s) (packed convert, re-expanded with a shift / a mask), lo = rne(fma(x, s, -hi))
__device__ __forceinline__ void scale_split_store(unsigned char* dst, unsigned char* dst_lo, const f32x8 x, const f32x8 s) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 hp;
    f32x8 res;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x2 xs = f32x2{x[2 * j], x[2 * j + 1]}, ss = f32x2{s[2 * j], s[2 * j + 1]};
        const f32x2 v = xs * ss;
        const unsigned h2 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
        hp[j] = h2;
        const f32x2 hf = f32x2{__builtin_bit_cast(float, h2 << 16), __builtin_bit_cast(float, h2 & 0xffff0000u)};
        f32x2 r;
        asm("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(r) : "v"(xs), "v"(ss), "v"(hf));
        res[2 * j] = r[0];
        res[2 * j + 1] = r[1];
    }
    *reinterpret_cast<u32x4*>(dst) = hp;
    *reinterpret_cast<bf16x8*>(dst_lo) = __builtin_convertvector(res, bf16x8);
}

// Analysis steps 2 and 3 and the variant list, for a block of NTHR threads whose step 1 has filled out / nz / grp / lab and zeroed need
// (barrier included).  Writes the tile's overflow flag where write_flag says so; false: the tile needs more than VMAX variant rows and
// the block leaves it to the region-select kernel.
template <int NTHR>
__device__ __forceinline__ bool variant_rows(const TileTables T, const int tid, const bool write_flag, int* flag, int& nvar) {
    static_assert(NTHR >= BM && NTHR % 64 == 0, "one thread per output pixel");
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // ---- 2: which foreign regions read each halo pixel ----
    if (tid < BM && T.out[tid] >= 0) {
        const int my = tid / TW, mx = tid % TW;
        const unsigned r = T.grp[tid];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int h = (my + tap / 3) * HALO_W + mx + tap % 3;
            const unsigned lab = T.lab[h];
            if (lab != 0xFFu && lab != r) atomicOr(&T.need[h], 1u << r);
        }
    }
    __syncthreads();
    // ---- 3: variant rows of halo pixel h start at HALO + base[h] (exclusive scan of the popcounts, one wave) ----
    if (wave == 0) {
        int cnt[6], tot = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int h = lane * 6 + k;
            cnt[k] = h < HALO ? __popc(T.need[h]) : 0;
            tot += cnt[k];
        }
        int inc = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        int ex = inc - tot;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int h = lane * 6 + k;
            if (h < HALO) T.base[h] = (unsigned short)min(ex, 65535);
            ex += cnt[k];
        }
        if (lane == 63) T.misc[0] = inc;
    }
    __syncthreads();
    nvar = T.misc[0];
    const bool overflow = nvar > VMAX;
    if (write_flag) *flag = overflow ? 1 : 0;
    if (overflow) return false;
    for (int h = tid; h < HALO; h += NTHR) {
        unsigned bits = T.need[h];
        int idx = T.base[h];
        while (bits) {
            const int r = __ffs(bits) - 1;
            T.var[idx++] = (unsigned short)((h << 4) | r);
            bits &= bits - 1;
        }
    }
    __syncthreads();
    return true;
}

// ---- 4: byte offset (k-half kh) of the LDS row that output pixel m of the tile reads through tap: the halo pixel's own row, or its
// variant row for m's region where the two regions differ ----
__device__ __forceinline__ int tap_row(const TileTables T, const int m, const int tap, const int kh) {
    const int my = m / TW, mx = m % TW;
    const unsigned r = T.grp[m];
    const bool valid = T.out[m] >= 0;
    const int h = (my + tap / 3) * HALO_W + mx + tap % 3;
    const unsigned lab = T.lab[h];
    int row = halo_row(h);
    if (valid && lab != 0xFFu && lab != r) row = var_row(T.base[h] + __popc(T.need[h] & ((1u << r) - 1u)));
    return swz(row, kh);
}

// staging item i of a thread of an NTHR-thread block: LDS row j = (tid + NTHR i) / 2 of a chunk (halo rows, then the tile's nvar variant
// rows), 8-channel half q.  src / sty: offsets (floats, chunk 0) of its x and of its style, dst: its offset in a row buffer, -1 where there
// is no such row.  Rows outside the image are zeroed here, once, in both buffers of sA.
struct StageItem {
    int src, sty, dst;
};
template <int NTHR>
__device__ __forceinline__ StageItem staging_item(const e4s_conv_params& p, const TileTables T, const Tile& tile, const int tid, const int i,
                                                  const int nvar, unsigned char* sA) {
    const int e = tid + NTHR * i, j = e >> 1, q = e & 1;
    int h = -1;
    unsigned r = 0xFFu;
    if (j < HALO) {
        h = j;
        r = T.lab[h];
    } else if (j < HALO + nvar) {
        const unsigned v = T.var[j - HALO];
        h = v >> 4;
        r = v & 15u;
    }
    StageItem it = {0, 0, -1};
    if (h >= 0) {
        const int lrow = j < HALO ? halo_row(j) : var_row(j - HALO);
        if (r == 0xFFu) {                          // outside the image: zero rows, written once
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2) {
                *reinterpret_cast<f32x4*>(sA + b2 * A_BYTES + swz(lrow, q)) = z;
                *reinterpret_cast<f32x4*>(sA + b2 * A_BYTES + (swz(lrow, q) ^ 32)) = z;
            }
        } else {
            const int hy = h / HALO_W, hx = h - hy * HALO_W;
            const int iy = tile.tyb * TH + hy - 1, ix = tile.txb * TW + hx - 1;
            it.src = (iy * p.Wi + ix) * p.Cin + q * 8;
            it.sty = (int)r * p.Cin + q * 8;
            it.dst = swz(lrow, q);
        }
    }
    return it;
}

#endif  // __HIPCC__

}  // namespace region_rows
