// Host side of the split-bf16 conv family that crosses translation units: the launch plans and the launchers one file calls in another.
// A plan is what ONE function per family decides about a launch; the workspace query, the path query and the launcher all read it, so a
// query cannot disagree with its launcher.  K-split rules: split_policy.h.
#pragma once
#include "common.h"
#include "split_policy.h"

// masked StyledConv (conv_region.hip: e4s_plan_masked)
struct e4s_masked_plan {
    int path;                  // 1: 8-wave variant-rows kernel, 2: one wave per SIMD, 3: packed small-map tiles of the region-select kernel
    int ksplit, cper;          // K split in 32-channel chunks (path 2 never splits)
    int64_t slab_floats;       // split-K slabs at the head of p.splitk_ws (0: no split)
    int64_t flag_ints;         // tile-flag table behind them (variant-rows entry point only)
};
// plain persistent kernel (conv_bf16x3.hip)
enum e4s_plain_config { E4S_PLAIN_L16, E4S_PLAIN_L, E4S_PLAIN_M, E4S_PLAIN_S, E4S_PLAIN_SHUF };
struct e4s_plain_plan {
    int config;                // column tile 128 (16- or 32-channel stages) / 64 / 32, or the polyphase up-conv's 4 Cout-column GEMM
    int ntn, ksplit, cper;     // column tiles; K split in 32-channel chunks
    int64_t slab_floats;
};
// strided gather kernel (conv_bf16x3.hip)
struct e4s_gather_plan {
    int ntn, ksplit, cper;
    int64_t npix, ntile, slab_floats;
};
// Winograd F(2,3) kernels (conv_wino.hip)
struct e4s_wino_plan {
    int ntn, tx_n, per_img, ksplit, cper;        // K split in 16-channel chunks
    int64_t slab_floats;
};

e4s_masked_plan e4s_plan_masked(const e4s_conv_params& p);                                             // conv_region.hip
bool e4s_region_packed(const e4s_conv_params& p);                                                      // conv_bf16x3.hip
int e4s_launch_region_select(const e4s_conv_params& p, const int* only_flagged, hipStream_t st);       // conv_bf16x3.hip
bool e4s_region_rows1w_ok(const e4s_conv_params& p);                                                   // conv_region1w.hip
int e4s_launch_region_rows1w(const e4s_conv_params& p, const void* w16, int* flags, hipStream_t st, int layout);
bool e4s_gather1w_ok(const e4s_conv_params& p);                                                        // conv_gather1w.hip
int e4s_launch_gather1w(const e4s_conv_params& p, const e4s_gather_plan& g, hipStream_t st);           // (K split: the caller runs the second stage)
int e4s_launch_wino1w(const e4s_conv_params& p, int ntn, int tx_n, int per_img, int ntiles, int grid, hipStream_t st);      // conv_wino1w.hip
// second stage of every split-K launch (conv_bf16x3.hip): slabs p.splitk_ws[k] are added in order, then noise / bias / activation;
// slabs_need_out_scale: the slabs are raw sums (the plain kernel's), not yet multiplied by p.out_scale
int e4s_splitk_epilogue(const e4s_conv_params& p, int ksplit, bool slabs_need_out_scale, hipStream_t st);
// per-channel noise (the editor's maps, NHWC [Bn][Ho][Wo][Cout]): every epilogue reads it 16 bytes at a time beside its output store
inline bool e4s_noise_pc(const e4s_conv_params& p) { return p.noise != nullptr && p.noise_per_channel != 0; }
inline bool e4s_noise_pc_ok(const e4s_conv_params& p) {
    return p.noise_w && aligned16(p.noise) && p.Cout % 4 == 0 && (p.noise_bstride == 0 || p.noise_bstride == (int64_t)p.Ho * p.Wo);
}
int e4s_num_cus();             // CUs of the current device (256 if it cannot be asked): the grid of the persistent kernels (conv_bf16x3.hip)
