"""ctypes binding of libe4s_hip.so (include/e4s_hip.h).

This is the thin host-side shim a maintainer of the reference would add in place of
``torch.utils.cpp_extension.load(...)`` (src/models/stylegan2/op/fused_act.py:8-15,
upfirdn2d.py:7-14): PyTorch supplies device memory (``Tensor.data_ptr()``) and the current HIP
stream; the library gets raw pointers and sizes.  There is NO fallback: if the shared object is
missing, or a tensor is not a contiguous fp32 tensor on a ROCm device, we raise.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("E4S_LIB_PATH") or os.path.join(_HERE, "libe4s_hip.so")      # (E4S_LIB_PATH: A/B runs of two builds)
ABI_VERSION = 30

c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_l = ctypes.c_int64
c_f = ctypes.c_float
c_d = ctypes.c_double


STYLE_GRAD_MAX_JOBS = 32


class StyleGradJob(ctypes.Structure):
    """Mirror of ``e4s_style_grad_job`` (include/e4s_hip.h)."""
    _fields_ = [
        ("ds_raw", c_p), ("dd_d", c_p), ("d", c_p), ("s", c_p), ("wsq", c_p), ("dws", c_p), ("w3", c_p), ("wmod", c_p), ("ds_total", c_p),
        ("conv_scale", c_f), ("mod_scale", c_f), ("G", c_i), ("Cin", c_i), ("Cout", c_i), ("slot", c_i), ("masked", c_i),
    ]


class ConvParams(ctypes.Structure):
    """Mirror of ``e4s_conv_params`` (include/e4s_hip.h)."""
    _fields_ = [
        ("x", c_p), ("w", c_p), ("y", c_p), ("rows", c_p), ("tiles", c_p), ("meta", c_p), ("tiles_cap", c_i),
        ("B", c_i), ("Ha", c_i), ("Wa", c_i),
        ("Hi", c_i), ("Wi", c_i), ("Ho", c_i), ("Wo", c_i), ("Cin", c_i), ("Cout", c_i),
        ("istride", c_i), ("ostride", c_i), ("ntaps", c_i), ("ncls", c_i),
        ("in_scale", c_p), ("out_scale", c_p), ("groups_per_batch", c_i),
        ("labels", c_p), ("Hm", c_i), ("Wm", c_i),
        ("noise", c_p), ("noise_w", c_p), ("noise_bstride", c_l), ("noise_per_channel", c_i),
        ("bias", c_p), ("slope", c_p), ("act", c_i), ("alpha", c_f), ("gain", c_f),
        ("in_stats", c_p), ("y_cstride", c_i), ("splitk_ws", c_p), ("stats_ws", c_p), ("stats_slots", c_i), ("tap_shift", c_i),
        ("split_hint", c_i), ("w_frag", c_p),
    ]


class ConvBwdParams(ctypes.Structure):
    """Mirror of ``e4s_conv_bwd_params`` (include/e4s_hip.h)."""
    _fields_ = [
        ("gz", c_p), ("wt", c_p), ("dx", c_p), ("x", c_p), ("ds", c_p), ("s", c_p), ("d", c_p), ("labels", c_p),
        ("Hm", c_i), ("Wm", c_i), ("R", c_i),
        ("B", c_i), ("Hx", c_i), ("Wx", c_i), ("Cx", c_i), ("Hy", c_i), ("Wy", c_i), ("Cy", c_i),
        ("ncls", c_i), ("ds_ws", c_p),
    ]


class ConvWgradParams(ctypes.Structure):
    """Mirror of ``e4s_conv_wgrad_params`` (include/e4s_hip.h)."""
    _fields_ = [
        ("gz", c_p), ("x", c_p), ("dw", c_p), ("ws", c_p), ("s", c_p), ("d", c_p), ("labels", c_p),
        ("Hm", c_i), ("Wm", c_i), ("R", c_i),
        ("B", c_i), ("Hi", c_i), ("Wi", c_i), ("Cin", c_i), ("Ha", c_i), ("Wa", c_i), ("Ho", c_i), ("Wo", c_i), ("Cout", c_i),
        ("istride", c_i), ("ostride", c_i), ("py", c_i), ("px", c_i), ("ntaps", c_i), ("tap_shift", c_i),
    ]


class RrdbParams(ctypes.Structure):
    """Mirror of ``e4s_rrdb_params`` (include/e4s_hip.h)."""
    _fields_ = [
        ("x", c_p), ("w", c_p), ("bias", c_p), ("y", c_p), ("r0", c_p), ("r1", c_p),
        ("B", c_i), ("Hi", c_i), ("Wi", c_i), ("Cin", c_i),
        ("x_cstride", c_i), ("y_cstride", c_i), ("y_coff", c_i),
        ("r0_cstride", c_i), ("r0_coff", c_i), ("r1_cstride", c_i), ("r1_coff", c_i),
        ("epilogue", c_i), ("up2", c_i), ("precision", c_i),
        ("s0", c_f), ("s1", c_f), ("slope", c_f),
    ]


class PconvParams(ctypes.Structure):
    """Mirror of ``e4s_pconv_params`` (include/e4s_hip.h)."""
    _fields_ = [
        ("x", c_p), ("w", c_p), ("scale", c_p), ("bias", c_p), ("r0", c_p), ("r1", c_p), ("y", c_p),
        ("B", c_i), ("Hi", c_i), ("Wi", c_i), ("Cin", c_i), ("Cout", c_i),
        ("x_cstride", c_i), ("y_cstride", c_i), ("r0_cstride", c_i), ("r1_cstride", c_i),
        ("stride", c_i), ("up2", c_i), ("lrelu", c_i), ("precision", c_i),
        ("slope", c_f),
    ]


class RconvParams(ctypes.Structure):
    """Mirror of ``e4s_rconv_params`` (include/e4s_hip.h)."""
    _fields_ = [
        ("x", c_p), ("w", c_p), ("bias", c_p), ("r0", c_p), ("y", c_p),
        ("B", c_i), ("Hi", c_i), ("Wi", c_i), ("Cin", c_i), ("Cout", c_i),
        ("x_cstride", c_i), ("y_cstride", c_i), ("y_coff", c_i), ("r0_cstride", c_i),
        ("r0_H", c_i), ("r0_W", c_i),
        ("k", c_i), ("stride", c_i), ("act", c_i), ("r0_mode", c_i), ("precision", c_i),
        ("slope", c_f),
    ]


class RetinaGeom(ctypes.Structure):
    """Mirror of ``e4s_retina_geom`` (include/e4s_hip.h)."""
    _fields_ = [
        ("imH", c_i), ("imW", c_i), ("nlevel", c_i), ("N", c_i),
        ("lh", c_i * 3), ("lw", c_i * 3), ("step", c_i * 3), ("base", c_i * 3),
        ("min_size", (c_f * 2) * 3),
        ("resize", c_f),
    ]


class Conv3dParams(ctypes.Structure):
    """Mirror of ``e4s_conv3d_params`` (include/e4s_hip.h)."""
    _fields_ = [
        ("x", c_p), ("w", c_p), ("bias", c_p), ("y", c_p),
        ("x_bstride", c_l), ("x_dstride", c_l), ("x_ystride", c_l), ("x_xstride", c_l),
        ("B", c_i), ("D", c_i), ("Hi", c_i), ("Wi", c_i), ("Cin", c_i), ("Cout", c_i),
        ("y_cstride", c_i),
        ("up2", c_i), ("relu", c_i), ("precision", c_i),
    ]


class Conv3dxParams(ctypes.Structure):
    """Mirror of ``e4s_conv3dx_params`` (include/e4s_hip.h)."""
    _fields_ = [
        ("x", c_p), ("w", c_p), ("bias", c_p), ("res", c_p), ("y", c_p),
        ("x_bstride", c_l), ("x_dstride", c_l), ("x_ystride", c_l), ("x_xstride", c_l),
        ("r_bstride", c_l), ("r_dstride", c_l), ("r_ystride", c_l), ("r_xstride", c_l),
        ("B", c_i), ("D", c_i), ("Hi", c_i), ("Wi", c_i), ("Cin", c_i), ("Cout", c_i),
        ("y_cstride", c_i),
        ("ksize", c_i),
        ("up2", c_i), ("relu", c_i), ("precision", c_i),
    ]


class PoseParams(ctypes.Structure):
    """Mirror of ``e4s_pose_params`` (include/e4s_hip.h)."""
    _fields_ = [
        ("x", c_p), ("w", c_p), ("bias", c_p), ("kp_value", c_p), ("kp_jacobian", c_p),
        ("raw", c_p), ("degrees", c_p), ("rot", c_p), ("value", c_p), ("jacobian", c_p),
        ("B", c_i), ("HW", c_i), ("C", c_i), ("x_cstride", c_i), ("nbins", c_i), ("K", c_i), ("kp_batch", c_i), ("fixed_mask", c_i),
        ("yaw", c_f), ("pitch", c_f), ("roll", c_f),
    ]


class SpadeSharedParams(ctypes.Structure):
    """Mirror of ``e4s_spade_shared_params`` (include/e4s_hip.h)."""
    _fields_ = [
        ("seg", c_p), ("w", c_p), ("bias", c_p), ("y", c_p),
        ("B", c_i), ("Hs", c_i), ("Ws", c_i), ("Cin", c_i), ("Cout", c_i),
        ("seg_cstride", c_i), ("y_cstride", c_i), ("y_coff", c_i),
        ("shift", c_i), ("precision", c_i),
    ]


class SpadeConvParams(ctypes.Structure):
    """Mirror of ``e4s_spade_conv_params`` (include/e4s_hip.h)."""
    _fields_ = [
        ("a", c_p), ("w", c_p), ("bias", c_p), ("x", c_p), ("stats", c_p), ("y", c_p),
        ("B", c_i), ("H", c_i), ("W", c_i), ("Cin", c_i), ("C", c_i),
        ("a_cstride", c_i), ("a_coff", c_i), ("x_cstride", c_i), ("xH", c_i), ("xW", c_i), ("y_cstride", c_i), ("y_coff", c_i),
        ("xs", c_i), ("act", c_i), ("precision", c_i),
    ]


# name -> argtypes (all return int except the two info calls); keep in sync with include/e4s_hip.h
SIGNATURES = {
    "e4s_fused_bias_act_f32": [c_p, c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_i, c_f, c_f, c_p],
    "e4s_upfirdn2d_f32": [c_p, c_p, c_p] + [c_i] * 14 + [c_p],
    "e4s_channel_sum_f32": [c_p, c_p, c_l, c_i, c_i, c_p],
    "e4s_rowdot_f32": [c_p, c_l, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p],
    "e4s_weight_sqsum_f32": [c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_pack_taps_f32": [c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_polyphase_weights_f32": [c_p, c_p, c_p, c_i, c_i, c_p],
    "e4s_polyphase_fold_f32": [c_p, c_p, c_p, c_i, c_i, c_p],
    "e4s_rgb_weights_f32": [c_p, c_p, c_p, c_i, c_i, c_f, c_p],
    "e4s_mask_labels": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_region_plan": [c_p] + [c_i] * 8 + [c_p, c_p, c_p, c_p, c_i, c_i, c_p],
    "e4s_conv_mfma_f32": [ctypes.POINTER(ConvParams), c_i, c_p],
    "e4s_upconv_mfma_f32": [ctypes.POINTER(ConvParams), c_p, c_p],
    "e4s_conv_bf16x3_f32": [ctypes.POINTER(ConvParams), c_p],
    "e4s_conv_bf16x3_ws_floats": [ctypes.POINTER(ConvParams)],
    "e4s_conv_mfma_ws_floats": [ctypes.POINTER(ConvParams), c_i],
    "e4s_gather_ksplit": [c_l, c_i, c_i],
    "e4s_split_bf16x2_f32": [c_p, c_p, c_l, c_i, c_p],
    "e4s_conv_region_bf16x3_f32": [ctypes.POINTER(ConvParams), c_p, c_p],
    "e4s_conv_region_ws_floats": [ctypes.POINTER(ConvParams)],
    "e4s_conv_region_path": [ctypes.POINTER(ConvParams)],
    "e4s_conv_gather_path": [ctypes.POINTER(ConvParams)],
    "e4s_split16_bytes": [ctypes.c_int64, c_i, c_i],
    "e4s_gather_frag_bytes": [c_i, c_i, c_i],
    "e4s_gather_frag_bf16x2_f32": [c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_split16_bf16x2_f32": [c_p, c_p, c_l, c_i, c_i, c_p],
    "e4s_upconv_blocks_per_cu": [],
    "e4s_instnorm_ws_doubles": [c_i, c_i, c_i],
    "e4s_conv_bwd_mfma_f32": [ctypes.POINTER(ConvBwdParams), c_p],
    "e4s_pack_taps_bwd_f32": [c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_demod_grad_f32": [c_p, c_p, c_p, c_p, c_l, c_p, c_f, c_f, c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_torgb_bwd_w_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_conv_bwd_ws_floats": [ctypes.POINTER(ConvBwdParams)],
    "e4s_seg_reduce_nsplit": [c_i, c_i, c_i, c_i],
    "e4s_grouped_linear_t_f32": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_p, c_f, c_p],
    "e4s_grouped_linear_t_ws_floats": [c_i, c_i, c_i, c_i],
    "e4s_reduce_parts_f32": [c_p, c_p, c_i, c_l, c_f, c_p],
    "e4s_reduce_parts_ws_floats": [c_i, c_l],
    "e4s_grouped_outer_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p],
    "e4s_style_grad_multi_f32": [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_swap_styles_f32": [c_p, c_p, c_p, c_i, c_i, c_i, ctypes.c_uint, c_i, c_i, c_i, c_p],
    "e4s_batch_sum_f32": [c_p, c_p, c_i, c_l, c_p],
    "e4s_adam_step_f32": [c_p, c_p, c_p, c_p, c_l, c_d, c_d, c_d, c_d, c_d, c_i, c_p],
    "e4s_subpixel_weights_f32": [c_p, c_p, c_i, c_i, c_p],
    "e4s_upconv_bf16x3_f32": [c_p, c_p, c_p],
    "e4s_colsum_f32": [c_p, c_p, c_p, c_l, c_i, c_p],
    "e4s_colsum_ws_floats": [c_l, c_i],
    "e4s_scale_dot_f32": [c_p, c_p, c_p, c_p, c_p, c_i, c_l, c_i, c_p],
    "e4s_scale_dot_ws_floats": [c_i, c_l, c_i],
    "e4s_mask_to_u8": [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_erode_u8": [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_gaussian_blur_u8": [c_p, c_p, c_i, c_i, c_i, c_i, ctypes.POINTER(c_i), c_p],
    "e4s_alpha_composite_u8": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_pyrdown_u8": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_pyrdown_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_pyrup_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_u8_to_f32": [c_p, c_p, c_l, c_p],
    "e4s_lap_level_f32": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_l, c_i, c_p],
    "e4s_clip_u8": [c_p, c_p, c_l, c_p],
    "e4s_conv_c32_bf16x3_f32": [c_p, c_p, c_p, c_p],
    "e4s_torgb_finish_f32": [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_rowdot_multi_f32": [c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_ema_f32": [c_p, c_p, c_l, c_d, c_p],
    "e4s_adam_step_dev_f32": [c_p, c_p, c_p, c_p, c_l, c_d, c_p, c_d, c_d, c_d, c_d, c_p, c_p],
    "e4s_advance_i64": [c_p, c_l, c_p],
    "e4s_conv_smallcin_col2im_f32": [c_p, c_p] + [c_i] * 10 + [c_p],
    "e4s_region_scale_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_col2im_region_nsplit": [c_i, c_i, c_i, c_i],
    "e4s_col2im_region_f32": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_act_bwd_demod_nsplit": [c_i, c_i, c_i, c_i],
    "e4s_act_bwd_demod_f32": [c_p, c_p, c_p, c_p, c_p, c_l, c_p, c_f, c_f, c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_pixel_unshuffle2_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_wino_weights_bytes": [c_i, c_i],
    "e4s_wino_weights_f32": [c_p, c_p, c_i, c_i, c_p],
    "e4s_conv_wino_covers": [c_p],
    "e4s_conv_wino_ws_floats": [c_p],
    "e4s_conv_wino_bf16x3_f32": [c_p, c_p],
    "e4s_adam_multi_dev_f32": [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_d, c_p, c_d, c_d, c_d, c_d, c_p],
    "e4s_ema_multi_f32": [c_i, c_p, c_p, c_p, c_d, c_p],
    "e4s_ranger_multi_ws_floats": [c_i, c_p, c_p],
    "e4s_ranger_multi_dev_f32": [c_i] + [c_p] * 9 + [c_l, c_d, c_p, c_d, c_d, c_d, c_d, c_d, c_i, c_d, c_p],
    "e4s_torgb_bwd_x_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_shift_scale_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_p] + [c_i] * 12 + [c_p],
    "e4s_torgb_f32": [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_mask_mul_add_f32": [c_p, c_p, c_p] + [c_i] * 10 + [c_p],
    "e4s_noise_bias_act_nhwc_f32": [c_p, c_p, c_p, c_l, c_p, c_p, c_i, c_i, c_i, c_f, c_f, c_p],
    "e4s_nchw_to_nhwc_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_nhwc_to_nchw_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_const_input_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_resize_bilinear_f32": [c_p, c_p] + [c_i] * 6 + [c_p],
    "e4s_conv3x3_small_f32": [c_p, c_p, c_p] + [c_i] * 5 + [c_p],
    "e4s_conv3x3_stem_f32": [c_p, c_p, c_p, c_p] + [c_i] * 5 + [c_p],
    "e4s_instnorm_stats_f32": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_p],
    "e4s_instnorm_finalize_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p],
    "e4s_instnorm_apply_stats_f32": [c_p] * 9 + [c_i] * 5 + [c_p],
    "e4s_instnorm_apply_f32": [c_p] * 7 + [c_i] * 5 + [c_p],
    "e4s_se_gate_f32": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_instnorm_finalize_se_f32": [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p],
    "e4s_region_mean_f32": [c_p, c_p, c_i, c_i, c_p, c_p] + [c_i] * 7 + [c_p],
    "e4s_region_mean_ws_floats": [c_i, c_i, c_i, c_i],
    "e4s_conv_wgrad_f32": [ctypes.POINTER(ConvWgradParams), c_p],
    "e4s_conv_wgrad_ws_floats": [ctypes.POINTER(ConvWgradParams)],
    "e4s_conv_wgrad_path": [ctypes.POINTER(ConvWgradParams)],
    "e4s_instnorm_bwd_f32": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_instnorm_bwd_ws_doubles": [c_i, c_i, c_i],
    "e4s_prelu_f32": [c_p, c_p, c_p, c_l, c_i, c_p],
    "e4s_prelu_bwd_f32": [c_p, c_p, c_p, c_p, c_p, c_p, c_l, c_i, c_p],
    "e4s_prelu_bwd_ws_floats": [c_l, c_i],
    "e4s_strided_scatter_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_strided_place_f32": [c_p, c_p] + [c_i] * 9 + [c_p],
    "e4s_region_mean_bwd_f32": [c_p, c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_conv1x1_small_f32": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_f, c_p],
    "e4s_noise_half_f32": [c_p, c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_f, c_f, c_p],
    "e4s_pixelnorm_f32": [c_p, c_p, c_i, c_i, c_p],
    "e4s_add_scale_f32": [c_p, c_p, c_p, c_f, c_l, c_p],
    "e4s_minibatch_stddev_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_onehot_u8_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_swap_head_mask_u8": [c_p, c_p, c_p, c_p, c_l, c_p],
    "e4s_foreground_mask_f32": [c_p, c_p, c_p, c_l, c_p],
    "e4s_morph_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_create_masks_f32": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_tensor2im_u8": [c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_stream_copy_u8": [c_p, c_p, ctypes.c_int64, c_i, c_p],
    "e4s_paste_u8": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_grouped_linear_f32": [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_p],
    "e4s_adaptive_pool_f32": [c_p, c_p] + [c_i] * 11 + [c_p, c_p, c_p],
    "e4s_adaptive_pool_bwd_f32": [c_p, c_p] + [c_i] * 11 + [c_p, c_i, c_p],
    "e4s_conv_smallcin_f32": [c_p, c_p, c_p, c_p] + [c_i] * 11 + [c_p],
    "e4s_conv_smallcin_bwd_f32": [c_p, c_p, c_p] + [c_i] * 10 + [c_p],
    "e4s_maxpool3s2_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_maxpool3s2_bwd_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_maxpool2_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_maxpool2_bwd_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_relu_bwd_f32": [c_p, c_p, c_p, c_l, c_i, c_p],
    "e4s_lpips_layer_f32": [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_lpips_layer_ws_doubles": [c_i, c_i],
    "e4s_lpips_layer_bwd_f32": [c_p, c_p, c_p, c_p, c_f, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_instnorm_bwd_sums_f32": [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_norm_bwd_frozen_f32": [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_cosine_f32": [c_p, c_p, c_p, c_p, c_i, c_l, c_p],
    "e4s_cosine_ws_doubles": [c_i, c_l],
    "e4s_cosine_bwd_f32": [c_p, c_p, c_p, c_p, c_f, c_p, c_i, c_l, c_i, c_p],
    "e4s_style_prep_f32": [c_p, c_p, c_p] + [c_i] * 8 + [c_p],
    "e4s_style_prep_bwd_f32": [c_p, c_p, c_p] + [c_i] * 8 + [c_p],
    "e4s_gram_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_gram_ws_floats": [c_i, c_i, c_i],
    "e4s_gram_mse_f32": [c_p, c_p, c_p, c_p, c_p, c_f, c_i, c_p, c_l, c_p],
    "e4s_gram_mse_ws_doubles": [c_l],
    "e4s_gram_grad_f32": [c_p, c_p, c_p, c_f, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_parser_preprocess_f32": [c_p, c_i, c_p, c_i, c_i, c_i, ctypes.POINTER(c_f), c_p],
    "e4s_maxpool3s2p1_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_add_relu_f32": [c_p, c_p, c_p, c_l, c_i, c_i, c_i, c_p],
    "e4s_mean_hw_f32": [c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_parser_fc_f32": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p],
    "e4s_gate_add_up2_f32": [c_p, c_p, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_parser_head_f32": [c_p] + [c_i] * 8 + [c_p, c_p, c_p, c_p],
    "e4s_quad_crop_u8": [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_perspective_paste_u8": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_rrdb_conv_f32": [ctypes.POINTER(RrdbParams), c_p],
    "e4s_rrdb_pack_f32": [c_p, c_p, c_i, c_i, c_p],
    "e4s_rrdb_pack_bytes": [c_i],
    "e4s_rrdb_head_f32": [c_p, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_rrdb_tail_f32": [c_p, c_i, c_p, c_p, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_pconv_f32": [ctypes.POINTER(PconvParams), c_p],
    "e4s_pconv_pack_f32": [c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_pconv_pack_bytes": [c_i, c_i],
    "e4s_parsenet_head_f32": [c_p, c_i, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_parsenet_tail_f32": [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_warp_affine": [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_d, c_d, c_d, c_d, c_d, c_d, c_p],
    "e4s_mask_prep_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_blur_pass_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_binomial3_u8": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_merge_blend_u8": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_rconv_f32": [ctypes.POINTER(RconvParams), c_p],
    "e4s_rconv_pack_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_rconv_pack_bytes": [c_i, c_i, c_i],
    "e4s_retina_prep_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_d, c_p],
    "e4s_retina_head_f32": [c_p, c_i, c_p, c_p, ctypes.POINTER(RetinaGeom), c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p],
    "e4s_retina_decode_f32": [c_p, c_p, c_p, ctypes.POINTER(RetinaGeom), c_i, c_p, c_p, c_p, c_p],
    "e4s_retina_select_f32": [c_p, c_p, c_p, c_p, c_i, c_i, c_f, c_f, c_i, c_i, c_f, c_p, c_p, c_p, c_p],
    "e4s_conv3d_f32": [ctypes.POINTER(Conv3dParams), c_p],
    "e4s_conv3d_pack_f32": [c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_conv3d_pack_bytes": [c_i, c_i],
    "e4s_softargmax3d_f32": [c_p, c_l, c_l, c_l, c_p, c_l, c_l, c_l] + [c_i] * 6 + [c_f, c_p, c_p, c_p],
    "e4s_aa_down_f32": [c_p, c_i, c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_p],
    "e4s_avgpool2_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_pose_f32": [ctypes.POINTER(PoseParams), c_p],
    "e4s_conv3dx_f32": [ctypes.POINTER(Conv3dxParams), c_p],
    "e4s_conv3dx_pack_f32": [c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "e4s_conv3dx_pack_bytes": [c_i, c_i, c_i],
    "e4s_avgpool2s_f32": [c_p, c_p] + [c_i] * 6 + [c_p],
    "e4s_bnrelu3d_f32": [c_p, c_l, c_l, c_l, c_l, c_p, c_p, c_p] + [c_i] * 5 + [c_p],
    "e4s_kp_jacobian_f32": [c_p, c_i, c_p, c_p, c_i, c_i, c_p],
    "e4s_sparse_warp_f32": [c_p, c_i, c_p, c_i, c_p, c_p, c_p] + [c_i] * 7 + [c_f, c_p],
    "e4s_motion_combine_f32": [c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_p] + [c_i] * 5 + [c_p],
    "e4s_warp3d_f32": [c_p, c_l, c_l, c_l, c_p, c_p] + [c_i] * 5 + [c_p],
    "e4s_occlusion_f32": [c_p, c_i, c_p, c_p, c_p] + [c_i] * 6 + [c_p],
    "e4s_scale_rows_f32": [c_p, c_p, c_l, c_i, c_p],
    "e4s_spade_shared_f32": [ctypes.POINTER(SpadeSharedParams), c_p],
    "e4s_spade_conv_f32": [ctypes.POINTER(SpadeConvParams), c_p],
    "e4s_spade_tail_f32": [c_p, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_resize_aa4_u8_f32": [c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_driven_seam_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_face_to_net_u8": [c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_p],
    "e4s_texture_mix_f32": [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "e4s_labels_to_color_u8": [c_p, c_p, c_l, c_p],
    "e4s_color_to_labels_u8": [c_p, c_p, c_l, c_p],
    "e4s_mask_brush_u8": [c_p, c_p, c_p, c_l, c_i, c_i, c_p],
    "e4s_pil_resample_h_u8": [c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_l, c_l, c_i, c_i, c_i, c_p],
    "e4s_pil_resample_v_u8": [c_p, c_l, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_p],
}

INT64_RETURN = {"e4s_split16_bytes", "e4s_gather_frag_bytes", "e4s_instnorm_ws_doubles", "e4s_conv_bwd_ws_floats", "e4s_grouped_linear_t_ws_floats", "e4s_reduce_parts_ws_floats", "e4s_instnorm_bwd_ws_doubles", "e4s_prelu_bwd_ws_floats", "e4s_conv_wgrad_ws_floats", "e4s_conv_bf16x3_ws_floats", "e4s_conv_region_ws_floats", "e4s_lpips_layer_ws_doubles", "e4s_conv_mfma_ws_floats",
                "e4s_cosine_ws_doubles", "e4s_region_mean_ws_floats", "e4s_colsum_ws_floats", "e4s_scale_dot_ws_floats", "e4s_wino_weights_bytes", "e4s_conv_wino_ws_floats", "e4s_rrdb_pack_bytes", "e4s_pconv_pack_bytes", "e4s_rconv_pack_bytes",
                "e4s_ranger_multi_ws_floats", "e4s_conv3d_pack_bytes", "e4s_conv3dx_pack_bytes", "e4s_gram_ws_floats", "e4s_gram_mse_ws_doubles"}       # size queries: return a count, not an error code

_lib = None


def load():
    """dlopen libe4s_hip.so (built in-tree by e4s_amd.build / __graft_entry__.build). Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: run `python -m e4s_amd.build` (hipcc, gfx950). "
                           "e4s_amd has no CPU / eager fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.e4s_abi_version.restype = c_i
    lib.e4s_build_arch.restype = ctypes.c_char_p
    if lib.e4s_abi_version() != ABI_VERSION:
        raise RuntimeError("libe4s_hip.so ABI version mismatch: rebuild with `python -m e4s_amd.build --force`")
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = c_l if name in INT64_RETURN else c_i
    _lib = lib
    return lib


def stream():
    return c_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a contiguous fp32/uint8/int32/f64 ROCm tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("e4s_amd kernels need tensors on a ROCm device (no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError("e4s_amd kernels need contiguous tensors")
    return c_p(t.data_ptr())


def fptr(t):
    if t is not None and t.dtype != torch.float32:
        raise RuntimeError(f"expected float32, got {t.dtype}")
    return ptr(t)


def check(code, what):
    if code != 0:
        raise RuntimeError(f"{what} failed: hipError {code}")


def call(name, *args):
    check(getattr(load(), name)(*args), name)
