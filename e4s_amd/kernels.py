"""Tensor-level wrappers over the C-ABI of libe4s_hip.so.

Each function allocates its outputs with torch (device memory + caching allocator are the
plumbing PyTorch provides) and enqueues one native call on the current HIP stream.  No function
here computes anything in torch; a missing library or a CPU tensor raises.
"""
import contextlib
import ctypes
import math
import os
import threading

import torch

from . import lib
from .lib import ConvBwdParams, ConvParams, ConvWgradParams, c_p, call, fptr, ptr, stream

BM = 128          # GEMM row tile of e4s_conv_mfma_f32
# Arithmetic of the contractions that have a split-bf16 kernel (the encoder's stride-1 3x3 convs):
#   "f32"    exact fp32 MFMA everywhere (v_mfma_f32_32x32x2_f32)
#   "bf16x3" three bf16 MFMAs per product on hi/lo-split fp32 operands, fp32 accumulate (~2^-16 per product; measured
#            1.6e-4 max-abs on the 1024^2 image against the reference, bound 1e-3), wherever the kernel applies
#   "auto"   (default) bf16x3 where it applies AND the launch fills the chip (its 256x128 tiles need >= BF16X3_MIN_BLOCKS
#            blocks to beat the fp32 kernel's 128-row tiles: batch-1 latency runs stay on fp32)
PRECISION = os.environ.get("E4S_PRECISION", "auto")
if PRECISION not in ("f32", "bf16x3", "auto"):
    raise RuntimeError(f"E4S_PRECISION must be f32, bf16x3 or auto, got {PRECISION!r}")
BF16X3_MIN_BLOCKS = int(os.environ.get("E4S_BF16X3_MIN_BLOCKS", "128"))          # (env: policy experiments, tools/; the default is what is tested)
LRELU_GAIN = math.sqrt(2.0)


def _f32(t):
    if t.dtype != torch.float32:
        raise RuntimeError(f"expected float32 tensor, got {t.dtype}")
    return t.contiguous()


# ---- 1:1 ops ---------------------------------------------------------------------------------
def fused_bias_act(x, bias, ref, act, grad, alpha, scale):
    """fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale) -- fused_bias_act.cpp:11-21."""
    x = _f32(x)
    y = torch.empty_like(x)
    has_b = bias is not None and bias.numel() > 0
    has_r = ref is not None and ref.numel() > 0
    step_b = 1
    for d in x.shape[2:]:
        step_b *= d
    call("e4s_fused_bias_act_f32", fptr(x), fptr(_f32(bias)) if has_b else None,
         fptr(_f32(ref)) if has_r else None, fptr(y), x.numel(), step_b, bias.numel() if has_b else 1,
         int(act), int(grad), float(alpha), float(scale), stream())
    return y


def channel_sum(g):
    """sum over every dim but 1 (grad_bias, op/fused_act.py:33-38)."""
    g = _f32(g)
    c = g.shape[1]
    step_b = 1
    for d in g.shape[2:]:
        step_b *= d
    out = torch.empty(c, device=g.device, dtype=torch.float32)
    call("e4s_channel_sum_f32", fptr(g), fptr(out), g.numel(), step_b, c, stream())
    return out


def upfirdn2d_raw(x, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """upfirdn2d_op.upfirdn2d(input[major,H,W,minor], kernel, ...) -- upfirdn2d.cpp:12-22."""
    x = _f32(x)
    kernel = _f32(kernel)
    major, in_h, in_w, minor = x.shape
    kh, kw = kernel.shape
    out_h = (in_h * up_y + pad_y0 + pad_y1 - kh) // down_y + 1
    out_w = (in_w * up_x + pad_x0 + pad_x1 - kw) // down_x + 1
    if out_h <= 0 or out_w <= 0:          # the kernel does not fit the padded input: nothing to compute, nothing to launch
        return torch.empty(major, max(out_h, 0), max(out_w, 0), minor, device=x.device, dtype=torch.float32)
    y = torch.empty(major, out_h, out_w, minor, device=x.device, dtype=torch.float32)
    call("e4s_upfirdn2d_f32", fptr(x), fptr(kernel), fptr(y), major, in_h, in_w, minor, kh, kw, up_x, up_y,
         down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1, stream())
    return y


# ---- layout ----------------------------------------------------------------------------------
def nchw_to_nhwc(x):
    x = _f32(x)
    b, c, h, w = x.shape
    y = torch.empty(b, h, w, c, device=x.device, dtype=torch.float32)
    call("e4s_nchw_to_nhwc_f32", fptr(x), fptr(y), b, c, h, w, stream())
    return y


def nhwc_to_nchw(x):
    x = _f32(x)
    b, h, w, c = x.shape
    y = torch.empty(b, c, h, w, device=x.device, dtype=torch.float32)
    call("e4s_nhwc_to_nchw_f32", fptr(x), fptr(y), b, c, h, w, stream())
    return y


def const_input(inp, batch):
    """ConstantInput.forward (model.py:345-349): [1,C,H,W] parameter -> NHWC [B,H,W,C]."""
    inp = _f32(inp)
    _, c, h, w = inp.shape
    y = torch.empty(batch, h, w, c, device=inp.device, dtype=torch.float32)
    call("e4s_const_input_f32", fptr(inp), fptr(y), batch, c, h, w, stream())
    return y


# ---- style prologue --------------------------------------------------------------------------
def modulate(latent, layer_idx, masked, mod_weight, mod_bias):
    """s = EqualLinear(512 -> Cin, bias_init=1)(style) for every (sample[, region]) group.
    latent [B,R,L,512] contiguous.  Returns [G, Cin] with G = B*R (masked) or B (region 0)."""
    b, r, nl, d = latent.shape
    cin = mod_weight.shape[0]
    g = b * r if masked else b
    stride = nl * d if masked else r * nl * d
    out = torch.empty(g, cin, device=latent.device, dtype=torch.float32)
    base = c_p(latent.data_ptr() + layer_idx * d * 4)
    call("e4s_rowdot_f32", base, stride, fptr(mod_weight), fptr(mod_bias), fptr(out), g, cin, d, 0,
         1.0 / math.sqrt(d), stream())
    return out


def modulate_vec(style, mod_weight, mod_bias):
    """Same for an explicit [G, 512] style matrix (module-level forward)."""
    style = _f32(style)
    g, d = style.shape
    cin = mod_weight.shape[0]
    out = torch.empty(g, cin, device=style.device, dtype=torch.float32)
    call("e4s_rowdot_f32", fptr(style), d, fptr(mod_weight), fptr(mod_bias), fptr(out), g, cin, d, 0,
         1.0 / math.sqrt(d), stream())
    return out


def rowdot_jobs(jobs, device):
    """jobs: list of dict(in_off, in_stride, out_off, M, bias, G, O, K, scale) -> (device table uint8 of e4s_rowdot_job records, njobs,
    max_O, max_G).  M / bias are tensors (kept alive by the caller: the table holds their raw pointers).  One H2D copy: build OUTSIDE
    graph capture (the generator caches the table per weight version)."""
    for j in jobs:
        if j["M"].dtype != torch.float32 or not j["M"].is_contiguous() or j["K"] % 4:
            raise RuntimeError("rowdot_jobs: contiguous fp32 matrices with K % 4 == 0")
    arr = (lib.RowdotJob * len(jobs))(*[lib.RowdotJob(int(j["in_off"]), int(j["in_stride"]), int(j["out_off"]), j["M"].data_ptr(),
                                                      j["bias"].data_ptr() if j["bias"] is not None else 0, int(j["G"]), int(j["O"]),
                                                      int(j["K"]), float(j["scale"])) for j in jobs])
    table = torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(device)
    return table, len(jobs), max(j["O"] for j in jobs), max(j["G"] for j in jobs)


def rowdot_multi(table, njobs, max_o, max_g, in_base, out_base, mode):
    call("e4s_rowdot_multi_f32", ptr(table), njobs, fptr(in_base), fptr(out_base), max_o, max_g, mode, stream())


def demod_coefs(s, wsq, conv_scale):
    """conv_scale * rsqrt(conv_scale^2 * sum_ci s^2 Wsq[co,ci] + 1e-8): [G, Cout]."""
    g, cin = s.shape
    cout = wsq.shape[0]
    out = torch.empty(g, cout, device=s.device, dtype=torch.float32)
    call("e4s_rowdot_f32", fptr(s), cin, fptr(wsq), None, fptr(out), g, cout, cin, 1, float(conv_scale), stream())
    return out


def weight_sqsum(w, out=None):
    """w [Cout,Cin,kh,kw] -> [Cout,Cin] sum of squares over taps (into `out` when given: the generator keeps ONE such matrix per
    layer for its lifetime, so the style prologue's job tables -- which hold its address -- survive weight updates)."""
    w = _f32(w)
    cout, cin = w.shape[:2]
    taps = w.shape[2] * w.shape[3]
    if out is None:
        out = torch.empty(cout, cin, device=w.device, dtype=torch.float32)
    elif out.shape != (cout, cin) or out.dtype != torch.float32 or out.device != w.device or not out.is_contiguous():
        raise RuntimeError("weight_sqsum: out must be a contiguous fp32 [Cout,Cin] tensor on the weight's device")
    call("e4s_weight_sqsum_f32", fptr(w), fptr(out), cout, cin, taps, stream())
    return out


def _into(out, shape, device):
    """`out` if given (checked: contiguous fp32 of exactly `shape` on `device`), else a fresh tensor.  The weight-pack builders take `out`
    so that a module can keep ONE buffer per pack for its lifetime: a re-pack after a weight update -- eager, or replayed inside a captured
    train step -- then writes in place and allocates nothing (stylegan2.ModulatedConv2d._buf)."""
    if out is None:
        return torch.empty(shape, device=device, dtype=torch.float32)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != device or not out.is_contiguous():
        raise RuntimeError(f"pack buffer mismatch: need contiguous fp32 {tuple(shape)} on {device}, got {tuple(out.shape)} {out.dtype} {out.device}")
    return out


def pack_taps(w, out=None):
    """w [Cout,Cin,kh,kw] -> [1, kh*kw, Cout, Cin] (the conv kernel's B operand layout)."""
    w = _f32(w)
    cout, cin = w.shape[:2]
    taps = w.shape[2] * w.shape[3]
    out = _into(out, (1, taps, cout, cin), w.device)
    call("e4s_pack_taps_f32", fptr(w), fptr(out), cout, cin, taps, stream())
    return out


def polyphase_weights(w, blur_kernel, out=None):
    """w [Cout,Cin,3,3] + 4x4 blur -> [4, 9, Cout, Cin] phase kernels of the fused transposed conv + blur."""
    w = _f32(w)
    cout, cin = w.shape[:2]
    out = _into(out, (4, 9, cout, cin), w.device)
    call("e4s_polyphase_weights_f32", fptr(w), fptr(_f32(blur_kernel)), fptr(out), cout, cin, stream())
    return out


def polyphase_fold(deff, blur_kernel, cout, cin):
    """Gradient of the 4 x 9 polyphase kernels [36, Cout, Cin] (contiguous) -> gradient of the 3x3 weight [Cout, Cin, 3, 3]: the transpose of
    polyphase_weights."""
    deff = _f32(deff)
    if deff.numel() != 36 * cout * cin:
        raise RuntimeError("polyphase_fold: deff must hold 4 * 9 * Cout * Cin values")
    dw = torch.empty(cout, cin, 3, 3, device=deff.device, dtype=torch.float32)
    call("e4s_polyphase_fold_f32", fptr(deff), fptr(_f32(blur_kernel)), fptr(dw), cout, cin, stream())
    return dw


def rgb_weights(w, s, scale):
    """ws[g,c,ci] = scale*w[c,ci]*s[g,ci]; w [3,Cin]."""
    g, cin = s.shape
    out = torch.empty(g, 3, cin, device=s.device, dtype=torch.float32)
    call("e4s_rgb_weights_f32", fptr(w), fptr(s), fptr(out), g, cin, float(scale), stream())
    return out


# ---- mask plan -------------------------------------------------------------------------------
_tls = threading.local()


@contextlib.contextmanager
def flag_sink(flags):
    """While active (HIP-graph capture), every mask_labels call OF THIS THREAD ORs its not-one-hot flag into `flags`
    (int32[1] device tensor) instead of a fresh tensor, so that a replayed graph can still be validated afterwards.
    Thread-local: another thread's strict-mask check keeps reading its own flag tensor."""
    prev = getattr(_tls, "sink", None)
    _tls.sink = flags
    try:
        yield flags
    finally:
        _tls.sink = prev


def mask_labels(mask):
    """one-hot [B,R,Hm,Wm] fp32 -> (labels uint8 [B,Hm,Wm], flags int32[1]); flags!=0 => not one-hot."""
    mask = _f32(mask)
    b, r, hm, wm = mask.shape
    labels = torch.empty(b, hm, wm, device=mask.device, dtype=torch.uint8)
    sink = getattr(_tls, "sink", None)
    flags = sink if sink is not None else torch.zeros(1, device=mask.device, dtype=torch.int32)
    call("e4s_mask_labels", fptr(mask), ptr(labels), ptr(flags), b, r, hm, wm, stream())
    return labels, flags


def swap_styles(tgt, src, comp_indices, below_face=False):
    """scripts/face_swap.py:117-146 per sample, one launch (e4s_swap_styles_f32): tgt / src [B,R,C] -> [B,R,C]."""
    tgt, src = _f32(tgt), _f32(src)
    b, r, c = tgt.shape
    out = torch.empty_like(tgt)
    sel = 0
    for i in comp_indices:
        sel |= 1 << int(i)
    call("e4s_swap_styles_f32", fptr(tgt), fptr(src), fptr(out), b, r, c, sel, 7, 9, 8 if below_face else -1, stream())
    return out


class RowPlan:
    __slots__ = ("rows", "tiles", "meta", "tiles_cap", "Ha", "Wa", "nphase", "R")


def region_plan(labels, num_regions, ha, wa, nphase):
    b, hm, wm = labels.shape
    nkeys = b * num_regions * nphase
    rows_cap = b * ha * wa * nphase + nkeys * BM
    tiles_cap = (rows_cap + BM - 1) // BM
    dev = labels.device
    pl = RowPlan()
    pl.rows = torch.empty(rows_cap, device=dev, dtype=torch.int32)
    pl.tiles = torch.empty(tiles_cap * 4, device=dev, dtype=torch.int32)
    pl.meta = torch.empty(4, device=dev, dtype=torch.int32)
    work = torch.empty(3 * nkeys, device=dev, dtype=torch.int32)
    call("e4s_region_plan", ptr(labels), b, num_regions, hm, wm, ha, wa, nphase, BM, ptr(pl.rows), ptr(pl.tiles),
         ptr(pl.meta), ptr(work), rows_cap, tiles_cap, stream())
    pl.tiles_cap, pl.Ha, pl.Wa, pl.nphase, pl.R = tiles_cap, ha, wa, nphase, num_regions
    return pl


# ---- the conv --------------------------------------------------------------------------------
_split_tl = threading.local()


@contextlib.contextmanager
def f32_plain_split(on=True):
    """Inside this context e4s_conv_mfma_f32 may split K on plain maps with < 256 blocks per sample (e4s_conv_params.split_hint): the frozen
    loss networks opt in (criteria.py, forward AND backward -- autograd runs the backward on its own thread, so each Function sets it again)."""
    prev = getattr(_split_tl, "on", False)
    _split_tl.on = bool(on)
    try:
        yield
    finally:
        _split_tl.on = prev


def conv_mfma(x, w, cout, *, plan=None, istride=1, ostride=1, ntaps=9, ncls=1, in_scale=None, out_scale=None,
              noise=None, noise_w=None, noise_per_channel=False, bias=None, slope=None, act=0, alpha=0.2,
              gain=LRELU_GAIN, spatial=None, anchors=None, labels=None, num_regions=1, w_split=None, in_stats=None,
              out=None, tap_shift=0, want_stats=False, w_split16=None, se=None, w_frag=None):
    """x NHWC [B,Hi,Wi,Cin]; w [ncls, ntaps, Cout, Cin] -> y NHWC [B,Ho,Wo,Cout].
    anchors = (Ha, Wa); defaults: up-conv (ncls=4) anchors = input grid, output 2x;
    strided conv anchors = output grid.
    w_split: the split-bf16 image of w (split_bf16x2); when given the contraction runs on e4s_conv_bf16x3_f32
    (callers check bf16x3_eligible first -- an ineligible shape is an error, not a silent fp32 run).
    w_split16: (masked layers, with w_split) the 16-channel-chunk split image (split16_bf16x2): the contraction runs on
    e4s_conv_region_bf16x3_f32 (variant-rows kernel; the region-select kernel for tiles / launches it does not take).
    w_frag: (strided / 1x1 launches, with w_split) the fragment-major split image (gather_frag_bf16x2): where the launch is eligible
    (Cout % 128 == 0) it runs the one-wave-per-SIMD gather kernel -- the same output bits; without it the 8-wave kernel.
    in_stats: [B,Cin,2] InstanceNorm statistics of x; the normalisation is applied while the input is staged (split-bf16
    kernel only).
    out: write the Cout channels into the FIRST channels of this wider NHWC tensor [B,Ho,Wo,Cy >= Cout] (returned).
    tap_shift: gather kernels only: 1 = padding-0 strided conv (input coord = anchor*istride + tap).
    se = (fc1 [Cr,C], fc2 [C,Cr]) with want_stats: the second element of the returned pair is the SE gate [B,Cout] of the
    normalised output instead of `pooled` (one launch with the statistics' second stage where the epilogue emitted them).
    want_stats: also return the InstanceNorm statistics of the OUTPUT, (y, (stats [B,Cout,2], pooled [B,Cout])): emitted by
    the split-bf16 kernels' epilogue (no extra pass over y) where that applies, by e4s_instnorm_stats_f32 otherwise."""
    b, hi, wi, cin = x.shape
    if anchors is None:
        anchors = (hi // istride, wi // istride)
    ha, wa = anchors
    ho, wo = ha * ostride, wa * ostride
    if spatial is None:
        spatial = plan is None and istride == 1 and ntaps == 9
    if labels is not None and not spatial:
        raise RuntimeError("per-pixel region labels need the spatial (halo-tiled) mode")
    if plan is None and not spatial and (ha * wa) % BM != 0 and w_split is None and (in_scale is not None or out_scale is not None):
        # with a per-sample style / demodulation row the tiles must not straddle samples: a trivial one-region plan
        plan = region_plan(torch.zeros(b, 1, 1, device=x.device, dtype=torch.uint8), 1, ha, wa, ncls)
    if out is None:
        y = torch.empty(b, ho, wo, cout, device=x.device, dtype=torch.float32)
    else:
        y = out
        if tuple(y.shape[:3]) != (b, ho, wo) or y.shape[3] < cout or labels is not None or plan is not None:
            raise RuntimeError("conv_mfma(out=...): need an unlabelled conv and an NHWC buffer [B,Ho,Wo,>=Cout]")
    p = ConvParams()
    p.x, p.w, p.y = fptr(x), fptr(w), fptr(y)
    p.y_cstride = y.shape[3] if out is not None else 0
    p.tap_shift = int(tap_shift)
    if plan is not None:
        p.rows, p.tiles, p.meta, p.tiles_cap = ptr(plan.rows), ptr(plan.tiles), ptr(plan.meta), plan.tiles_cap
        p.groups_per_batch = plan.R
    else:
        p.rows = p.tiles = p.meta = None
        p.tiles_cap = 0
        p.groups_per_batch = num_regions if labels is not None else 1
    if labels is not None:
        p.labels, p.Hm, p.Wm = ptr(labels), labels.shape[1], labels.shape[2]
    else:
        p.labels, p.Hm, p.Wm = None, 0, 0
    p.B, p.Ha, p.Wa = b, ha, wa
    p.Hi, p.Wi, p.Ho, p.Wo, p.Cin, p.Cout = hi, wi, ho, wo, cin, cout
    p.istride, p.ostride, p.ntaps, p.ncls = istride, ostride, ntaps, ncls
    p.in_scale, p.out_scale = fptr(in_scale), fptr(out_scale)
    if noise is not None:
        p.noise, p.noise_w = fptr(noise), fptr(noise_w)
        p.noise_bstride = ho * wo if noise.shape[0] > 1 else 0
        p.noise_per_channel = 1 if noise_per_channel else 0
    else:
        p.noise = p.noise_w = None
        p.noise_bstride = 0
        p.noise_per_channel = 0
    p.bias, p.slope = fptr(bias), fptr(slope)
    p.act, p.alpha, p.gain = act, alpha, gain
    p.in_stats = fptr(in_stats)
    p.split_hint = 1 if getattr(_split_tl, "on", False) else 0
    if w_split is not None:
        gather_ok = (istride == 2 or ntaps == 1) and cin % 32 == 0 and (cout % 128 == 0 or cout == 64) and ncls == 1 and ostride == 1 \
            and plan is None and labels is None and in_scale is None and out_scale is None and noise is None \
            and in_stats is None
        if not gather_ok and (
                not bf16x3_eligible(cin, cout, istride=istride, ostride=ostride, ntaps=ntaps, ncls=ncls,
                                    masked=labels is not None)
                or not spatial or (noise_per_channel and (in_scale is None or in_stats is not None))
                or (labels is not None and in_scale is None)
                or (in_stats is not None and (in_scale is not None or labels is not None))):
            raise RuntimeError("e4s_conv_bf16x3_f32 does not cover this contraction")
        p.w = fptr(w_split)
        if w_split16 is not None:
            if labels is None or out is not None:
                raise RuntimeError("e4s_conv_region_bf16x3_f32 is the masked-layer kernel")
            nws = lib.load().e4s_conv_region_ws_floats(ctypes.byref(p))    # tile flags, or split-K slabs
            if nws <= 0:
                raise RuntimeError("e4s_conv_region_bf16x3_f32 does not cover this contraction")
            skws = torch.empty(nws, device=x.device, dtype=torch.float32)
            p.splitk_ws = fptr(skws)
            global LAST_REGION_PATH
            LAST_REGION_PATH = lib.load().e4s_conv_region_path(ctypes.byref(p))     # 1: 8-wave kernel, 2: one wave per SIMD, 3: packed small-map tiles (tests / bench)
            call("e4s_conv_region_bf16x3_f32", ctypes.byref(p), ptr(w_split16), stream())
            return y
        if gather_ok:
            p.w_frag = ptr(w_frag) if w_frag is not None else None
            global LAST_GATHER_PATH
            LAST_GATHER_PATH = lib.load().e4s_conv_gather_path(ctypes.byref(p))     # 1: 8-wave kernel, 2: one wave per SIMD (tests / bench)
        nws = lib.load().e4s_conv_bf16x3_ws_floats(ctypes.byref(p))        # split-K partial sums (few-tile launches)
        skws = torch.empty(nws, device=x.device, dtype=torch.float32) if nws else None
        p.splitk_ws = fptr(skws)
        fused = None
        if want_stats and nws == 0 and act == 0 and noise is None and out_scale is None and labels is None and ncls == 1 \
                and cout % 64 == 0 and out is None:
            if gather_ok:
                slots = (ha * wa) // 256 if (ha * wa) % 256 == 0 else 0
            else:
                slots = ((ha + 15) // 16) * ((wa + 15) // 16)
            if slots:
                fused = torch.empty(b * cout * slots * 2, device=x.device, dtype=torch.float64)
                p.stats_ws, p.stats_slots = ptr(fused), slots
        call("e4s_conv_bf16x3_f32", ctypes.byref(p), stream())
        if fused is not None:
            stats = torch.empty(b, cout, 2, device=x.device, dtype=torch.float32)
            pooled = torch.empty(b, cout, device=x.device, dtype=torch.float32)
            if se is not None:
                call("e4s_instnorm_finalize_se_f32", ptr(fused), fptr(stats), fptr(se[0]), fptr(se[1]), fptr(pooled), b, ho * wo,
                     cout, se[0].shape[0], p.stats_slots, 1e-5, stream())
            else:
                call("e4s_instnorm_finalize_f32", ptr(fused), fptr(stats), fptr(pooled), b, ho * wo, cout, p.stats_slots, 1e-5,
                     stream())
            return y, (stats, pooled)
    elif in_stats is not None:
        raise RuntimeError("fused InstanceNorm staging exists only in e4s_conv_bf16x3_f32")
    else:
        nws = lib.load().e4s_conv_mfma_ws_floats(ctypes.byref(p), 1 if spatial else 0)     # split-K slabs (few-block launches)
        skws = torch.empty(nws, device=x.device, dtype=torch.float32) if nws else None
        p.splitk_ws = fptr(skws)
        call("e4s_conv_mfma_f32", ctypes.byref(p), 1 if spatial else 0, stream())
    if want_stats:
        stats, pooled = instnorm_stats(y, want_pooled=True)
        return y, (stats, se_gate(pooled, se[0], se[1]) if se is not None else pooled)
    return y


def bf16x3_eligible(cin, cout, *, istride=1, ostride=1, ntaps=9, ncls=1, masked=False):
    """Shapes e4s_conv_bf16x3_f32 covers (include/e4s_hip.h): natural-order 3x3, plain or polyphase up-conv; column
    tiles of 128 / 64 / 32 without a label map, 128 with one (region-select kernel)."""
    return (cin % 32 == 0 and cout % (128 if masked else 32) == 0 and istride == 1 and ntaps == 9
            and (ncls, ostride) in ((1, 1), (4, 2)))


def fills_chip(tiles, nchunk, ksplit=None):
    """Policy ESTIMATE: does a split-bf16 launch of `tiles` tiles over `nchunk` input-channel chunks keep the chip busy -- >= BF16X3_MIN_BLOCKS
    tiles, or >= 64 blocks once the library splits K?  The library's rules are csrc/split_policy.h; only the gather rule is asked there
    (ksplit = gather_split(...)).  Otherwise the splits are taken as the number few_tiles_split WANTS, min(nchunk // 2, ceil(256 / tiles)),
    which overcounts: the rule rounds it down to ceil(nchunk / ceil(nchunk / want)) parts, the Winograd form refuses a split whose last
    part is one chunk, and neither splits above 128 tiles (DESIGN section 6 lists the shapes where the answers differ)."""
    if tiles >= BF16X3_MIN_BLOCKS:
        return True
    if ksplit is None:
        ksplit = min(nchunk // 2, -(-256 // tiles)) if nchunk >= 4 else 1
    return tiles * max(ksplit, 1) >= 64


def want_bf16x3(b, h, w, cin, cout, ncls=1, masked=False):
    """Policy of PRECISION for a natural-order 3x3 conv (ncls = 4: polyphase up-conv) on [b,h,w,cin] -> cout."""
    if PRECISION == "f32" or not bf16x3_eligible(cin, cout, ncls=ncls, ostride=2 if ncls == 4 else 1, masked=masked):
        return False
    if PRECISION == "bf16x3":
        return True
    # 256-pixel x 128/64/32-column tiles (unmasked polyphase up-conv: ONE GEMM with 4*Cout columns)
    n = 4 * cout if (ncls == 4 and not masked) else cout
    bn = 128 if n % 128 == 0 else 64 if n % 64 == 0 else 32
    tiles = b * ((h + 15) // 16) * ((w + 15) // 16) * (n // bn) * (ncls if masked else 1)
    return fills_chip(tiles, cin // 32)       # few tiles (batch-1 latency runs): the kernels split the input channels over blocks


def gather_split(tiles, cin, ntaps):
    """K splits of a strided (gather-kernel) split-bf16 launch of `tiles` 256-pixel x 128-column tiles: the library's own rule
    (e4s_gather_ksplit: 3x3, <= 64 tiles, Cin >= 256)."""
    return lib.load().e4s_gather_ksplit(tiles, cin, ntaps)


def split_bf16x2(w, out=None):
    """fp32 [..., Cin] -> its split-bf16 image (hi|lo per 32-channel chunk), returned as an opaque fp32-typed tensor of
    the same shape/byte size (only e4s_conv_bf16x3_f32 reads it)."""
    w = _f32(w)
    out = _into(out, tuple(w.shape), w.device)
    cin = w.shape[-1]
    call("e4s_split_bf16x2_f32", fptr(w), ptr(out), w.numel() // cin, cin, stream())
    return out


def gather_frag_bf16x2(w, out=None):
    """fp32 tap-packed weights [1, ntaps, Cout, Cin] -> the fragment-major split image the one-wave-per-SIMD gather kernel loads its weight
    fragments from (conv_mfma's w_frag; opaque fp32-typed tensor of the same shape / byte size).  Cin % 32 == 0, Cout % 32 == 0."""
    w = _f32(w)
    out = _into(out, tuple(w.shape), w.device)
    ntaps, cout, cin = w.shape[-3], w.shape[-2], w.shape[-1]
    if w.numel() != ntaps * cout * cin or lib.load().e4s_gather_frag_bytes(ntaps, cout, cin) != out.numel() * 4:
        raise RuntimeError("gather_frag_bf16x2: one set of taps [ntaps, Cout, Cin] with Cin % 32 == 0 and Cout % 32 == 0")
    call("e4s_gather_frag_bf16x2_f32", fptr(w), ptr(out), ntaps, cout, cin, stream())
    return out


def split16_shape(w_shape):
    """Shape of the opaque fp32-typed tensor split16_bf16x2 fills for tap-packed weights of shape w_shape: (k,) + w_shape, k = 2 when Cout % 32 == 0
    (plane-major image + fragment-major image, e4s_split16_bytes), else 1."""
    return (2 if w_shape[-2] % 32 == 0 else 1,) + tuple(w_shape)


def split16_bf16x2(w, out=None):
    """fp32 tap-packed weights [ncls, 9, Cout, Cin] -> the split images e4s_conv_region_bf16x3_f32 reads (opaque): [ncls*9][Cin/16][Cout][16 hi | 16 lo]
    and, for Cout % 32 == 0, behind it the same values fragment-major (the one-wave-per-SIMD kernel's B fragments come straight from it)."""
    w = _f32(w)
    out = _into(out, split16_shape(w.shape), w.device)
    cout, cin = w.shape[-2], w.shape[-1]
    rows = w.numel() // (cout * cin)
    if lib.load().e4s_split16_bytes(rows, cout, cin) != out.numel() * 4:
        raise RuntimeError("split16_bf16x2: buffer size")
    call("e4s_split16_bf16x2_f32", fptr(w), ptr(out), rows, cout, cin, stream())
    return out


REGION_1W = os.environ.get("E4S_REGION_1W", "1") != "0"        # the library reads the same variable (csrc/conv_region.hip e4s_plan_masked)
REGION_PACK = os.environ.get("E4S_REGION_PACK", "1") != "0"    # the library reads the same variable (csrc/conv_bf16x3.hip): packed small-map tiles
LAST_GATHER_PATH = 0           # which kernel the last strided / 1x1 split-bf16 launch took (e4s_conv_gather_path): 1 8-wave kernel, 2 one wave per SIMD
LAST_REGION_PATH = 0           # which kernel the last masked launch took (e4s_conv_region_path): 1 8-wave rows kernel, 2 one wave per SIMD, 3 packed small-map tiles
WINO = os.environ.get("E4S_WINO", "1") == "1"        # policy switch of the Winograd F(2,3) kernel (encoders._conv3x3)


def wino_eligible(b, h, w, cin, cout, in_stats=False):
    """Shapes e4s_conv_wino_bf16x3_f32 covers, and whether the launch fills the chip (one 16x16-pixel x 128-column tile per block; launches
    of <= 128 tiles split the input-channel chunks over blocks: fills_chip's estimate).  in_stats: the launch folds an
    InstanceNorm into its input transform, whose {mean, rstd} tables live in LDS: Cin <= 1024 (the launcher refuses more)."""
    if not WINO or PRECISION == "f32":
        return False
    if h % 16 or w % 16 or cin % 16 or cin < 32 or cout % 128:
        return False
    if in_stats and cin > 1024:
        return False
    if PRECISION == "bf16x3":
        return True
    return fills_chip(b * (h // 16) * (w // 16) * (cout // 128), cin // 16)


def wino_weights(w9):
    """tap-packed fp32 weights [1, 9, Cout, Cin] (pack_taps) -> the transformed, hi/lo-split operand of conv_wino (opaque uint8)."""
    w9 = _f32(w9)
    cout, cin = w9.shape[-2], w9.shape[-1]
    if w9.numel() != 9 * cout * cin:
        raise RuntimeError("wino_weights: one set of nine taps [9, Cout, Cin]")
    n = lib.load().e4s_wino_weights_bytes(cout, cin)
    if n <= 0:
        raise RuntimeError("wino_weights: Cin must be a multiple of 16")
    out = torch.empty(n, device=w9.device, dtype=torch.uint8)
    call("e4s_wino_weights_f32", fptr(w9), ptr(out), cout, cin, stream())
    return out


def conv_wino(x, u, cout, *, in_stats=None, bias=None, slope=None, act=0, alpha=0.2, gain=LRELU_GAIN, want_stats=False, se=None):
    """Stride-1 3x3 conv of x NHWC [B,H,W,Cin] as Winograd F(2,3) along the rows (e4s_conv_wino_bf16x3_f32); u = wino_weights(...).
    in_stats / act / slope / want_stats / se as conv_mfma."""
    b, h, w, cin = x.shape
    y = torch.empty(b, h, w, cout, device=x.device, dtype=torch.float32)
    p = ConvParams()
    p.x, p.w, p.y = fptr(x), ptr(u), fptr(y)
    p.rows = p.tiles = p.meta = None
    p.B, p.Ha, p.Wa, p.Hi, p.Wi, p.Ho, p.Wo, p.Cin, p.Cout = b, h, w, h, w, h, w, cin, cout
    p.istride, p.ostride, p.ntaps, p.ncls, p.groups_per_batch = 1, 1, 9, 1, 1
    p.bias, p.slope = fptr(bias), fptr(slope)
    p.act, p.alpha, p.gain = act, alpha, gain
    p.in_stats = fptr(in_stats)
    fused = None
    if want_stats and act != 0:
        raise RuntimeError("conv_wino: output statistics are those of the raw conv output (act = 0)")
    nws = lib.load().e4s_conv_wino_ws_floats(ctypes.byref(p))            # split-K slabs (few-tile launches)
    skws = torch.empty(nws, device=x.device, dtype=torch.float32) if nws else None
    p.splitk_ws = fptr(skws)
    if want_stats and not nws:
        slots = (h // 16) * (w // 16)
        fused = torch.empty(b * cout * slots * 2, device=x.device, dtype=torch.float64)
        p.stats_ws, p.stats_slots = ptr(fused), slots
    call("e4s_conv_wino_bf16x3_f32", ctypes.byref(p), stream())
    if fused is None:
        if not want_stats:
            return y
        stats, pooled = instnorm_stats(y, want_pooled=True)              # split launch: the separate statistics pass
        return y, (stats, se_gate(pooled, se[0], se[1]) if se is not None else pooled)
    stats = torch.empty(b, cout, 2, device=x.device, dtype=torch.float32)
    pooled = torch.empty(b, cout, device=x.device, dtype=torch.float32)
    if se is not None:
        call("e4s_instnorm_finalize_se_f32", ptr(fused), fptr(stats), fptr(se[0]), fptr(se[1]), fptr(pooled), b, h * w, cout,
             se[0].shape[0], p.stats_slots, 1e-5, stream())
    else:
        call("e4s_instnorm_finalize_f32", ptr(fused), fptr(stats), fptr(pooled), b, h * w, cout, p.stats_slots, 1e-5, stream())
    return y, (stats, pooled)


def upconv_mfma(x, w3, cout, k4, *, in_scale=None, out_scale=None, labels=None, num_regions=1, noise=None,
                noise_w=None, noise_per_channel=False, bias=None, act=0, alpha=0.2, gain=LRELU_GAIN, out=None):
    """Exact transposed-conv + blur up-sampling conv.  x NHWC [B,H,W,Cin]; w3 [1,9,Cout,Cin] (plain taps);
    k4 the 4x4 blur kernel -> y NHWC [B,2H,2W,Cout]."""
    b, hi, wi, cin = x.shape
    ho, wo = 2 * hi, 2 * wi
    y = torch.empty(b, ho, wo, cout, device=x.device, dtype=torch.float32) if out is None else out
    p = ConvParams()
    p.x, p.w, p.y = fptr(x), fptr(w3), fptr(y)
    p.y_cstride = y.shape[3] if out is not None else 0
    p.rows = p.tiles = p.meta = None
    p.tiles_cap = 0
    p.B, p.Ha, p.Wa = b, hi, wi
    p.Hi, p.Wi, p.Ho, p.Wo, p.Cin, p.Cout = hi, wi, ho, wo, cin, cout
    p.istride, p.ostride, p.ntaps, p.ncls = 1, 2, 9, 1
    p.in_scale, p.out_scale = fptr(in_scale), fptr(out_scale)
    p.groups_per_batch = num_regions if labels is not None else 1
    if labels is not None:
        p.labels, p.Hm, p.Wm = ptr(labels), labels.shape[1], labels.shape[2]
    else:
        p.labels, p.Hm, p.Wm = None, 0, 0
    if noise is not None:
        p.noise, p.noise_w = fptr(noise), fptr(noise_w)
        p.noise_bstride = ho * wo if noise.shape[0] > 1 else 0
        p.noise_per_channel = 1 if noise_per_channel else 0
    else:
        p.noise = p.noise_w = None
        p.noise_bstride = 0
        p.noise_per_channel = 0
    p.bias, p.slope = fptr(bias), None
    p.act, p.alpha, p.gain = act, alpha, gain
    call("e4s_upconv_mfma_f32", ctypes.byref(p), fptr(_f32(k4)), stream())
    return y


def subpixel_weights(w, out=None):
    """w [Cout,Cin,3,3] -> the packed, hi/lo-split sub-pixel GEMM operand of e4s_upconv_bf16x3_f32 (csrc/upconv_bf16x3.hip):
    [Cin/32, Cout/32, 9 blocks, 32 co, 32 hi | 32 lo bf16], returned as an opaque fp32-typed tensor of the same byte size."""
    w = _f32(w)
    cout, cin = w.shape[:2]
    out = _into(out, (cin // 32, cout // 32, 9, 32, 32), w.device)
    call("e4s_subpixel_weights_f32", fptr(w), ptr(out), cout, cin, stream())
    return out


def upconv_bf16x3_eligible(cin, cout):
    """e4s_upconv_bf16x3_f32: 32-channel output tiles, 32-channel chunks of packed weights, the sample's style row (<= 512 channels) in LDS."""
    return cin % 64 == 0 and cin <= 512 and cout % 32 == 0


def upconv_bf16x3(x, w_sub, cout, k4, *, in_scale=None, out_scale=None, noise=None, noise_w=None, noise_per_channel=False, bias=None,
                  act=0, alpha=0.2, gain=LRELU_GAIN, out=None):
    """Exact transposed conv + blur + noise + bias + act on the split-bf16 matrix-core path, one style per sample.
    x NHWC [B,H,W,Cin]; w_sub = subpixel_weights(w); k4 the 4x4 blur kernel (device tensor) -> NHWC [B,2H,2W,Cout].
    noise [1|B,1,2H,2W], or with noise_per_channel NHWC [1|B,2H,2W,Cout] (needs in_scale)."""
    b, hi, wi, cin = x.shape
    ho, wo = 2 * hi, 2 * wi
    y = torch.empty(b, ho, wo, cout, device=x.device, dtype=torch.float32) if out is None else out
    p = ConvParams()
    p.x, p.w, p.y = fptr(x), fptr(w_sub), fptr(y)
    p.y_cstride = y.shape[3] if out is not None else 0
    p.rows = p.tiles = p.meta = None
    p.tiles_cap = 0
    p.B, p.Ha, p.Wa = b, hi, wi
    p.Hi, p.Wi, p.Ho, p.Wo, p.Cin, p.Cout = hi, wi, ho, wo, cin, cout
    p.istride, p.ostride, p.ntaps, p.ncls = 1, 2, 9, 1
    p.in_scale, p.out_scale = fptr(in_scale), fptr(out_scale)
    p.groups_per_batch = 1
    p.labels, p.Hm, p.Wm = None, 0, 0
    if noise is not None:
        p.noise, p.noise_w = fptr(noise), fptr(noise_w)
        p.noise_bstride = ho * wo if noise.shape[0] > 1 else 0
    else:
        p.noise = p.noise_w = None
        p.noise_bstride = 0
    p.noise_per_channel = 1 if (noise is not None and noise_per_channel) else 0
    p.bias, p.slope = fptr(bias), None
    p.act, p.alpha, p.gain = act, alpha, gain
    call("e4s_upconv_bf16x3_f32", ctypes.byref(p), fptr(_f32(k4)), stream())
    return y


def conv_c32(x, w_split, cout, *, in_scale=None, out_scale=None, noise=None, noise_w=None, noise_per_channel=False, bias=None, act=0,
             alpha=0.2, gain=LRELU_GAIN, rgb_ws=None):
    """3x3 stride-1 conv with 32 input channels on e4s_conv_c32_bf16x3_f32 (weights resident in LDS).  x NHWC [B,H,W,32];
    w_split = split_bf16x2(pack_taps(w)); rgb_ws [B,3,32]: also return the ToRGB partial [B,3,H,W] of the OUTPUT (Cout == 32).
    noise [1|B,1,H,W], or with noise_per_channel NHWC [1|B,H,W,Cout] (needs in_scale).  Returns y NHWC [B,H,W,Cout] or (y, rgb_partial)."""
    b, h, w, cin = x.shape
    if cin != 32 or cout % 32:
        raise RuntimeError("conv_c32: Cin == 32 and Cout % 32 == 0")
    y = torch.empty(b, h, w, cout, device=x.device, dtype=torch.float32)
    p = ConvParams()
    p.x, p.w, p.y = fptr(x), fptr(w_split), fptr(y)
    p.y_cstride = 0
    p.rows = p.tiles = p.meta = None
    p.tiles_cap = 0
    p.B, p.Ha, p.Wa = b, h, w
    p.Hi, p.Wi, p.Ho, p.Wo, p.Cin, p.Cout = h, w, h, w, cin, cout
    p.istride, p.ostride, p.ntaps, p.ncls = 1, 1, 9, 1
    p.in_scale, p.out_scale = fptr(in_scale), fptr(out_scale)
    p.groups_per_batch = 1
    p.labels, p.Hm, p.Wm = None, 0, 0
    if noise is not None:
        p.noise, p.noise_w = fptr(noise), fptr(noise_w)
        p.noise_bstride = h * w if noise.shape[0] > 1 else 0
    else:
        p.noise = p.noise_w = None
        p.noise_bstride = 0
    p.noise_per_channel = 1 if (noise is not None and noise_per_channel) else 0
    p.bias, p.slope = fptr(bias), None
    p.act, p.alpha, p.gain = act, alpha, gain
    partial = None
    if rgb_ws is not None:
        if cout != 32 or tuple(rgb_ws.shape) != (b, 3, 32):
            raise RuntimeError("conv_c32: the fused ToRGB partial needs Cout == 32 and rgb_ws [B,3,32]")
        partial = torch.empty(b, 3, h, w, device=x.device, dtype=torch.float32)
    call("e4s_conv_c32_bf16x3_f32", ctypes.byref(p), fptr(rgb_ws), fptr(partial), stream())
    return y if partial is None else (y, partial)


def torgb_finish(partial, bias, skip, k4):
    """partial [B,3,H,W] (the fused ToRGB contraction) + bias + FIR-upsampled skip [B,3,H/2,W/2] -> [B,3,H,W]."""
    b, _, h, w = partial.shape
    out = torch.empty_like(partial)
    call("e4s_torgb_finish_f32", fptr(partial), fptr(_f32(bias)), fptr(skip), fptr(_f32(k4)) if skip is not None else None,
         fptr(out), b, h, w, stream())
    return out


def torgb(x, ws, bias, skip, k4, labels, num_regions):
    """x NHWC [B,H,W,Cin]; ws [G,3,Cin]; skip NCHW [B,3,H/2,W/2] or None -> NCHW [B,3,H,W]."""
    b, h, w, cin = x.shape
    out = torch.empty(b, 3, h, w, device=x.device, dtype=torch.float32)
    hm = wm = 0
    if labels is not None:
        hm, wm = labels.shape[1:]
    call("e4s_torgb_f32", fptr(x), fptr(ws), fptr(bias), fptr(skip), fptr(k4), ptr(labels), hm, wm, num_regions,
         fptr(out), b, h, w, cin, stream())
    return out


def mask_mul_add(y, mask, r, out, channels_last):
    """out (+)= y * nearest(mask)[:, r]  (soft-mask fallback); out=None allocates (overwrite)."""
    if channels_last:
        b, h, w, c = y.shape
    else:
        b, c, h, w = y.shape
    acc = 1 if out is not None else 0
    if out is None:
        out = torch.empty_like(y)
    mask = _f32(mask)
    call("e4s_mask_mul_add_f32", fptr(y), fptr(mask), fptr(out), r, b, h, w, c, mask.shape[1], mask.shape[2],
         mask.shape[3], 1 if channels_last else 0, acc, stream())
    return out


def noise_bias_act_nhwc(x, noise, noise_w, bias, alpha, gain):
    b, h, w, c = x.shape
    y = torch.empty_like(x)
    nb = 0 if noise is None or noise.shape[0] == 1 else h * w
    call("e4s_noise_bias_act_nhwc_f32", fptr(x), fptr(noise), fptr(noise_w) if noise is not None else None, nb,
         fptr(bias), fptr(y), b, h * w, c, float(alpha), float(gain), stream())
    return y


# ---- encoder ---------------------------------------------------------------------------------
def resize_bilinear_to_nhwc(x, ho, wo):
    x = _f32(x)
    b, c, hi, wi = x.shape
    y = torch.empty(b, ho, wo, c, device=x.device, dtype=torch.float32)
    call("e4s_resize_bilinear_f32", fptr(x), fptr(y), b, c, hi, wi, ho, wo, stream())
    return y


def conv3x3_small(x, w, want_stats=False):
    """Stem conv (3x3, pad 1, tiny Cin): x NHWC [B,H,W,Cin], w [Cout,Cin,3,3] -> NHWC [B,H,W,Cout].  Cin = 3, Cout = 64 on maps that are
    multiples of 16 run on the tiled kernel (e4s_conv3x3_stem_f32); want_stats: (y, InstanceNorm statistics of y [B,Cout,2]), emitted by
    that kernel's epilogue where it applies, by e4s_instnorm_stats_f32 otherwise."""
    b, h, wd, cin = x.shape
    cout = w.shape[0]
    y = torch.empty(b, h, wd, cout, device=x.device, dtype=torch.float32)
    if cin == 3 and cout == 64 and h % 16 == 0 and wd % 16 == 0:
        slots = (h // 16) * (wd // 16)
        fused = torch.empty(b * cout * slots * 2, device=x.device, dtype=torch.float64) if want_stats else None
        call("e4s_conv3x3_stem_f32", fptr(x), fptr(_f32(w)), fptr(y), ptr(fused), b, h, wd, cin, cout, stream())
        if not want_stats:
            return y
        stats = torch.empty(b, cout, 2, device=x.device, dtype=torch.float32)
        call("e4s_instnorm_finalize_f32", ptr(fused), fptr(stats), None, b, h * wd, cout, slots, 1e-5, stream())
        return y, stats
    call("e4s_conv3x3_small_f32", fptr(x), fptr(w), fptr(y), b, h, wd, cin, cout, stream())
    if want_stats:
        return y, instnorm_stats(y)[0]
    return y


def instnorm_stats(x, want_pooled=False, eps=1e-5):
    b, h, w, c = x.shape
    stats = torch.empty(b, c, 2, device=x.device, dtype=torch.float32)
    pooled = torch.empty(b, c, device=x.device, dtype=torch.float32) if want_pooled else None
    ws = torch.empty(lib.load().e4s_instnorm_ws_doubles(b, h * w, c), device=x.device, dtype=torch.float64)
    call("e4s_instnorm_stats_f32", fptr(x), fptr(stats), fptr(pooled), ptr(ws), b, h * w, c, float(eps), stream())
    return stats, pooled


def instnorm_apply(x, stats, gate=None, res=None, res_stats=None, slope=None, rs=1, want_stats=False):
    """want_stats: also return the InstanceNorm statistics of the OUTPUT ((y, stats [B,C,2])), accumulated by the same
    pass (the next encoder unit normalises this tensor first thing, helpers.py:128)."""
    b, h, w, c = x.shape
    # the kernels index these by (b, c) and res as [B, H rs, W rs, C] without looking at their extents: a residual from an odd map
    # (15^2 -> 8^2 at stride 2) would be read past its end
    if res is not None and tuple(res.shape) != (b, h * rs, w * rs, c):
        raise ValueError(f"instnorm_apply: res {tuple(res.shape)} is not [B, H rs, W rs, C] = {(b, h * rs, w * rs, c)} (rs = {rs})")
    for name, t, n in (("stats", stats, b * c * 2), ("res_stats", res_stats, b * c * 2), ("gate", gate, b * c), ("slope", slope, c)):
        if t is not None and t.numel() != n:
            raise ValueError(f"instnorm_apply: {name} has {t.numel()} elements, expected {n}")
    y = torch.empty_like(x)
    if want_stats and c % 64 == 0:
        ws = torch.empty(lib.load().e4s_instnorm_ws_doubles(b, h * w, c), device=x.device, dtype=torch.float64)
        nslots = ctypes.c_int(0)
        call("e4s_instnorm_apply_stats_f32", fptr(x), fptr(stats), fptr(gate), fptr(res), fptr(res_stats), fptr(slope),
             fptr(y), ptr(ws), ctypes.byref(nslots), b, h, w, c, rs, stream())
        out_stats = torch.empty(b, c, 2, device=x.device, dtype=torch.float32)
        call("e4s_instnorm_finalize_f32", ptr(ws), fptr(out_stats), None, b, h * w, c, nslots.value, 1e-5, stream())
        return y, out_stats
    call("e4s_instnorm_apply_f32", fptr(x), fptr(stats), fptr(gate), fptr(res), fptr(res_stats), fptr(slope), fptr(y),
         b, h, w, c, rs, stream())
    if want_stats:
        return y, instnorm_stats(y)[0]
    return y


def se_gate(pooled, fc1, fc2):
    b, c = pooled.shape
    cr = fc1.shape[0]
    gate = torch.empty(b, c, device=pooled.device, dtype=torch.float32)
    call("e4s_se_gate_f32", fptr(pooled), fptr(fc1), fptr(fc2), fptr(gate), b, c, cr, stream())
    return gate


def region_mean_into(feats, labels, out, num_regions, out_off):
    b, h, w, c = feats.shape
    hm, wm = labels.shape[1:]
    nws = lib.load().e4s_region_mean_ws_floats(b, h * w, c, num_regions)
    ws = torch.empty(nws, device=feats.device, dtype=torch.float32) if nws else None
    call("e4s_region_mean_f32", fptr(feats), ptr(labels), hm, wm, fptr(out), fptr(ws), b, h, w, c, num_regions,
         out.shape[2], out_off, stream())


def grouped_linear(x, w, bias, add, scale, act=0, alpha=0.01):
    """x [B,R,K]; w [R,O,K]; bias [R,O]; add [O] or None -> [B,R,O]."""
    b, r, k = x.shape
    o = w.shape[1]
    y = torch.empty(b, r, o, device=x.device, dtype=torch.float32)
    call("e4s_grouped_linear_f32", fptr(x), fptr(w), fptr(bias), fptr(add), fptr(y), b, r, k, o, float(scale), act,
         float(alpha), stream())                    # any batch: each weight row is read once and kept in registers
    return y


def grouped_linear_t(g, w, scale, base=None, mul=None, ref=None, alpha=1.0):
    """out[b,r,k] = base + mul * scale * (ref > 0 ? 1 : alpha) * sum_o g[b,r,o] * w[r,o,k]   (g [B,R,O]; w [R,O,K]):
    the transposed contraction of the LocalMLP backward and of the style prologue's chain rule, weights streamed once
    per 16 samples, split partial sums added in order (bit-reproducible)."""
    b, r, o = g.shape
    k = w.shape[2]
    out = torch.empty(b, r, k, device=g.device, dtype=torch.float32)
    for lo in range(0, b, 16):
        n = min(16, b - lo)
        ws = torch.empty(lib.load().e4s_grouped_linear_t_ws_floats(n, r, o, k), device=g.device, dtype=torch.float32)
        sl = slice(lo, lo + n)
        call("e4s_grouped_linear_t_f32", fptr(g[sl]), fptr(w), fptr(out[sl]), fptr(ws), n, r, o, k, float(scale),
             fptr(base[sl]) if base is not None else None, fptr(mul[sl]) if mul is not None else None,
             fptr(ref[sl]) if ref is not None else None, float(alpha), stream())
    return out


# the style-gradient tails of the generator backward batched over the layers (E4S_STYLE_GRAD_MULTI=0: one chain per layer, for A/B runs)
STYLE_GRAD_MULTI = os.environ.get("E4S_STYLE_GRAD_MULTI", "1") != "0"


def style_grad_multi(jobs, b, r, nl, sdim, device):
    """The style-gradient tail of the generator backward for every layer in two launches (e4s_style_grad_multi_f32).
    jobs: dicts in the order their layers' gradients arrive, each
        StyledConv: ds_raw [G,Cin], dd_d [G,Cout], d [G,Cout], s [G,Cin], wsq [Cout,Cin]
        ToRGB:      dws [G,3,Cin], w3 [3,Cin], conv_scale
        both:       wmod [Cin,S], mod_scale, slot, masked
    Returns (dlat [B,R,NL,S], [ds_total [G,Cin] per job]): dL/ds per layer including the demodulation path, dL/dlatent with every
    layer's contribution in its slot (jobs of one slot added in job order)."""
    if len(jobs) > lib.STYLE_GRAD_MAX_JOBS:
        raise RuntimeError(f"{len(jobs)} style-gradient jobs: the ABI carries at most {lib.STYLE_GRAD_MAX_JOBS}")
    arr = (lib.StyleGradJob * max(len(jobs), 1))()
    ws = torch.empty(sum(j["G"] * j["Cin"] for j in jobs), device=device, dtype=torch.float32)
    outs, keep, off = [], [], 0
    for q, j in zip(arr, jobs):
        n = j["G"] * j["Cin"]
        out = ws[off:off + n].view(j["G"], j["Cin"])
        off += n
        outs.append(out)
        rgb = "dws" in j
        for name in (("dws", "w3") if rgb else ("ds_raw", "dd_d", "d", "s", "wsq")) + ("wmod",):
            t = _f32(j[name])
            keep.append(t)
            setattr(q, name, fptr(t).value)
        q.ds_total = fptr(out).value
        q.conv_scale = float(j.get("conv_scale", 0.0))
        q.mod_scale = float(j["mod_scale"])
        q.G, q.Cin, q.Cout, q.slot, q.masked = j["G"], j["Cin"], j.get("Cout", 0), j["slot"], int(j["masked"])
    dlat = torch.empty(b, r, nl, sdim, device=device, dtype=torch.float32)
    call("e4s_style_grad_multi_f32", ctypes.cast(arr, ctypes.c_void_p), len(jobs), fptr(dlat), b, r, nl, sdim, stream())
    return dlat, outs


def grouped_outer(g, h, scale):
    """dw[r,o,k] = scale * sum_b g[b,r,o] * h[b,r,k]."""
    b, r, o = g.shape
    k = h.shape[2]
    dw = torch.empty(r, o, k, device=g.device, dtype=torch.float32)
    call("e4s_grouped_outer_f32", fptr(g), fptr(h), fptr(dw), b, r, o, k, float(scale), stream())
    return dw


def batch_sum(x):
    """sum over dim 0 of a contiguous [B, ...] tensor."""
    x = _f32(x)
    out = torch.empty(x.shape[1:], device=x.device, dtype=torch.float32)
    call("e4s_batch_sum_f32", fptr(x), fptr(out), x.shape[0], out.numel(), stream())
    return out


def colsum(x):
    """[C] = sum over every dim but the last of a contiguous channels-last tensor (ordered two-level reduction)."""
    x = _f32(x)
    c = x.shape[-1]
    rows = x.numel() // c
    if rows <= 64 or c % 4 or c > 1024:
        return batch_sum(x.view(rows, c))
    out = torch.empty(c, device=x.device, dtype=torch.float32)
    ws = torch.empty(lib.load().e4s_colsum_ws_floats(rows, c), device=x.device, dtype=torch.float32)
    call("e4s_colsum_f32", fptr(x), fptr(out), fptr(ws), rows, c, stream())
    return out


def sum_all(x):
    """0-dim sum of every element on the native ordered two-level column sum (bit-reproducible).  Also the reason it exists: ATen's large
    reductions allocate a semaphore buffer and clear it with hipMemsetAsync -- captured into a HIP graph that is a MEMSET NODE, and memset
    nodes misbehave on replay on this ROCm (round 3: the region plan's memsets faulted, profiles/r03a_plan_fault_ab.json; round 5: a
    captured train step with `gz.sum((0, 1, 2))` in it came back with its loss scalar zeroed, profiles/r05_graphed_trainG_bisect.json).
    Nothing this library captures issues a memset."""
    x = _f32(x)
    n = x.numel()
    if n % 4 == 0 and n // 4 > 64:
        return colsum(x.view(-1, 4)).sum()                 # the last 4 values: a single-block ATen reduce (no semaphores)
    return x.sum()


def adam_step(p, grad, m, v, lr, beta1, beta2, eps, weight_decay, step):
    """torch.optim.Adam's update of one fp32 tensor, in place, as ONE kernel."""
    call("e4s_adam_step_f32", fptr(p), fptr(_f32(grad)), fptr(m), fptr(v), p.numel(), float(lr), float(beta1), float(beta2),
         float(eps), float(weight_decay), int(step), stream())


def _ptr_array(tensors, dtype=torch.float32):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        if t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
            raise RuntimeError(f"multi-tensor call: contiguous {dtype} ROCm tensors expected")
        arr[i] = t.data_ptr()
    return arr


def advance_steps(steps):
    """steps (device int64, any shape) += 1 in one launch."""
    if steps.dtype != torch.int64 or not steps.is_cuda:
        raise RuntimeError("advance_steps: device int64 tensor")
    call("e4s_advance_i64", ptr(steps), steps.numel(), stream())


def adam_step_dev(p, grad, m, v, lr, beta1, beta2, eps, weight_decay, step, lr_dev=None):
    """adam_step with the step count (already advanced: the step being taken) in a device int64[1] tensor and, optionally, the
    learning rate in a device float64[1] tensor: capturable in a HIP graph."""
    if step.dtype != torch.int64 or not step.is_cuda:
        raise RuntimeError("adam_step_dev: step must be a device int64 tensor")
    if lr_dev is not None and (lr_dev.dtype != torch.float64 or not lr_dev.is_cuda):
        raise RuntimeError("adam_step_dev: lr_dev must be a device float64 tensor")
    call("e4s_adam_step_dev_f32", fptr(p), fptr(_f32(grad)), fptr(m), fptr(v), p.numel(), float(lr), ptr(lr_dev), float(beta1),
         float(beta2), float(eps), float(weight_decay), ptr(step), stream())


def adam_multi_dev(ps, grads, ms, vs, steps, lr, beta1, beta2, eps, weight_decay, lr_dev=None):
    """adam_step_dev for lists of tensors: ceil(len / 48) launches (pointers travel in the kernel arguments)."""
    n = len(ps)
    if not (n == len(grads) == len(ms) == len(vs) == len(steps)):
        raise RuntimeError("adam_multi_dev: list lengths differ")
    if lr_dev is not None and (lr_dev.dtype != torch.float64 or not lr_dev.is_cuda):
        raise RuntimeError("adam_multi_dev: lr_dev must be a device float64 tensor")
    for p, g in zip(ps, grads):
        if g.shape != p.shape:
            raise RuntimeError("adam_multi_dev: gradient shape differs from its parameter's")
    sizes = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
    call("e4s_adam_multi_dev_f32", n, _ptr_array(ps), _ptr_array(grads), _ptr_array(ms), _ptr_array(vs), sizes,
         _ptr_array(steps, torch.int64), float(lr), ptr(lr_dev), float(beta1), float(beta2), float(eps), float(weight_decay), stream())


def _multi_sizes(name, ps, grads, *states, lr_dev=None):
    n = len(ps)
    if len(grads) != n or any(len(s) != n for s in states):
        raise RuntimeError(f"{name}: list lengths differ")
    if lr_dev is not None and (lr_dev.dtype != torch.float64 or not lr_dev.is_cuda):
        raise RuntimeError(f"{name}: lr_dev must be a device float64 tensor")
    for p, g in zip(ps, grads):
        if g.shape != p.shape:
            raise RuntimeError(f"{name}: gradient shape differs from its parameter's")
    for s in states:
        for p, t in zip(ps, s):
            if t.numel() != p.numel():
                raise RuntimeError(f"{name}: a state tensor's size differs from its parameter's")
    return n, (ctypes.c_int64 * n)(*[p.numel() for p in ps])


def sgd_multi_dev(ps, grads, bufs, lr, momentum, dampening, weight_decay, lr_dev=None):
    """torch.optim.SGD's update (nesterov=False) of lists of tensors: ceil(len / 48) launches, capturable.  bufs: the momentum buffers
    (zeros before the first step), or None with momentum == 0."""
    if (momentum != 0) != (bufs is not None):
        raise RuntimeError("sgd_multi_dev: momentum buffers come with momentum != 0, and only then")
    n, sizes = _multi_sizes("sgd_multi_dev", ps, grads, *(() if bufs is None else (bufs,)), lr_dev=lr_dev)
    call("e4s_sgd_multi_dev_f32", n, _ptr_array(ps), _ptr_array(grads), None if bufs is None else _ptr_array(bufs), sizes, float(lr),
         ptr(lr_dev), float(momentum), float(dampening), float(weight_decay), stream())


def adamax_multi_dev(ps, grads, ms, us, steps, lr, beta1, beta2, eps, weight_decay, lr_dev=None):
    """torch.optim.Adamax's update of lists of tensors: ceil(len / 48) launches, capturable.  steps: device int64[1] tensors, already
    advanced; ms / us: exp_avg / exp_inf."""
    n, sizes = _multi_sizes("adamax_multi_dev", ps, grads, ms, us, lr_dev=lr_dev)
    if len(steps) != n:
        raise RuntimeError("adamax_multi_dev: list lengths differ")
    call("e4s_adamax_multi_dev_f32", n, _ptr_array(ps), _ptr_array(grads), _ptr_array(ms), _ptr_array(us), sizes,
         _ptr_array(steps, torch.int64), float(lr), ptr(lr_dev), float(beta1), float(beta2), float(eps), float(weight_decay), stream())


def scalar_log(srcs, step, log):
    """log[step - 1, j] = srcs[j] for up to 16 one-element fp32 device tensors, `step` a device int64[1] (the step being taken, >= 1)
    and `log` a contiguous fp32 [rows, len(srcs)]: one launch, no host sync; a step outside 1 .. rows writes nothing."""
    if len(srcs) > 16:
        raise RuntimeError("scalar_log: at most 16 scalars per launch")
    if step.dtype != torch.int64 or not step.is_cuda or step.numel() != 1:
        raise RuntimeError("scalar_log: step must be a one-element device int64 tensor")
    if log.dtype != torch.float32 or not log.is_cuda or not log.is_contiguous() or log.dim() != 2 or log.shape[1] != len(srcs):
        raise RuntimeError(f"scalar_log: log must be a contiguous device float32 [rows,{len(srcs)}] tensor")
    for s in srcs:
        if s.numel() != 1:
            raise RuntimeError("scalar_log: the sources are one-element tensors")
    call("e4s_scalar_log_f32", len(srcs), _ptr_array(srcs), ptr(step), fptr(log), log.shape[0], stream())


def ranger_ws_floats(sizes, row_lens):
    """Floats of row-sum workspace ranger_multi_dev needs for tensors of `sizes` elements whose centralised rows are `row_lens` long
    (0: the tensor's gradient is not centralised)."""
    n = len(sizes)
    if n != len(row_lens):
        raise RuntimeError("ranger_ws_floats: list lengths differ")
    need = lib.load().e4s_ranger_multi_ws_floats(n, (ctypes.c_int64 * n)(*sizes), (ctypes.c_int64 * n)(*row_lens))
    if need < 0:
        raise RuntimeError("ranger_ws_floats: a row length must be 0 or divide its tensor's size")
    return int(need)


def ranger_multi_dev(ps, grads, ms, vs, slows, row_lens, steps, ws, lr, beta1, beta2, eps, weight_decay, alpha, k, nsma_threshold,
                     lr_dev=None):
    """One Ranger step (src/training/ranger.py:78-164) of lists of tensors: 2 * ceil(len / 40) launches, capturable.  steps: device
    int64[1] tensors, already advanced; row_lens: length of a centralised row per tensor or 0; ws: fp32 workspace of at least
    ranger_ws_floats(...) floats (may be None when nothing is centralised).  The gradients are only read."""
    n = len(ps)
    if not (n == len(grads) == len(ms) == len(vs) == len(slows) == len(row_lens) == len(steps)):
        raise RuntimeError("ranger_multi_dev: list lengths differ")
    if lr_dev is not None and (lr_dev.dtype != torch.float64 or not lr_dev.is_cuda):
        raise RuntimeError("ranger_multi_dev: lr_dev must be a device float64 tensor")
    if ws is not None and (ws.dtype != torch.float32 or not ws.is_cuda or not ws.is_contiguous()):
        raise RuntimeError("ranger_multi_dev: ws must be a contiguous device float32 tensor")
    for p, g in zip(ps, grads):
        if g.shape != p.shape:
            raise RuntimeError("ranger_multi_dev: gradient shape differs from its parameter's")
    sizes = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
    rows = (ctypes.c_int64 * n)(*[int(r) for r in row_lens])
    call("e4s_ranger_multi_dev_f32", n, _ptr_array(ps), _ptr_array(grads), _ptr_array(ms), _ptr_array(vs), _ptr_array(slows), sizes, rows,
         _ptr_array(steps, torch.int64), ptr(ws), 0 if ws is None else ws.numel(), float(lr), ptr(lr_dev), float(beta1), float(beta2),
         float(eps), float(weight_decay), float(alpha), int(k), float(nsma_threshold), stream())


def ema_multi_(dsts, srcs, decay):
    """dst <- dst * decay + src * (1 - decay) for lists of tensors: ceil(len / 48) launches; version counters advance."""
    n = len(dsts)
    if n != len(srcs):
        raise RuntimeError("ema_multi_: list lengths differ")
    for d, s_ in zip(dsts, srcs):
        if d.shape != s_.shape:
            raise RuntimeError("ema_multi_: shapes differ")
    sizes = (ctypes.c_int64 * n)(*[d.numel() for d in dsts])
    call("e4s_ema_multi_f32", n, _ptr_array(dsts), _ptr_array(srcs), sizes, float(decay), stream())
    torch.autograd.graph.increment_version(dsts)         # raw-pointer writes: keep (data_ptr, _version) pack keys honest


def ema_(dst, src, decay):
    """dst <- dst * decay + src * (1 - decay) in place (torch_utils.accumulate, one launch per tensor)."""
    if dst.dtype != torch.float32 or src.dtype != torch.float32 or dst.shape != src.shape or not dst.is_contiguous():
        raise RuntimeError("ema_: contiguous fp32 tensors of one shape")
    call("e4s_ema_f32", fptr(dst), fptr(src.contiguous()), dst.numel(), float(decay), stream())
    torch.autograd.graph.increment_version(dst)          # raw-pointer write: keep (data_ptr, _version) pack keys honest
    return dst


LAST_WGRAD_PATH = 0            # which kernel the last conv_wgrad launch took (e4s_conv_wgrad_path)


def conv_wgrad(gz, x, *, ntaps=9, istride=1, anchors=None, ostride=1, phase=(0, 0), s=None, d=None, labels=None,
               num_regions=1, tap_shift=0):
    """dw [ntaps, Cout, Cin] of a 3x3 / 1x1 conv (see e4s_conv_wgrad_f32): gz NHWC [B,Ho,Wo,Cout], x NHWC [B,Hi,Wi,Cin].
    anchors default to the output grid (ostride 1) / the input grid (polyphase phase, ostride 2)."""
    b, ho, wo, cout = gz.shape
    _, hi, wi, cin = x.shape
    if anchors is None:
        anchors = (ho // ostride, wo // ostride)
    dw = torch.empty(ntaps, cout, cin, device=x.device, dtype=torch.float32)
    p = ConvWgradParams()
    p.gz, p.x, p.dw, p.s, p.d = fptr(_f32(gz)), fptr(x), fptr(dw), fptr(s), fptr(d)
    if labels is not None:
        p.labels, p.Hm, p.Wm, p.R = ptr(labels), labels.shape[1], labels.shape[2], num_regions
    else:
        p.labels, p.Hm, p.Wm, p.R = None, 0, 0, 1
    p.B, p.Hi, p.Wi, p.Cin, p.Ha, p.Wa, p.Ho, p.Wo, p.Cout = b, hi, wi, cin, anchors[0], anchors[1], ho, wo, cout
    p.istride, p.ostride, p.py, p.px, p.ntaps = istride, ostride, phase[0], phase[1], ntaps
    p.tap_shift = int(tap_shift)
    p.ws = None
    global LAST_WGRAD_PATH
    LAST_WGRAD_PATH = lib.load().e4s_conv_wgrad_path(ctypes.byref(p))          # 1: split-bf16 kernel, 0: exact-fp32 kernel (tests)
    ws = torch.empty(lib.load().e4s_conv_wgrad_ws_floats(ctypes.byref(p)), device=x.device, dtype=torch.float32)
    p.ws = fptr(ws)
    call("e4s_conv_wgrad_f32", ctypes.byref(p), stream())
    return dw


# ---- encoder backward (config 5) -------------------------------------------------------------------
def instnorm_bwd(dy, x, stats, gate=None, dx_acc=None):
    """InstanceNorm2d backward (x NHWC [B,H,W,C], stats from instnorm_stats; gate [B,C] = the SE gate that multiplied the
    normalised tensor, or None).  Returns (dx (accumulated into dx_acc if given), sums [B,C,2] = {sum dy, sum dy*xhat})."""
    b, h, w, c = x.shape
    sums = torch.empty(b, c, 2, device=x.device, dtype=torch.float32)
    dx = dx_acc if dx_acc is not None else torch.empty_like(x)
    ws = torch.empty(lib.load().e4s_instnorm_bwd_ws_doubles(b, h * w, c), device=x.device, dtype=torch.float64)
    call("e4s_instnorm_bwd_f32", fptr(_f32(dy)), fptr(x), fptr(stats), fptr(gate), fptr(sums), fptr(dx), ptr(ws), b, h * w, c,
         1 if dx_acc is not None else 0, stream())
    return dx, sums


def prelu(u, slope):
    y = torch.empty_like(u)
    call("e4s_prelu_f32", fptr(u), fptr(slope), fptr(y), u.numel() // u.shape[-1], u.shape[-1], stream())
    return y


def prelu_bwd(dy, u, slope):
    """(du, dslope [C]) of y = PReLU(u), u NHWC [..., C]."""
    c = u.shape[-1]
    npix = u.numel() // c
    du = torch.empty_like(u)
    dslope = torch.empty(c, device=u.device, dtype=torch.float32)
    ws = torch.empty(lib.load().e4s_prelu_bwd_ws_floats(npix, c), device=u.device, dtype=torch.float32)
    call("e4s_prelu_bwd_f32", fptr(_f32(dy)), fptr(u), fptr(slope), fptr(du), fptr(dslope), fptr(ws), npix, c, stream())
    return du, dslope


def pixel_unshuffle2(x):
    """NHWC [B,2H,2W,C] -> [B,H,W,4C]: channel (py*2+px)*C + c of pixel (a, b) = x[2a+py, 2b+px, c]."""
    b, h2, w2, c = x.shape
    if h2 % 2 or w2 % 2 or c % 4:
        raise RuntimeError("pixel_unshuffle2: even H, W and C % 4 == 0")
    out = torch.empty(b, h2 // 2, w2 // 2, 4 * c, device=x.device, dtype=torch.float32)
    call("e4s_pixel_unshuffle2_f32", fptr(_f32(x)), fptr(out), b, h2 // 2, w2 // 2, c, stream())
    return out


def strided_scatter(src, s, out=None):
    """out[b, y*s, x*s] (+)= src[b, y, x]; src NHWC [B,H,W,C].  out=None: a zero-inserted [B,H*s,W*s,C] tensor."""
    b, h, w, c = src.shape
    acc = 1 if out is not None else 0
    if out is None:
        out = torch.empty(b, h * s, w * s, c, device=src.device, dtype=torch.float32)
    call("e4s_strided_scatter_f32", fptr(_f32(src)), fptr(out), b, h, w, c, int(s), acc, stream())
    return out


def strided_place(src, s, oy, ox, out_hw):
    """[B,Ho,Wo,C] with out[b, y*s+oy, x*s+ox] = src[b, y, x] and zeros elsewhere."""
    b, h, w, c = src.shape
    out = torch.empty(b, out_hw[0], out_hw[1], c, device=src.device, dtype=torch.float32)
    call("e4s_strided_place_f32", fptr(_f32(src)), fptr(out), b, h, w, c, int(s), int(oy), int(ox), out_hw[0], out_hw[1],
         stream())
    return out


def torgb_bwd_w(drgb, x):
    """dws[b,c,ci] = sum_p drgb[b,c,p] * x[b,p,ci] (drgb NCHW [B,3,H,W], x NHWC [B,H,W,C]) -> [B,3,C]."""
    b, h, w, c = x.shape
    dws = torch.empty(b, 3, c, device=x.device, dtype=torch.float32)
    L = lib.load()
    scratch = torch.empty(L.e4s_reduce_parts_ws_floats(L.e4s_seg_reduce_nsplit(b, h, w, c), dws.numel()), device=x.device,
                          dtype=torch.float32)
    call("e4s_torgb_bwd_w_f32", fptr(_f32(drgb)), fptr(x), None, 0, 0, 1, fptr(dws), fptr(scratch), b, h, w, c, stream())
    return dws


def region_mean_bwd(dcodes, labels, num_regions, shape, off, dfeat_acc=None):
    """dfeat[b,p,c] (+)= dcodes[b, label(p), off + c] / count[b, label(p)];  shape = (B,H,W,C) of the feature map."""
    b, h, w, c = shape
    dfeat = dfeat_acc if dfeat_acc is not None else torch.empty(b, h, w, c, device=dcodes.device, dtype=torch.float32)
    counts = torch.empty(b * num_regions, device=dcodes.device, dtype=torch.int32)
    dcodes = _f32(dcodes)
    call("e4s_region_mean_bwd_f32", fptr(dcodes), ptr(labels), labels.shape[1], labels.shape[2], ptr(counts), fptr(dfeat),
         b, h, w, c, num_regions, dcodes.shape[2], int(off), 1 if dfeat_acc is not None else 0, stream())
    return dfeat


# ---- GPEN FullGenerator / Discriminator support ------------------------------------------------
def conv1x1_small(x_nchw, w, bias, scale, act=0, alpha=0.2, gain=LRELU_GAIN, out=None):
    """x NCHW [B,Cin<=4,H,W]; w [Cout,Cin] -> NHWC [B,H,W,Cout] = act(x.w*scale + bias)."""
    x = _f32(x_nchw)
    b, cin, h, wd = x.shape
    cout = w.shape[0]
    y = torch.empty(b, h, wd, cout, device=x.device, dtype=torch.float32) if out is None else out
    call("e4s_conv1x1_small_f32", fptr(x), fptr(_f32(w)), fptr(bias), fptr(y), b, h * wd, cin, cout, y.shape[3],
         float(scale), int(act), float(alpha), float(gain), stream())
    return y


def noise_half(feat, noise_w, bias, out, coff, alpha=0.2, gain=LRELU_GAIN):
    """out[..., coff:coff+C] = lrelu(noise_w*feat + bias)*gain; feat NHWC [B,H,W,C], out NHWC [B,H,W,Cy]."""
    b, h, w, c = feat.shape
    call("e4s_noise_half_f32", fptr(feat), fptr(noise_w), fptr(bias), fptr(out), b * h * w, c, out.shape[3], int(coff),
         float(alpha), float(gain), stream())
    return out


def pixelnorm(x):
    x = _f32(x)
    y = torch.empty_like(x)
    call("e4s_pixelnorm_f32", fptr(x), fptr(y), x.shape[0], x.shape[1], stream())
    return y


def add_scale(a, b, scale):
    out = torch.empty_like(a)
    call("e4s_add_scale_f32", fptr(a), fptr(b), fptr(out), float(scale), a.numel(), stream())
    return out


def minibatch_stddev(x, cy, group):
    """x NHWC [B,H,W,C] -> NHWC [B,H,W,cy] = [x | group stddev statistic | zeros]."""
    b, h, w, c = x.shape
    y = torch.empty(b, h, w, cy, device=x.device, dtype=torch.float32)
    call("e4s_minibatch_stddev_f32", fptr(x), fptr(y), b, h * w, c, cy, int(group), stream())
    return y


def upfirdn2d_nhwc(x, kernel, up=1, down=1, pad=(0, 0)):
    """upfirdn2d on an NHWC activation: the op's native [major, H, W, minor] view with major = B, minor = C."""
    return upfirdn2d_raw(x, kernel, up, up, down, down, pad[0], pad[1], pad[0], pad[1])


# ---- backward (generator) --------------------------------------------------------------------
def pack_taps_bwd(w_fwd, out=None):
    """forward-packed [ncls,9,Cout,Cin] -> backward layout [ncls,9,Cin,Cout] (taps flipped)."""
    ncls, taps, cout, cin = w_fwd.shape
    assert taps == 9
    wt = _into(out, (ncls, 9, cin, cout), w_fwd.device)
    call("e4s_pack_taps_bwd_f32", fptr(w_fwd), fptr(wt), ncls, cout, cin, stream())
    return wt


def conv_bwd(gz, wt, x, s, d, labels, num_regions, ncls, want_ds=True):
    """gz NHWC [B,Hy,Wy,Cy]; wt [ncls,9,Cx,Cy]; x NHWC [B,Hx,Wx,Cx] -> (dx like x, ds [G,Cx] or None)."""
    b, hy, wy, cy = gz.shape
    _, hx, wx, cx = x.shape
    dx = torch.empty_like(x)
    want_ds = want_ds and s is not None
    ds = torch.empty(s.shape[0], cx, device=x.device, dtype=torch.float32) if want_ds else None
    p = ConvBwdParams()
    p.gz, p.wt, p.dx, p.x, p.ds, p.s, p.d = fptr(gz), fptr(wt), fptr(dx), fptr(x), fptr(ds), fptr(s), fptr(d)
    if labels is not None:
        p.labels, p.Hm, p.Wm, p.R = ptr(labels), labels.shape[1], labels.shape[2], num_regions
    else:
        p.labels, p.Hm, p.Wm, p.R = None, 0, 0, 1
    p.B, p.Hx, p.Wx, p.Cx, p.Hy, p.Wy, p.Cy, p.ncls = b, hx, wx, cx, hy, wy, cy, ncls
    # partial sums of ds (and of dx where the tap groups are split over blocks), added in order by the entry point
    nws = lib.load().e4s_conv_bwd_ws_floats(ctypes.byref(p))
    ws = torch.empty(nws, device=x.device, dtype=torch.float32) if nws else None
    p.ds_ws = fptr(ws)
    call("e4s_conv_bwd_mfma_f32", ctypes.byref(p), stream())
    return dx, ds


def region_scale(gz, d, labels, num_regions, ncls=1):
    """u = gz * d[region of the output pixel] (e4s_region_scale_f32): gz NHWC [B,Ho,Wo,C], d [B*R,C], labels uint8 [B,Hm,Wm].
    ncls == 1: u like gz.  ncls == 4 (polyphase up-conv, Ho = 2H): u [4,B,H,W,C], one contiguous map per output phase."""
    gz = _f32(gz)
    b, ho, wo, c = gz.shape
    if ncls == 4:
        if ho % 2 or wo % 2:
            raise RuntimeError("region_scale: the polyphase form needs an even output grid")
        h, w = ho // 2, wo // 2
        u = torch.empty(4, b, h, w, c, device=gz.device, dtype=torch.float32)
    else:
        h, w = ho, wo
        u = torch.empty_like(gz)
    call("e4s_region_scale_f32", fptr(gz), fptr(_f32(d)), ptr(labels), labels.shape[1], labels.shape[2], int(num_regions), fptr(u),
         b, h, w, c, int(ncls), stream())
    return u


def col2im_region_ok(c):
    return c % 4 == 0 and 4 <= c <= 1024 and 256 % (c // 4) == 0


SCATTER_DGRAD = os.environ.get("E4S_SCATTER_DGRAD", "1") != "0"


SCATTER_DGRAD_MAX_BYTES = int(os.environ.get("E4S_SCATTER_DGRAD_MAX_BYTES", str(6 << 30)))      # 6 GiB: batch 2 of the 1024^2 generator's largest masked layer is 2.4 GB


def scatter_dgrad_wanted(b, h, w, cy, cx):
    """Policy of the scatter-form input gradient of a masked StyledConv (x [b,h,w,cx] -> cy channels; for an up-conv h, w are the INPUT
    grid and one launch runs per output phase): a 1x1 split-bf16 contraction [b h w, cy] x [cy, 9 cx] on the gather kernel (256-row x
    128-column tiles) + e4s_col2im_region_f32.  `auto`: where that launch fills the chip, `bf16x3`: wherever the kernels apply, `f32`: never
    (the exact-fp32 dx + ds kernel)."""
    if not SCATTER_DGRAD or PRECISION == "f32" or cy % 32 or (9 * cx) % 128 or not col2im_region_ok(cx):
        return False
    if 4 * b * h * w * 9 * cx * 4 > SCATTER_DGRAD_MAX_BYTES:          # the product tensor G [ncls <= 4, b, h, w, 9 cx] fp32 (a captured step's pool keeps it)
        return False                                                    # -> the exact-fp32 dx + ds kernel, which needs no scratch
    if PRECISION == "bf16x3":
        return True
    return (b * h * w + 255) // 256 * ((9 * cx) // 128) >= BF16X3_MIN_BLOCKS


def col2im_region(G, x, s, labels, num_regions, ncls=1):
    """(dx, ds) of a masked StyledConv from the scatter-form products (e4s_col2im_region_f32): G [ncls,B,H,W,9*C] (tap-major columns: the 1x1
    contraction of u with the tap-stacked weights), x NHWC [B,H,W,C] the layer's input, s [B*R,C] -> dx like x, ds like s."""
    b, h, w, c = x.shape
    if G.numel() != ncls * b * h * w * 9 * c or not G.is_contiguous() or not x.is_contiguous():
        raise RuntimeError("col2im_region: G must be contiguous [ncls,B,H,W,9*C] for x [B,H,W,C]")
    r = int(num_regions)
    dx = torch.empty_like(x)
    ds = torch.empty(b * r, c, device=x.device, dtype=torch.float32)
    L = lib.load()
    nsplit = L.e4s_col2im_region_nsplit(b, h, w, c)
    if nsplit <= 0:
        raise RuntimeError("col2im_region: unsupported channel count")
    ws = torch.empty(L.e4s_reduce_parts_ws_floats(nsplit, ds.numel()), device=x.device, dtype=torch.float32)
    call("e4s_col2im_region_f32", fptr(G), fptr(x), fptr(_f32(s)), ptr(labels), labels.shape[1], labels.shape[2], r, fptr(dx), fptr(ds),
         fptr(ws), b, h, w, c, int(ncls), stream())
    return dx, ds


def scale_dot(u, x, s):
    """u, x NHWC [B,H,W,C]; s [B,C]: u <- u * s[b] in place (returned) and ds[b,c] = sum_p x * u (the unscaled u), ordered sums."""
    b, h, w, c = u.shape
    assert u.is_contiguous() and x.is_contiguous() and x.shape == u.shape and s.shape == (b, c)
    ds = torch.empty(b, c, device=u.device, dtype=torch.float32)
    ws = torch.empty(lib.load().e4s_scale_dot_ws_floats(b, h * w, c), device=u.device, dtype=torch.float32)
    call("e4s_scale_dot_f32", fptr(u), fptr(x), fptr(s), fptr(ds), fptr(ws), b, h * w, c, stream())
    return u, ds


def act_bwd_demod(dy, y, noise, noise_w, bias, alpha, gain, labels, num_regions):
    """(gz, dd): gz = dy * lrelu'(y) * gain (fused_bias_act(dy, None, y, 3, 1, alpha, gain)) and dd = demod_grad(gz, y, ...) in ONE pass
    over dy and y (e4s_act_bwd_demod_f32); None when the channel count is outside the kernel's set."""
    b, h, w, c = dy.shape
    if c % 4 or c > 1024 or c < 4 or 256 % (c // 4) or not dy.is_contiguous() or not y.is_contiguous():
        return None
    r = num_regions if labels is not None else 1
    gz = torch.empty_like(dy)
    dd = torch.empty(b * r, c, device=dy.device, dtype=torch.float32)
    hm = wm = 0
    if labels is not None:
        hm, wm = labels.shape[1:]
    nb = 0
    if noise is not None:
        nb = h * w if noise.shape[0] > 1 else 0
    L = lib.load()
    ws = torch.empty(L.e4s_reduce_parts_ws_floats(L.e4s_act_bwd_demod_nsplit(b, h, w, c), dd.numel()), device=dy.device, dtype=torch.float32)
    call("e4s_act_bwd_demod_f32", fptr(_f32(dy)), fptr(y), fptr(gz), fptr(noise), fptr(noise_w) if noise is not None else None, nb,
         fptr(bias), float(alpha), float(gain), ptr(labels), hm, wm, r, fptr(dd), fptr(ws), b, h, w, c, stream())
    return gz, dd


def demod_grad(gz, y, noise, noise_w, bias, alpha, gain, labels, num_regions):
    """dL/dd [G, C] for out_pre = d * c (see e4s_demod_grad_f32); the caller divides by d."""
    b, h, w, c = gz.shape
    r = num_regions if labels is not None else 1
    dd = torch.empty(b * r, c, device=gz.device, dtype=torch.float32)
    hm = wm = 0
    if labels is not None:
        hm, wm = labels.shape[1:]
    nb = 0
    if noise is not None:
        nb = h * w if noise.shape[0] > 1 else 0
    L = lib.load()
    ws = torch.empty(L.e4s_reduce_parts_ws_floats(L.e4s_seg_reduce_nsplit(b, h, w, c), dd.numel()), device=gz.device,
                     dtype=torch.float32)
    call("e4s_demod_grad_f32", fptr(gz), fptr(y), fptr(noise), fptr(noise_w) if noise is not None else None, nb,
         fptr(bias), float(alpha), float(gain), ptr(labels), hm, wm, r, fptr(dd), fptr(ws), b, h, w, c, stream())
    return dd


def torgb_bwd(drgb, x, ws, labels, num_regions, dx_acc=None):
    """drgb NCHW [B,3,H,W]; x NHWC; ws [G,3,C] -> (dx NHWC (accumulated into dx_acc if given), dws [G,3,C])."""
    b, h, w, c = x.shape
    r = num_regions if labels is not None else 1
    hm = wm = 0
    if labels is not None:
        hm, wm = labels.shape[1:]
    dws = torch.empty(b * r, 3, c, device=x.device, dtype=torch.float32)
    drgb = _f32(drgb)
    L = lib.load()
    scratch = torch.empty(L.e4s_reduce_parts_ws_floats(L.e4s_seg_reduce_nsplit(b, h, w, c), dws.numel()), device=x.device,
                          dtype=torch.float32)
    call("e4s_torgb_bwd_w_f32", fptr(drgb), fptr(x), ptr(labels), hm, wm, r, fptr(dws), fptr(scratch), b, h, w, c, stream())
    acc = 1 if dx_acc is not None else 0
    dx = dx_acc if dx_acc is not None else torch.empty_like(x)
    call("e4s_torgb_bwd_x_f32", fptr(drgb), fptr(ws), ptr(labels), hm, wm, r, fptr(dx), b, h, w, c, acc, stream())
    return dx, dws


def shift_scale(x, tab, labels, num_regions, anchors, istride=1, dy=0, dx=0, os=1, py=0, px=0):
    """out[b,a,c] = tab[group(out pixel of a)][c] * x[b, a*istride + (dy,dx), c] (0 outside); x NHWC."""
    b, hi, wi, c = x.shape
    ha, wa = anchors
    out = torch.empty(b, ha, wa, c, device=x.device, dtype=torch.float32)
    hm = wm = 0
    if labels is not None:
        hm, wm = labels.shape[1:]
    call("e4s_shift_scale_f32", fptr(x), fptr(tab), ptr(labels), hm, wm, num_regions if labels is not None else 1,
         fptr(out), b, ha, wa, hi, wi, c, istride, dy, dx, os, py, px, stream())
    return out


# ---- loss networks (csrc/criteria.hip) -------------------------------------------------------------------------
def adaptive_pool(x, out_hw, crop=None, in_nchw=True, scale=None, shift=None):
    """F.adaptive_avg_pool2d of x[:, :, y0:y0+hc, x0:x0+wc] (+ per-channel affine) -> NHWC [B,Ho,Wo,C]."""
    x = _f32(x)
    if in_nchw:
        b, c, hi, wi = x.shape
    else:
        b, hi, wi, c = x.shape
    y0, x0, hc, wc = crop if crop is not None else (0, 0, hi, wi)
    ho, wo = out_hw
    y = torch.empty(b, ho, wo, c, device=x.device, dtype=torch.float32)
    call("e4s_adaptive_pool_f32", fptr(x), fptr(y), b, c, hi, wi, y0, x0, hc, wc, ho, wo, 1 if in_nchw else 0,
         fptr(scale), fptr(shift), stream())
    return y


def adaptive_pool_bwd(dy, in_shape, crop=None, in_nchw=True, scale=None, dx_acc=None):
    """gradient of adaptive_pool w.r.t. its input (shape in_shape, the input's layout); accumulated into dx_acc if given."""
    if in_nchw:
        b, c, hi, wi = in_shape
    else:
        b, hi, wi, c = in_shape
    y0, x0, hc, wc = crop if crop is not None else (0, 0, hi, wi)
    ho, wo = dy.shape[1:3]
    dx = dx_acc if dx_acc is not None else torch.empty(in_shape, device=dy.device, dtype=torch.float32)
    call("e4s_adaptive_pool_bwd_f32", fptr(_f32(dy)), fptr(dx), b, c, hi, wi, y0, x0, hc, wc, ho, wo, 1 if in_nchw else 0,
         fptr(scale), 1 if dx_acc is not None else 0, stream())
    return dx


def pack_smallcin(w):
    """[Cout,Cin,k,k] -> [k*k*Cin, Cout] (tap-major; e4s_conv_smallcin_f32's operand) -- a one-off layout change."""
    cout, cin, k, _ = w.shape
    return w.detach().float().permute(2, 3, 1, 0).reshape(k * k * cin, cout).contiguous()


def conv_smallcin(x, wp, bias, cout, k, stride, pad, relu=False):
    b, hi, wi, cin = x.shape
    ho, wo = (hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1
    y = torch.empty(b, ho, wo, cout, device=x.device, dtype=torch.float32)
    call("e4s_conv_smallcin_f32", fptr(x), fptr(wp), fptr(bias), fptr(y), b, hi, wi, cin, ho, wo, cout, k, stride, pad,
         1 if relu else 0, stream())
    return y


def conv_smallcin_bwd(dy, wp, in_shape, k, stride, pad, cache=None):
    """Image gradient of conv_smallcin.  Large kernels (AlexNet's 11x11 / 4 stem: k*k*Cin >= 128 columns): GEMM form -- ONE 1x1
    contraction z = dy . wp^T on the fp32 MFMA conv kernel + a col2im pass (e4s_conv_smallcin_col2im_f32); small kernels: the per-pixel
    kernel (e4s_conv_smallcin_bwd_f32).  cache: a dict owned by whoever owns `wp` (the module's weight pack), where the zero-padded GEMM
    image of wp is kept -- per pack, not per process: two loss networks alternating no longer evict each other, and a pack that dies takes
    its image with it."""
    b, hi, wi, cin = in_shape
    _, ho, wo, cout = dy.shape
    dx = torch.empty(in_shape, device=dy.device, dtype=torch.float32)
    ncol = k * k * cin
    if ncol >= 128 and cout % 32 == 0 and dy.is_contiguous():
        zc = (ncol + 31) // 32 * 32
        key = (wp.data_ptr(), wp._version, zc)
        hit = cache.get("wz") if cache is not None else None
        if hit is None or hit[0] != key:
            wz = torch.zeros(1, 1, zc, cout, device=wp.device, dtype=torch.float32)
            wz[0, 0, :ncol] = wp                                                  # wp is [k*k*Cin][Cout]: the GEMM's [N][K] matrix
            hit = (key, wz)
            if cache is not None:
                cache["wz"] = hit
        wz = hit[1]
        z = conv_mfma(_f32(dy), wz, zc, ntaps=1, spatial=False)
        call("e4s_conv_smallcin_col2im_f32", fptr(z), fptr(dx), b, hi, wi, cin, ho, wo, zc, k, stride, pad, stream())
        return dx
    call("e4s_conv_smallcin_bwd_f32", fptr(_f32(dy)), fptr(wp), fptr(dx), b, hi, wi, cin, ho, wo, cout, k, stride, pad,
         stream())
    return dx


def maxpool3s2(x):
    b, hi, wi, c = x.shape
    ho, wo = (hi - 3) // 2 + 1, (wi - 3) // 2 + 1
    y = torch.empty(b, ho, wo, c, device=x.device, dtype=torch.float32)
    idx = torch.empty(b, ho, wo, c, device=x.device, dtype=torch.uint8)
    call("e4s_maxpool3s2_f32", fptr(x), fptr(y), ptr(idx), b, hi, wi, c, stream())
    return y, idx


def maxpool3s2_bwd(dy, idx, in_shape):
    b, hi, wi, c = in_shape
    dx = torch.empty(in_shape, device=dy.device, dtype=torch.float32)
    call("e4s_maxpool3s2_bwd_f32", fptr(_f32(dy)), ptr(idx), fptr(dx), b, hi, wi, c, stream())
    return dx


def maxpool2(x):
    b, hi, wi, c = x.shape
    y = torch.empty(b, hi // 2, wi // 2, c, device=x.device, dtype=torch.float32)
    idx = torch.empty(b, hi // 2, wi // 2, c, device=x.device, dtype=torch.uint8)
    call("e4s_maxpool2_f32", fptr(x), fptr(y), ptr(idx), b, hi, wi, c, stream())
    return y, idx


def maxpool2_bwd(dy, idx, in_shape):
    b, hi, wi, c = in_shape
    dx = torch.empty(in_shape, device=dy.device, dtype=torch.float32)
    call("e4s_maxpool2_bwd_f32", fptr(_f32(dy)), ptr(idx), fptr(dx), b, hi, wi, c, stream())
    return dx


def relu_bwd(dy, y, dx_acc=None):
    """dx (+)= dy * [y > 0], from the ReLU's output."""
    dx = dx_acc if dx_acc is not None else torch.empty_like(y)
    call("e4s_relu_bwd_f32", fptr(_f32(dy)), fptr(y), fptr(dx), y.numel(), 1 if dx_acc is not None else 0, stream())
    return dx


def lpips_layer(fx, fy, w):
    """[B] = spatial mean of the lin-weighted squared distance of the unit-normalised features (NHWC)."""
    b, h, wd, c = fx.shape
    out = torch.empty(b, device=fx.device, dtype=torch.float32)
    ws = torch.empty(lib.load().e4s_lpips_layer_ws_doubles(b, h * wd), device=fx.device, dtype=torch.float64)
    call("e4s_lpips_layer_f32", fptr(fx), fptr(fy), fptr(w), fptr(out), ptr(ws), b, h * wd, c, stream())
    return out


def lpips_layer_bwd(fx, fy, w, gout, gmul, dfx_acc=None):
    """dfx (+)= gout[0] * gmul * d(sum_b lpips_layer[b]) / d(fx)."""
    b, h, wd, c = fx.shape
    dfx = dfx_acc if dfx_acc is not None else torch.empty_like(fx)
    call("e4s_lpips_layer_bwd_f32", fptr(fx), fptr(fy), fptr(w), fptr(gout), float(gmul), fptr(dfx), b, h * wd, c,
         1 if dfx_acc is not None else 0, stream())
    return dfx


def instnorm_bwd_sums(dy, x, stats):
    """[B,C,2] = {sum_p dy, sum_p dy * (x - mean) * rstd} (ordered)."""
    b, h, w, c = x.shape
    sums = torch.empty(b, c, 2, device=x.device, dtype=torch.float32)
    ws = torch.empty(lib.load().e4s_instnorm_bwd_ws_doubles(b, h * w, c), device=x.device, dtype=torch.float64)
    call("e4s_instnorm_bwd_sums_f32", fptr(_f32(dy)), fptr(x), fptr(stats), fptr(sums), ptr(ws), b, h * w, c, stream())
    return sums


def norm_bwd_frozen(dy, stats, gate=None, extra=None, dx_acc=None):
    """dx (+)= rstd * (gate * dy + extra): backward of a normalisation whose statistics are constants."""
    b, h, w, c = dy.shape
    dx = dx_acc if dx_acc is not None else torch.empty_like(dy)
    call("e4s_norm_bwd_frozen_f32", fptr(_f32(dy)), fptr(stats), fptr(gate), fptr(extra), fptr(dx), b, h * w, c,
         1 if dx_acc is not None else 0, stream())
    return dx


def cosine(a, b):
    """rows of a, b [B, D] -> [B,3] = {cos, alpha, beta}, d(cos)/da = alpha*b + beta*a."""
    n, d = a.shape[0], a.numel() // a.shape[0]
    out = torch.empty(n, 3, device=a.device, dtype=torch.float32)
    ws = torch.empty(lib.load().e4s_cosine_ws_doubles(n, d), device=a.device, dtype=torch.float64)
    call("e4s_cosine_f32", fptr(a), fptr(b), fptr(out), ptr(ws), n, d, stream())
    return out


def cosine_bwd(a, b, coef, gout, gmul, da_acc=None):
    n, d = a.shape[0], a.numel() // a.shape[0]
    da = da_acc if da_acc is not None else torch.empty_like(a)
    call("e4s_cosine_bwd_f32", fptr(a), fptr(b), fptr(coef), fptr(gout), float(gmul), fptr(da), n, d,
         1 if da_acc is not None else 0, stream())
    return da


# ---- VGG16 Gram-matrix StyleLoss (csrc/gram.hip) ----------------------------------------------------------------
def style_prep(x, mask, out_hw, normalize):
    """NCHW image [B,3,H,W] (+ mask [B,1,Hm,Wm] or None) -> NHWC [B,oh,ow,3]: bilinear resize, ImageNet normalisation, times the
    bilinearly resized mask (style_loss.py:143-170)."""
    x = _f32(x)
    b, c, h, w = x.shape
    if c != 3:
        raise ValueError(f"style_prep: a 3-channel image, got {c} channels")
    hm, wm = _style_mask(mask, b)
    oh, ow = out_hw
    y = torch.empty(b, oh, ow, 3, device=x.device, dtype=torch.float32)
    call("e4s_style_prep_f32", fptr(x), fptr(mask), fptr(y), b, h, w, hm, wm, oh, ow, 1 if normalize else 0, stream())
    return y


def _style_mask(mask, b):
    if mask is None:
        return 0, 0
    if mask.dim() != 4 or mask.shape[0] != b or mask.shape[1] != 1 or mask.dtype != torch.float32 or not mask.is_contiguous():
        raise ValueError(f"style_prep: the mask is a contiguous fp32 [B,1,Hm,Wm] tensor, got {tuple(mask.shape)} {mask.dtype}")
    return mask.shape[2], mask.shape[3]


def style_prep_bwd(dy, mask, in_shape, normalize):
    """The transpose of style_prep's linear map: dy NHWC [B,oh,ow,3] -> dx NCHW in_shape."""
    b, c, h, w = in_shape
    hm, wm = _style_mask(mask, b)
    oh, ow = dy.shape[1:3]
    dx = torch.empty(in_shape, device=dy.device, dtype=torch.float32)
    call("e4s_style_prep_bwd_f32", fptr(_f32(dy)), fptr(mask), fptr(dx), b, h, w, hm, wm, oh, ow, 1 if normalize else 0, stream())
    return dx


def gram(f):
    """NHWC tap [N,H,W,C] -> G [NC,NC] = F F^T / (N H W C) over the [N C, H W] view of the batch (style_loss.py:213-221)."""
    n, h, w, c = f.shape
    nws = lib.load().e4s_gram_ws_floats(n, h * w, c)
    if nws <= 0:
        raise ValueError(f"gram: C % 64 == 0 and N C <= 16384, got N {n}, C {c}")
    g = torch.empty(n * c, n * c, device=f.device, dtype=torch.float32)
    ws = torch.empty(nws, device=f.device, dtype=torch.float32)
    call("e4s_gram_f32", fptr(f), fptr(g), fptr(ws), n, h * w, c, stream())
    return g


def gram_mse(gx, gy, acc, weight, init=False):
    """-> (term [1] = mean((gx - gy)^2), D = gx - gy); acc[0] (+)= weight * term (init: acc[0] = weight * term)."""
    d = torch.empty_like(gx)
    term = torch.empty(1, device=gx.device, dtype=torch.float32)
    ws = torch.empty(lib.load().e4s_gram_mse_ws_doubles(gx.numel()), device=gx.device, dtype=torch.float64)
    call("e4s_gram_mse_f32", fptr(gx), fptr(gy), fptr(d), fptr(term), fptr(acc), float(weight), 1 if init else 0, ptr(ws), gx.numel(), stream())
    return term, d


def gram_grad(f, d, gloss, coef, addend=None):
    """dF[n,p,c] = addend + coef * gloss[0] * sum_j A[p][j] D[j][n C + c] (A the Gram's operand, D symmetric)."""
    n, h, w, c = f.shape
    df = torch.empty_like(f)
    call("e4s_gram_grad_f32", fptr(f), fptr(d), fptr(gloss), float(coef), fptr(addend), fptr(df), n, h * w, c, stream())
    return df


# ---- BiSeNet face parser (face_parser.py) ---------------------------------------------------
def parser_preprocess(src, taps):
    """uint8 NHWC [B,H,W,3] or fp32 NCHW [B,3,H,W] in [0,1] -> the parser's input NHWC [B,H/2,W/2,3]: bicubic /2 (reflect),
    clamp(0,1), ImageNet normalisation.  taps: the 8 host-side filter taps (a sequence of floats)."""
    if src.dtype == torch.uint8:
        b, h, w, c = src.shape
        is_u8 = 1
    else:
        src = _f32(src)
        b, c, h, w = src.shape
        is_u8 = 0
    if c != 3:
        raise RuntimeError(f"parser_preprocess: 3-channel images, got shape {tuple(src.shape)}")
    y = torch.empty(b, h // 2, w // 2, 3, device=src.device, dtype=torch.float32)
    k = (ctypes.c_float * 8)(*[float(t) for t in taps])
    call("e4s_parser_preprocess_f32", ptr(src.contiguous()), is_u8, fptr(y), b, h, w, k, stream())
    return y


def maxpool3s2p1(x):
    """nn.MaxPool2d(3, 2, padding=1) of x NHWC."""
    x = _f32(x)
    b, hi, wi, c = x.shape
    y = torch.empty(b, (hi - 1) // 2 + 1, (wi - 1) // 2 + 1, c, device=x.device, dtype=torch.float32)
    call("e4s_maxpool3s2p1_f32", fptr(x), fptr(y), b, hi, wi, c, stream())
    return y


def add_relu(a, r=None, out=None, coff=0):
    """relu(a + r) of NHWC maps (r None: relu(a)), into `out` (a wider NHWC map: channels coff .. coff+C) when given."""
    a = _f32(a)
    c = a.shape[-1]
    npix = a.numel() // c
    if out is None:
        out = torch.empty_like(a)
    elif tuple(out.shape[:-1]) != tuple(a.shape[:-1]) or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError("add_relu(out=...): a contiguous fp32 NHWC map with the pixels of a")
    call("e4s_add_relu_f32", fptr(a), fptr(_f32(r)) if r is not None else None, fptr(out), npix, c, out.shape[-1], coff, stream())
    return out


def mean_hw(x):
    """x NHWC [B,H,W,C] -> [B,C] spatial mean."""
    x = _f32(x)
    b, c = x.shape[0], x.shape[-1]
    out = torch.empty(b, c, device=x.device, dtype=torch.float32)
    call("e4s_mean_hw_f32", fptr(x), fptr(out), b, x.numel() // (b * c), c, stream())
    return out


def parser_fc(v, w, bias, act=0, offset=0.0):
    """act(v @ w.T + bias) + offset on [B,Ci] (w [Co,Ci], or None: identity); act 0 none, 1 ReLU, 2 sigmoid."""
    v = _f32(v)
    b, ci = v.shape
    co = w.shape[0] if w is not None else ci
    out = torch.empty(b, co, device=v.device, dtype=torch.float32)
    call("e4s_parser_fc_f32", fptr(v), fptr(_f32(w)) if w is not None else None, fptr(_f32(bias)) if bias is not None else None,
         fptr(out), b, ci, co, int(act), float(offset), stream())
    return out


def gate_add_up2(x, gate, add):
    """nearest x2 of (x * gate[:, None, None] + add): x NHWC [B,h,w,C], gate [B,C], add [B,C] or NHWC [B,h,w,C]."""
    x = _f32(x)
    b, h, w, c = x.shape
    add = _f32(add)
    add_map = 1 if add.dim() == 4 else 0
    if tuple(add.shape) != ((b, h, w, c) if add_map else (b, c)) or tuple(gate.shape) != (b, c):
        raise RuntimeError("gate_add_up2: gate [B,C], add [B,C] or [B,h,w,C]")
    y = torch.empty(b, 2 * h, 2 * w, c, device=x.device, dtype=torch.float32)
    call("e4s_gate_add_up2_f32", fptr(x), fptr(_f32(gate)), fptr(add), add_map, fptr(y), b, h, w, c, stream())
    return y


def parser_head(logits, ncls, size, seg12=False, labels=True, onehot=False, nchw=False):
    """Bilinear (align_corners=True) upsampling of NHWC logits [B,h,w,>=ncls] to size (H, W) + first-maximum argmax.
    Returns (labels uint8 [B,H,W] | None, one-hot fp32 [B,12|ncls,H,W] | None, logits NCHW [B,ncls,H,W] | None)."""
    logits = _f32(logits)
    b, h, w, cs = logits.shape
    hh, ww = size
    dev = logits.device
    lab = torch.empty(b, hh, ww, device=dev, dtype=torch.uint8) if labels else None
    oh = torch.empty(b, 12 if seg12 else ncls, hh, ww, device=dev, dtype=torch.float32) if onehot else None
    nc = torch.empty(b, ncls, hh, ww, device=dev, dtype=torch.float32) if nchw else None
    call("e4s_parser_head_f32", fptr(logits), b, h, w, ncls, cs, hh, ww, 1 if seg12 else 0, ptr(lab), fptr(oh), fptr(nc), stream())
    return lab, oh, nc


# ---- Real-ESRNet x4 super-resolution (sr.py) ------------------------------------------------
def sr_f32():
    """Whether the dense-block conv runs on the exact fp32 MFMA (PRECISION "f32"); "bf16x3" and "auto" take the split-bf16 path."""
    return PRECISION == "f32"


def rrdb_pack(w, f32):
    """nn.Conv2d weight [32,Cin,3,3] -> the opaque image e4s_rrdb_conv_f32 reads ([Cin/32][9][32][128 bytes], fp32-typed)."""
    w = _f32(w)
    cout, cin, kh, kw = w.shape
    if cout != 32 or kh != 3 or kw != 3 or cin % 32:
        raise RuntimeError(f"rrdb_pack: a [32, 32k, 3, 3] weight, got {tuple(w.shape)}")
    nbytes = lib.load().e4s_rrdb_pack_bytes(cin)
    out = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
    call("e4s_rrdb_pack_f32", fptr(w), ptr(out), cin, 0 if f32 else 1, stream())
    return out


def _slice32(t, coff, what):
    """(pointer, channel stride) of an fp32 NHWC buffer whose 32 channels at coff are read or written in place."""
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4 or coff < 0 or coff + 32 > t.shape[-1]:
        raise RuntimeError(f"rrdb_conv({what}): a contiguous fp32 NHWC buffer with 32 channels at offset {coff}")
    return fptr(t), t.shape[-1]


def rrdb_conv(x, cin, w_pack, bias, y, y_coff=0, *, epilogue=0, r0=None, r0_coff=0, s0=1.0, r1=None, r1_coff=0, s1=1.0, up2=False,
              slope=0.2, f32=None):
    """Dense-block 3x3 conv: the first cin channels of the NHWC buffer x -> 32 channels at y_coff of the NHWC buffer y (which may
    be x itself when y_coff >= cin).  epilogue 0: LeakyReLU(slope); 1: acc * s0 + r0; 2: (acc * s0 + r0) * s1 + r1 (r0 / r1: the 32
    channels at r*_coff of NHWC buffers at the output resolution).  up2: x is read through a nearest x2 upsampling.  Writes y in
    place and returns it."""
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 4:
        raise RuntimeError("rrdb_conv: x is a contiguous fp32 NHWC buffer")
    b, hi, wi, xcs = x.shape
    ho, wo = (2 * hi, 2 * wi) if up2 else (hi, wi)
    yp, ycs = _slice32(y, y_coff, "y")
    if tuple(y.shape[:3]) != (b, ho, wo):
        raise RuntimeError(f"rrdb_conv: y must hold {(b, ho, wo)} pixels, got {tuple(y.shape[:3])}")
    p = lib.RrdbParams()
    p.x, p.w, p.bias, p.y = fptr(x), fptr(w_pack), fptr(_f32(bias)), yp
    p.B, p.Hi, p.Wi, p.Cin = b, hi, wi, cin
    p.x_cstride, p.y_cstride, p.y_coff = xcs, ycs, y_coff
    for name, r, coff in (("r0", r0, r0_coff), ("r1", r1, r1_coff)):
        if r is not None:
            rp, rcs = _slice32(r, coff, name)
            if tuple(r.shape[:3]) != (b, ho, wo):
                raise RuntimeError(f"rrdb_conv: {name} must hold {(b, ho, wo)} pixels")
            setattr(p, name, rp)
            setattr(p, name + "_cstride", rcs)
            setattr(p, name + "_coff", coff)
    p.epilogue, p.up2, p.precision = int(epilogue), 1 if up2 else 0, 1 if (sr_f32() if f32 is None else f32) else 0
    p.s0, p.s1, p.slope = float(s0), float(s1), float(slope)
    call("e4s_rrdb_conv_f32", ctypes.byref(p), stream())
    return y


def rrdb_head(src, wp, bias, y, y2=None, flip=False):
    """conv_first: uint8 NHWC [B,H,W,3] (x / 255) or fp32 NCHW [B,3,H,W] -> channels [0, 32) of the NHWC buffers y (and y2)."""
    if src.dtype == torch.uint8:
        b, h, w, c = src.shape
        is_u8 = 1
    else:
        src = _f32(src)
        b, c, h, w = src.shape
        is_u8 = 0
    if c != 3:
        raise RuntimeError(f"rrdb_head: 3-channel images, got shape {tuple(src.shape)}")
    for t in (y, y2):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape[:3]) != (b, h, w)):
            raise RuntimeError("rrdb_head: y / y2 are contiguous fp32 NHWC buffers with the image's pixels")
    call("e4s_rrdb_head_f32", ptr(src.contiguous()), is_u8, 1 if flip else 0, fptr(_f32(wp)), fptr(_f32(bias)), fptr(y), y.shape[-1],
         fptr(y2), y2.shape[-1] if y2 is not None else 0, b, h, w, stream())
    return y


def rrdb_tail(x, wp, bias, *, u8=False, nchw=True, flip=False):
    """conv_last on the first 32 channels of NHWC x: the fp32 result (NCHW or NHWC, before any clamp), or with u8 the uint8 HWC
    image round_half_even(clamp(v, 0, 1) * 255) (channel order reversed with flip)."""
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 4:
        raise RuntimeError("rrdb_tail: x is a contiguous fp32 NHWC buffer")
    b, h, w, cs = x.shape
    if u8:
        out = torch.empty(b, h, w, 3, device=x.device, dtype=torch.uint8)
        yf, yu = None, out
    else:
        out = torch.empty((b, 3, h, w) if nchw else (b, h, w, 3), device=x.device, dtype=torch.float32)
        yf, yu = out, None
    call("e4s_rrdb_tail_f32", fptr(x), cs, fptr(_f32(wp)), fptr(_f32(bias)), fptr(yf), 1 if nchw else 0, ptr(yu), 1 if flip else 0,
         b, h, w, stream())
    return out


# ---- GPEN ParseNet (parsenet.py) ------------------------------------------------------------
def pconv_out_size(n, stride=1, up2=False):
    """Output rows of reflect pad 1 + 3x3 at `stride` on n rows (2 n behind a nearest x2 upsampling)."""
    g = 2 * n if up2 else n
    if g < 2:
        raise RuntimeError(f"pconv: reflect padding 1 needs 2 or more rows and columns, got {g}")
    return (g + 2 - 3) // stride + 1


def pconv_pack(w, f32):
    """nn.Conv2d weight [Cout,Cin,3,3] (both multiples of 32) -> the opaque image e4s_pconv_f32 reads, fp32-typed."""
    w = _f32(w)
    cout, cin, kh, kw = w.shape
    nbytes = lib.load().e4s_pconv_pack_bytes(cin, cout)
    if kh != 3 or kw != 3 or nbytes == 0:
        raise RuntimeError(f"pconv_pack: a [32j, 32k, 3, 3] weight, got {tuple(w.shape)}")
    out = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
    call("e4s_pconv_pack_f32", fptr(w), ptr(out), cin, cout, 0 if f32 else 1, stream())
    out.pconv_f32 = bool(f32)                                                # pconv refuses a pack of the other precision
    return out


def _nhwc(t, c, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4 or t.shape[-1] < c:
        raise RuntimeError(f"pconv({what}): a contiguous fp32 NHWC buffer of {c} or more channels")
    return fptr(t), t.shape[-1]


def pconv(x, cin, w_pack, cout, y, *, scale=None, bias=None, lrelu=False, r0=None, r1=None, stride=1, up2=False, slope=0.2, f32=None):
    """Reflect-padded 3x3 conv: the first cin channels of the NHWC buffer x -> the first cout channels of the NHWC buffer y.
    v = acc * scale + bias, LeakyReLU(slope) with lrelu, then + r0, then + r1 (NHWC buffers at the output resolution).  up2: x is
    read through a nearest x2 upsampling (stride 1).  Writes y in place and returns it."""
    xp, xcs = _nhwc(x, cin, "x")
    b, hi, wi, _ = x.shape
    if up2 and stride != 1:
        raise RuntimeError("pconv: up2 goes with stride 1")
    ho, wo = pconv_out_size(hi, stride, up2), pconv_out_size(wi, stride, up2)
    p = lib.PconvParams()
    p.y, p.y_cstride = _nhwc(y, cout, "y")
    if tuple(y.shape[:3]) != (b, ho, wo):
        raise RuntimeError(f"pconv: y must hold {(b, ho, wo)} pixels, got {tuple(y.shape[:3])}")
    f32 = sr_f32() if f32 is None else bool(f32)
    want = lib.load().e4s_pconv_pack_bytes(cin, cout)
    if want == 0 or w_pack.dtype != torch.float32 or w_pack.numel() * 4 != want or getattr(w_pack, "pconv_f32", f32) != f32:
        raise RuntimeError(f"pconv: w_pack is not pconv_pack's image of a [{cout},{cin},3,3] weight in this precision")
    for name, t in (("w_pack", w_pack), ("y", y), ("scale", scale), ("bias", bias), ("r0", r0), ("r1", r1)):
        if t is not None and t.device != x.device:
            raise RuntimeError(f"pconv: {name} is on {t.device}, x on {x.device}")
    p.x, p.w, p.x_cstride = xp, fptr(w_pack), xcs
    for name, v in (("scale", scale), ("bias", bias)):
        if v is not None:
            if v.numel() != cout:
                raise RuntimeError(f"pconv: {name} has {v.numel()} entries for {cout} channels")
            setattr(p, name, fptr(_f32(v)))
    for name, r in (("r0", r0), ("r1", r1)):
        if r is not None:
            rp, rcs = _nhwc(r, cout, name)
            if tuple(r.shape[:3]) != (b, ho, wo):
                raise RuntimeError(f"pconv: {name} must hold {(b, ho, wo)} pixels")
            setattr(p, name, rp)
            setattr(p, name + "_cstride", rcs)
    p.B, p.Hi, p.Wi, p.Cin, p.Cout = b, hi, wi, cin, cout
    p.stride, p.up2, p.lrelu, p.precision = int(stride), 1 if up2 else 0, 1 if lrelu else 0, 1 if f32 else 0
    p.slope = float(slope)
    call("e4s_pconv_f32", ctypes.byref(p), stream())
    return y


def parsenet_head(src, wp, bias, y, flip=False):
    """The first conv: uint8 NHWC [B,H,W,3] (x / 255 * 2 - 1) or fp32 NCHW [B,3,H,W] -> the NHWC buffer y [B,H,W,Cout]."""
    if src.dtype == torch.uint8:
        b, h, w, c = src.shape
        is_u8 = 1
    else:
        src = _f32(src)
        b, c, h, w = src.shape
        is_u8 = 0
    if c != 3:
        raise RuntimeError(f"parsenet_head: 3-channel images, got shape {tuple(src.shape)}")
    cout = wp.shape[-1]
    if y.dtype != torch.float32 or not y.is_contiguous() or tuple(y.shape) != (b, h, w, cout) or tuple(wp.shape) != (27, cout):
        raise RuntimeError("parsenet_head: y is a contiguous fp32 NHWC buffer [B,H,W,Cout], wp [27,Cout]")
    call("e4s_parsenet_head_f32", ptr(src.contiguous()), is_u8, 1 if flip else 0, fptr(_f32(wp)), fptr(_f32(bias)), fptr(y), cout,
         b, h, w, stream())
    return y


def parsenet_tail(x, cin, wp, bias, *, mask=True, labels=False, logits=False):
    """out_mask_conv on the first cin channels of NHWC x, wp [9,cin,20] -> (mask uint8 [B,H,W] of 0 / 255, labels uint8 [B,H,W],
    logits fp32 [B,19,H,W]); what is not asked for is None."""
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 4 or tuple(wp.shape) != (9, cin, 20) or bias.numel() != 19:
        raise RuntimeError("parsenet_tail: x is a contiguous fp32 NHWC buffer, wp [9,Cin,20], bias [19]")
    b, h, w, cs = x.shape
    dev = x.device
    m = torch.empty(b, h, w, device=dev, dtype=torch.uint8) if mask else None
    lab = torch.empty(b, h, w, device=dev, dtype=torch.uint8) if labels else None
    lg = torch.empty(b, 19, h, w, device=dev, dtype=torch.float32) if logits else None
    call("e4s_parsenet_tail_f32", fptr(x), cs, cin, fptr(_f32(wp)), fptr(_f32(bias)), ptr(m), ptr(lab), fptr(lg), b, h, w, stream())
    return m, lab, lg


# ---- RetinaFace-R50 face detector (retinaface.py) ------------------------------------------
def rconv_out_size(n, k, stride=1):
    """Output rows of a zero-padded (k / 2) k x k conv at `stride` on n rows: ceil(n / stride) for k = 1 and 3."""
    return (n + 2 * (k // 2) - k) // stride + 1


def rconv_pack(w, f32):
    """nn.Conv2d weight [Cout,Cin,k,k] (Cin % 32 == 0, Cout % 64 == 0, k 1 or 3) -> the opaque image e4s_rconv_f32 reads."""
    w = _f32(w)
    cout, cin, kh, kw = w.shape
    nbytes = lib.load().e4s_rconv_pack_bytes(cin, cout, kh) if kh == kw else 0
    if nbytes == 0:
        raise RuntimeError(f"rconv_pack: a [64j, 32k, 1|3, 1|3] weight, got {tuple(w.shape)}")
    out = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
    call("e4s_rconv_pack_f32", fptr(w), ptr(out), cin, cout, kh, 0 if f32 else 1, stream())
    out.rconv_f32 = bool(f32)                                                # rconv refuses a pack of the other precision
    out.rconv_shape = (cout, cin, kh)
    return out


def rconv(x, cin, w_pack, cout, k, y, *, y_coff=0, bias=None, act=False, slope=0.0, r0=None, r0_after=False, stride=1, f32=None):
    """Zero-padded k x k conv (k 1 or 3): the first cin channels of the NHWC buffer x -> channels y_coff .. y_coff + cout of the NHWC
    buffer y.  v = acc + bias; + r0 (r0_after False); LeakyReLU(slope) with act (slope 0: ReLU); + r0 (r0_after True).  r0: an NHWC
    map at the output resolution, or a smaller one that is read through a nearest upsampling to it.  Writes y in place."""
    xp, xcs = _nhwc(x, cin, "x")
    b, hi, wi, _ = x.shape
    ho, wo = rconv_out_size(hi, k, stride), rconv_out_size(wi, k, stride)
    p = lib.RconvParams()
    p.y, p.y_cstride = _nhwc(y, y_coff + cout, "y")
    if tuple(y.shape[:3]) != (b, ho, wo):
        raise RuntimeError(f"rconv: y must hold {(b, ho, wo)} pixels, got {tuple(y.shape[:3])}")
    f32 = sr_f32() if f32 is None else bool(f32)
    if getattr(w_pack, "rconv_shape", None) != (cout, cin, k) or getattr(w_pack, "rconv_f32", None) != f32:
        raise RuntimeError(f"rconv: w_pack is not rconv_pack's image of a [{cout},{cin},{k},{k}] weight in this precision")
    for name, t in (("w_pack", w_pack), ("y", y), ("bias", bias), ("r0", r0)):
        if t is not None and t.device != x.device:
            raise RuntimeError(f"rconv: {name} is on {t.device}, x on {x.device}")
    p.x, p.w, p.x_cstride, p.y_coff = xp, fptr(w_pack), xcs, int(y_coff)
    if bias is not None:
        if bias.numel() != cout:
            raise RuntimeError(f"rconv: bias has {bias.numel()} entries for {cout} channels")
        p.bias = fptr(_f32(bias))
    if r0 is not None:
        p.r0, p.r0_cstride = _nhwc(r0, cout, "r0")
        if r0.shape[0] != b:
            raise RuntimeError("rconv: r0 has another batch size")
        if tuple(r0.shape[1:3]) != (ho, wo):
            p.r0_H, p.r0_W = r0.shape[1], r0.shape[2]
        p.r0_mode = 2 if r0_after else 1
    p.B, p.Hi, p.Wi, p.Cin, p.Cout = b, hi, wi, cin, cout
    p.k, p.stride, p.act, p.precision, p.slope = int(k), int(stride), 1 if act else 0, 1 if f32 else 0, float(slope)
    call("e4s_rconv_f32", ctypes.byref(p), stream())
    return y


def retina_prep(frames_u8, out, scale=1.0):
    """uint8 BGR [B,H,W,3] -> out fp32 [B,Hd,Wd,3] minus (104, 117, 123); Hd x Wd other than H x W: a half-pixel bilinear resize
    first, source coordinate (d + 0.5) * scale - 0.5."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3 or not frames_u8.is_contiguous():
        raise RuntimeError("retina_prep: contiguous uint8 frames [B,H,W,3]")
    b, h, w, _ = frames_u8.shape
    if out.dtype != torch.float32 or out.dim() != 4 or out.shape[0] != b or out.shape[-1] != 3 or not out.is_contiguous():
        raise RuntimeError("retina_prep: out is a contiguous fp32 buffer [B,Hd,Wd,3]")
    call("e4s_retina_prep_f32", ptr(frames_u8), fptr(out), b, h, w, out.shape[1], out.shape[2], float(scale), stream())
    return out


def retina_stem(x, wp, bias, y):
    """The 7x7 stride-2 stem (BatchNorm folded, ReLU) on e4s_conv_smallcin_f32, into the caller's buffer y."""
    b, hi, wi, cin = x.shape
    _, ho, wo, cout = y.shape
    if (ho, wo) != ((hi + 6 - 7) // 2 + 1, (wi + 6 - 7) // 2 + 1) or y.shape[0] != b or not y.is_contiguous():
        raise RuntimeError("retina_stem: y holds the stride-2 output of x")
    call("e4s_conv_smallcin_f32", fptr(_f32(x)), fptr(_f32(wp)), fptr(_f32(bias)), fptr(y), b, hi, wi, cin, ho, wo, cout, 7, 2, 3, 1, stream())
    return y


def retina_pool(x, y):
    """nn.MaxPool2d(3, 2, padding=1) of NHWC x into the caller's buffer y (e4s_maxpool3s2p1_f32)."""
    b, hi, wi, c = x.shape
    if tuple(y.shape) != (b, (hi - 1) // 2 + 1, (wi - 1) // 2 + 1, c) or not y.is_contiguous():
        raise RuntimeError("retina_pool: y holds the stride-2 output of x")
    call("e4s_maxpool3s2p1_f32", fptr(_f32(x)), fptr(y), b, hi, wi, c, stream())
    return y


def retina_geom(im_h, im_w, resize=1.0, steps=(8, 16, 32), min_sizes=((16, 32), (64, 128), (256, 512))):
    """The prior grid of an im_h x im_w network input (prior_box.py:14): lib.RetinaGeom."""
    g = lib.RetinaGeom()
    g.imH, g.imW, g.nlevel, g.resize = int(im_h), int(im_w), len(steps), float(resize)
    base = 0
    for l, st in enumerate(steps):
        g.lh[l], g.lw[l], g.step[l], g.base[l] = -(-im_h // st), -(-im_w // st), st, base
        g.min_size[l][0], g.min_size[l][1] = float(min_sizes[l][0]), float(min_sizes[l][1])
        base += g.lh[l] * g.lw[l] * 2
    g.N = base
    return g


def retina_head(x, wp, bias, geom, level, boxes, scores, landms, raw=None):
    """One level's fused heads + softmax + prior + decode: x NHWC [B,lh,lw,>=256] -> that level's rows of boxes [B,N,4], scores
    [B,N], landms [B,N,10] (and of raw = (loc, conf, landms) when given)."""
    xp, xcs = _nhwc(x, 256, "x")
    b = x.shape[0]
    if tuple(x.shape[1:3]) != (geom.lh[level], geom.lw[level]) or tuple(wp.shape) != (256, 32) or bias.numel() != 32:
        raise RuntimeError("retina_head: x is the level's map, wp [256,32], bias [32]")
    for t, shp in ((boxes, (b, geom.N, 4)), (scores, (b, geom.N)), (landms, (b, geom.N, 10))):
        if tuple(t.shape) != shp or not t.is_contiguous():
            raise RuntimeError(f"retina_head: an output is not a contiguous {shp} buffer")
    rl, rc, rm = raw if raw is not None else (None, None, None)
    if raw is not None and (tuple(rl.shape) != (b, geom.N, 4) or tuple(rc.shape) != (b, geom.N, 2) or tuple(rm.shape) != (b, geom.N, 10)):
        raise RuntimeError("retina_head: raw = (loc [B,N,4], conf [B,N,2], landms [B,N,10])")
    call("e4s_retina_head_f32", xp, xcs, fptr(_f32(wp)), fptr(_f32(bias)), ctypes.byref(geom), int(level), b, fptr(boxes), fptr(scores),
         fptr(landms), fptr(rl), fptr(rc), fptr(rm), stream())


def retina_decode(loc, conf, lm, geom, boxes, scores, landms):
    """prior + decode + scaling of the network's raw outputs loc [B,N,4], conf [B,N,2] (softmaxed), lm [B,N,10]."""
    b = loc.shape[0]
    for t, shp in ((loc, (b, geom.N, 4)), (conf, (b, geom.N, 2)), (lm, (b, geom.N, 10)), (boxes, (b, geom.N, 4)), (scores, (b, geom.N)),
                   (landms, (b, geom.N, 10))):
        if tuple(t.shape) != shp:
            raise RuntimeError(f"retina_decode: expected a {shp} tensor, got {tuple(t.shape)}")
    call("e4s_retina_decode_f32", fptr(_f32(loc)), fptr(_f32(conf)), fptr(_f32(lm)), ctypes.byref(geom), b, fptr(boxes), fptr(scores),
         fptr(landms), stream())


def retina_select(boxes, landms, sorted_scores, sorted_idx, conf_thr, nms_thr, top_k, keep_top_k, ss, dets, lm_out, counts):
    """Threshold, top_k, greedy NMS, keep_top_k and the landmark re-layout on score-sorted candidates: -> dets [B,K,5], lm_out
    [B,K,10], counts int32 [B]."""
    b, n, _ = boxes.shape
    if sorted_idx.dtype != torch.int64 or counts.dtype != torch.int32 or tuple(dets.shape) != (b, keep_top_k, 5) \
            or tuple(lm_out.shape) != (b, keep_top_k, 10) or tuple(sorted_scores.shape) != (b, n) or tuple(sorted_idx.shape) != (b, n):
        raise RuntimeError("retina_select: sorted_idx int64 [B,N], counts int32 [B], dets [B,K,5], lm_out [B,K,10]")
    call("e4s_retina_select_f32", fptr(boxes), fptr(landms), fptr(sorted_scores), ptr(sorted_idx), b, n, float(conf_thr), float(nms_thr),
         int(top_k), int(keep_top_k), float(ss), fptr(dets), fptr(lm_out), ptr(counts), stream())


# ---- pasting restored faces into a frame (face_paste.py) --------------------------------------
def warp_affine(src, inv, out_hw):
    """OpenCV's warpAffine (bilinear, constant border 0) of a uint8 [H,W,3] or fp32 [H,W] image; inv: the six doubles of the inverse
    map (a00, a01, b0, a10, a11, b1), destination -> source."""
    hd, wd = int(out_hw[0]), int(out_hw[1])
    if src.dtype == torch.uint8 and src.dim() == 3 and src.shape[2] == 3:
        dst, is_f32 = torch.empty(hd, wd, 3, device=src.device, dtype=torch.uint8), 0
    elif src.dtype == torch.float32 and src.dim() == 2:
        dst, is_f32 = torch.empty(hd, wd, device=src.device, dtype=torch.float32), 1
    else:
        raise RuntimeError(f"warp_affine: a uint8 [H,W,3] or fp32 [H,W] image, got {tuple(src.shape)} {src.dtype}")
    a = [float(v) for v in inv]
    if len(a) != 6:
        raise RuntimeError("warp_affine: six coefficients")
    call("e4s_warp_affine", ptr(src.contiguous()), ptr(dst), is_f32, src.shape[0], src.shape[1], hd, wd, *a, stream())
    return dst


def mask_prep(mask_u8, thres):
    """uint8 [B,H,W] -> fp32 mask / 255 with a frame of thres pixels zeroed."""
    if mask_u8.dtype != torch.uint8 or mask_u8.dim() != 3:
        raise RuntimeError("mask_prep: uint8 [B,H,W] masks")
    b, h, w = mask_u8.shape
    out = torch.empty(b, h, w, device=mask_u8.device, dtype=torch.float32)
    call("e4s_mask_prep_f32", ptr(mask_u8.contiguous()), fptr(out), b, h, w, int(thres), stream())
    return out


def blur_pass(x, taps, axis, out=None):
    """One pass of a separable filter over fp32 [B,H,W] along x (axis 1) or y (axis 0), BORDER_REFLECT_101."""
    x = _f32(x)
    if x.dim() != 3 or taps.dim() != 1 or taps.device != x.device:
        raise RuntimeError("blur_pass: fp32 [B,H,W] maps and a 1-D tap tensor on the same device")
    out = torch.empty_like(x) if out is None else out
    b, h, w = x.shape
    call("e4s_blur_pass_f32", fptr(x), fptr(out), fptr(_f32(taps)), taps.numel(), b, h, w, int(axis), stream())
    return out


def binomial3_u8(x):
    """cv2.filter2D with [1 2 1] x [1 2 1] / 16 on uint8 [B,H,W,C]."""
    if x.dtype != torch.uint8 or x.dim() != 4:
        raise RuntimeError("binomial3_u8: uint8 [B,H,W,C] images")
    x = x.contiguous()
    out = torch.empty_like(x)
    b, h, w, c = x.shape
    call("e4s_binomial3_u8", ptr(x), ptr(out), b, h, w, c, stream())
    return out


def merge_blend(masks, faces, bg, out=None):
    """masks fp32 [n,H,W], faces uint8 [n,H,W,3] (both warped into the frame), bg uint8 [H,W,3] -> the blended frame (out may be bg)."""
    if bg.dtype != torch.uint8 or bg.dim() != 3 or bg.shape[2] != 3 or not bg.is_contiguous():
        raise RuntimeError("merge_blend: bg is a contiguous uint8 [H,W,3] frame")
    h, w, _ = bg.shape
    n = 0 if masks is None else masks.shape[0]
    if n and (tuple(masks.shape) != (n, h, w) or tuple(faces.shape) != (n, h, w, 3) or masks.dtype != torch.float32
              or faces.dtype != torch.uint8 or masks.device != bg.device or faces.device != bg.device):
        raise RuntimeError("merge_blend: masks fp32 [n,H,W] and faces uint8 [n,H,W,3] at the frame's size and on its device")
    out = torch.empty_like(bg) if out is None else out
    if tuple(out.shape) != tuple(bg.shape) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != bg.device:
        raise RuntimeError("merge_blend: out is a contiguous uint8 frame like bg")
    call("e4s_merge_blend_u8", fptr(masks.contiguous()) if n else None, ptr(faces.contiguous()) if n else None, ptr(bg), ptr(out), n, h, w,
         stream())
    return out


# ---- face-vid2vid keypoints and head pose (reenact.py) -----------------------------------------
def conv3d_pack(w, f32):
    """nn.Conv3d weight [Cout,Cin,3,3,3] (Cin % 32 == 0, any Cout) -> the opaque image e4s_conv3d_f32 reads (Cout padded to 32)."""
    w = _f32(w)
    if w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3):
        raise RuntimeError(f"conv3d_pack: a [Cout, 32k, 3, 3, 3] weight, got {tuple(w.shape)}")
    cout, cin = w.shape[:2]
    nbytes = lib.load().e4s_conv3d_pack_bytes(cin, cout)
    if nbytes == 0:
        raise RuntimeError(f"conv3d_pack: a [Cout, 32k, 3, 3, 3] weight, got {tuple(w.shape)}")
    out = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
    call("e4s_conv3d_pack_f32", fptr(w), ptr(out), cin, cout, 0 if f32 else 1, stream())
    out.conv3d_f32 = bool(f32)                                               # conv3d refuses a pack of the other precision
    out.conv3d_shape = (cout, cin)
    return out


def conv3d(x, w_pack, cout, y, *, bias=None, relu=False, up2=False, f32=None):
    """Zero-padded 3x3x3 conv: x fp32 [B,D,H,W,Cin] with contiguous channels (any other strides: a permuted view is read in place)
    -> the first cout channels of the contiguous y [B,D,Ho,Wo,C].  up2: x is read through the nearest (1, 2, 2) up-sampling.
    v = acc + bias, ReLU with relu.  Writes y in place and returns it."""
    if x.dtype != torch.float32 or x.dim() != 5 or not x.is_cuda or x.stride(4) != 1:
        raise RuntimeError("conv3d: x is an fp32 device volume [B,D,H,W,C] with contiguous channels")
    b, d, hi, wi, cin = x.shape
    ho, wo = (2 * hi, 2 * wi) if up2 else (hi, wi)
    if y.dtype != torch.float32 or y.dim() != 5 or not y.is_contiguous() or tuple(y.shape[:4]) != (b, d, ho, wo) or y.shape[4] < cout:
        raise RuntimeError(f"conv3d: y is a contiguous fp32 volume of {(b, d, ho, wo)} voxels and {cout} or more channels, got {tuple(y.shape)}")
    f32 = sr_f32() if f32 is None else bool(f32)
    if getattr(w_pack, "conv3d_shape", None) != (cout, cin) or getattr(w_pack, "conv3d_f32", None) != f32:
        raise RuntimeError(f"conv3d: w_pack is not conv3d_pack's image of a [{cout},{cin},3,3,3] weight in this precision")
    for name, t in (("w_pack", w_pack), ("y", y), ("bias", bias)):
        if t is not None and t.device != x.device:
            raise RuntimeError(f"conv3d: {name} is on {t.device}, x on {x.device}")
    p = lib.Conv3dParams()
    p.x, p.w, p.y = c_p(x.data_ptr()), fptr(w_pack), fptr(y)
    if bias is not None:
        if bias.numel() != cout:
            raise RuntimeError(f"conv3d: bias has {bias.numel()} entries for {cout} channels")
        p.bias = fptr(_f32(bias))
    p.x_bstride, p.x_dstride, p.x_ystride, p.x_xstride = x.stride(0), x.stride(1), x.stride(2), x.stride(3)
    p.B, p.D, p.Hi, p.Wi, p.Cin, p.Cout = b, d, hi, wi, cin, cout
    p.y_cstride = y.shape[4]
    p.up2, p.relu, p.precision = 1 if up2 else 0, 1 if relu else 0, 1 if f32 else 0
    call("e4s_conv3d_f32", ctypes.byref(p), stream())
    return y


def softargmax3d(logits, temperature, jac=None, channels_last=False, value=None, jacobian=None):
    """KPDetector's head.  logits fp32 [B,K,D,H,W] (or, channels_last, [B,D,H,W,K]); jac: the jacobian maps [B,J*9,D,H,W] (or
    [B,D,H,W,J*9]), J = K or 1 -> (value [B,K,3], jacobian [B,K,3,3] or None).  Sums are taken in an order fixed by (D, H, W)."""
    def strides(t, what):
        if t.dtype != torch.float32 or t.dim() != 5 or not t.is_contiguous() or not t.is_cuda:
            raise RuntimeError(f"softargmax3d: {what} is a contiguous fp32 5-D device tensor")
        if channels_last:
            b, d, h, w, c = t.shape
            return (b, c, d, h, w), (d * h * w * c, 1, c)
        b, c, d, h, w = t.shape
        return (b, c, d, h, w), (c * d * h * w, d * h * w, 1)
    (b, k, d, h, w), ls = strides(logits, "logits")
    dev = logits.device
    value = torch.empty(b, k, 3, device=dev, dtype=torch.float32) if value is None else value
    js, nj = (0, 0, 0), 0
    if jac is not None:
        (jb, jc, jd, jh, jw), js = strides(jac, "jac")
        if (jb, jd, jh, jw) != (b, d, h, w) or jc not in (9, 9 * k):
            raise RuntimeError(f"softargmax3d: jac holds 9 or {9 * k} maps of the logits' volume, got {tuple(jac.shape)}")
        nj = jc // 9
        jacobian = torch.empty(b, k, 3, 3, device=dev, dtype=torch.float32) if jacobian is None else jacobian
    else:
        jacobian = None
    call("e4s_softargmax3d_f32", fptr(logits), ls[0], ls[1], ls[2], fptr(jac), js[0], js[1], js[2], nj, b, k, d, h, w, float(temperature),
         fptr(value), fptr(jacobian), stream())
    return value, jacobian


def aa_down(frames, taps, step, out=None):
    """AntiAliasInterpolation2d at the kept positions: frames [B,H,W,3] fp32 or uint8 (read as x / 255), taps: odd-length fp32 device
    vector of the normalised 1-D Gaussian -> fp32 [B,ceil(H/step),ceil(W/step),3].  One tap of 1.0 at step 1 converts a frame."""
    if frames.dtype not in (torch.float32, torch.uint8) or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise RuntimeError("aa_down: contiguous fp32 or uint8 frames [B,H,W,3]")
    b, h, w, _ = frames.shape
    ho, wo = -(-h // step), -(-w // step)
    out = torch.empty(b, ho, wo, 3, device=frames.device, dtype=torch.float32) if out is None else out
    if tuple(out.shape) != (b, ho, wo, 3) or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError(f"aa_down: out is a contiguous fp32 buffer {(b, ho, wo, 3)}")
    call("e4s_aa_down_f32", ptr(frames), 1 if frames.dtype == torch.uint8 else 0, fptr(out), b, h, w, fptr(taps), taps.numel(), int(step),
         stream())
    return out


def avgpool2(x, y=None):
    """nn.AvgPool2d(2) of NHWC x -> [B,H/2,W/2,C] (odd sizes drop the last row / column)."""
    b, hi, wi, c = x.shape
    y = torch.empty(b, hi // 2, wi // 2, c, device=x.device, dtype=torch.float32) if y is None else y
    if tuple(y.shape) != (b, hi // 2, wi // 2, c) or not y.is_contiguous():
        raise RuntimeError("avgpool2: y holds the floored half-size output of x")
    call("e4s_avgpool2_f32", fptr(_f32(x)), fptr(y), b, hi, wi, c, stream())
    return y


def pose(x, w, bias, nbins, num_kp, out, kp_value=None, kp_jacobian=None, fixed=(None, None, None)):
    """HEEstimator's tail + keypoint_transformation: x NHWC [B,h,w,C], w [3 nbins + 3 + 3 K, C] (rows yaw, pitch, roll, t, exp),
    out: dict of contiguous fp32 buffers raw [B,3 nbins + 3 + 3 K], degrees [B,3], rot [B,3,3], and with kp_value [1|B,K,3] value
    [B,K,3], with kp_jacobian [1|B,K,3,3] jacobian [B,K,3,3].  fixed: (yaw, pitch, roll) degrees that replace the estimate, or None."""
    b, h, ww, c = x.shape
    nout = 3 * nbins + 3 + 3 * num_kp
    if tuple(w.shape) != (nout, c) or bias.numel() != nout or not x.is_contiguous():
        raise RuntimeError(f"pose: w [{nout},{c}], bias [{nout}], x contiguous NHWC")
    p = lib.PoseParams()
    p.x, p.w, p.bias = fptr(x), fptr(w), fptr(bias)
    p.raw, p.degrees, p.rot = fptr(out["raw"]), fptr(out["degrees"]), fptr(out["rot"])
    if out["raw"].numel() != b * nout or out["degrees"].numel() != b * 3 or out["rot"].numel() != b * 9:
        raise RuntimeError("pose: raw / degrees / rot sizes")
    if kp_value is not None:
        if kp_value.shape[0] not in (1, b) or tuple(kp_value.shape[1:]) != (num_kp, 3) or out["value"].numel() != b * num_kp * 3:
            raise RuntimeError("pose: kp_value [1|B,K,3] and value [B,K,3]")
        p.kp_value, p.value, p.kp_batch = fptr(kp_value), fptr(out["value"]), kp_value.shape[0]
        if kp_jacobian is not None:
            if kp_jacobian.shape[0] != kp_value.shape[0] or kp_jacobian.numel() != kp_value.numel() * 3 or out["jacobian"].numel() != b * num_kp * 9:
                raise RuntimeError("pose: kp_jacobian [1|B,K,3,3] and jacobian [B,K,3,3]")
            p.kp_jacobian, p.jacobian = fptr(kp_jacobian), fptr(out["jacobian"])
    elif kp_jacobian is not None:
        raise RuntimeError("pose: kp_jacobian goes with kp_value")
    p.B, p.HW, p.C, p.x_cstride, p.nbins, p.K = b, h * ww, c, c, int(nbins), int(num_kp)
    mask = 0
    for i, (name, v) in enumerate(zip(("yaw", "pitch", "roll"), fixed)):
        if v is not None:
            mask |= 1 << i
            setattr(p, name, float(v))
    p.fixed_mask = mask
    call("e4s_pose_f32", ctypes.byref(p), stream())
    return out


def conv_smallcin_into(x, wp, bias, y, k, stride, pad, relu=False):
    """e4s_conv_smallcin_f32 (a k x k conv of an image of <= 4 channels) into the caller's NHWC buffer y."""
    b, hi, wi, cin = x.shape
    ho, wo = (hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1
    if tuple(y.shape[:3]) != (b, ho, wo) or not y.is_contiguous() or not x.is_contiguous():
        raise RuntimeError(f"conv_smallcin_into: y holds {(b, ho, wo)} pixels")
    call("e4s_conv_smallcin_f32", fptr(x), fptr(wp), fptr(bias), fptr(y), b, hi, wi, cin, ho, wo, y.shape[3], k, stride, pad,
         1 if relu else 0, stream())
    return y


# ---- face-vid2vid dense motion and 3-D feature warp (reenact_warp.py) ---------------------------
def _vol(t, what, c=None):
    """Check an fp32 device volume [B,D,H,W,C] with contiguous channels (any other strides); c: the channels that are read."""
    if t.dtype != torch.float32 or t.dim() != 5 or not t.is_cuda or t.stride(4) != 1 or (c is not None and t.shape[4] < c):
        raise RuntimeError(f"{what}: an fp32 device volume [B,D,H,W,C] with contiguous channels" + (f" (C >= {c})" if c else ""))
    return t


def conv3dx_pack(w, f32, cin_pad=None):
    """nn.Conv3d weight [Cout,Cin,k,k,k] (k 1, 3 or 7; any Cout) -> the opaque image e4s_conv3dx_f32 reads.  cin_pad: the input
    channels are padded with zero columns to this multiple of 32 (Cin 80 -> 96, 112 -> 128: the conv then reads a buffer whose pad
    channels hold zeros)."""
    w = _f32(w)
    if w.dim() != 5 or w.shape[2] != w.shape[3] or w.shape[2] != w.shape[4]:
        raise RuntimeError(f"conv3dx_pack: a [Cout, Cin, k, k, k] weight, got {tuple(w.shape)}")
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    cin_pad = cin if cin_pad is None else int(cin_pad)
    if cin_pad < cin:
        raise RuntimeError(f"conv3dx_pack: cin_pad {cin_pad} is below the weight's {cin} input channels")
    if cin_pad != cin:
        wide = torch.zeros(cout, cin_pad, k, k, k, device=w.device, dtype=torch.float32)
        wide[:, :cin] = w
        w = wide
    nbytes = lib.load().e4s_conv3dx_pack_bytes(cin_pad, cout, k)
    if nbytes == 0:
        raise RuntimeError(f"conv3dx_pack: a [Cout, 32j, k, k, k] weight with k 1, 3 or 7 (after padding), got {tuple(w.shape)}")
    out = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
    call("e4s_conv3dx_pack_f32", fptr(w), ptr(out), cin_pad, cout, k, 0 if f32 else 1, stream())
    out.conv3dx_f32 = bool(f32)
    out.conv3dx_shape = (cout, cin_pad, k)
    return out


def conv3dx(x, w_pack, cout, y, *, y_coff=0, bias=None, res=None, relu=False, up2=False, f32=None):
    """The 3-D conv family: the zero-padded k^3 conv of x fp32 [1|B,D,H,W,Cin] (contiguous channels, any other strides; a batch-1 x
    is broadcast over y's batch) -> channels y_coff .. y_coff + cout of the contiguous y [B,D,Ho,Wo,C].  v = acc + bias + res, ReLU
    with relu; res: a volume [B,D,Ho,Wo,>= cout] read through its strides.  up2 (k = 3): x is read through the nearest (1, 2, 2)
    up-sampling.  Writes y in place and returns it."""
    _vol(x, "conv3dx: x")
    xb, d, hi, wi, cin = x.shape
    ho, wo = (2 * hi, 2 * wi) if up2 else (hi, wi)
    if y.dtype != torch.float32 or y.dim() != 5 or not y.is_contiguous() or tuple(y.shape[1:4]) != (d, ho, wo) or y.shape[4] < y_coff + cout \
            or y_coff % 4 or y_coff < 0:
        raise RuntimeError(f"conv3dx: y is a contiguous fp32 volume of {(d, ho, wo)} voxels with channels {y_coff} .. {y_coff + cout} (y_coff % 4 == 0), "
                           f"got {tuple(y.shape)}")
    b = y.shape[0]
    if xb != b and xb != 1:
        raise RuntimeError(f"conv3dx: x has batch {xb}, y {b}")
    f32 = sr_f32() if f32 is None else bool(f32)
    shape = getattr(w_pack, "conv3dx_shape", None)
    if shape is None or shape[:2] != (cout, cin) or getattr(w_pack, "conv3dx_f32", None) != f32:
        raise RuntimeError(f"conv3dx: w_pack is not conv3dx_pack's image of a [{cout},{cin},k,k,k] weight in this precision")
    for name, t in (("w_pack", w_pack), ("y", y), ("bias", bias), ("res", res)):
        if t is not None and t.device != x.device:
            raise RuntimeError(f"conv3dx: {name} is on {t.device}, x on {x.device}")
    p = lib.Conv3dxParams()
    p.x, p.w, p.y = c_p(x.data_ptr()), fptr(w_pack), c_p(y.data_ptr() + 4 * y_coff)
    if bias is not None:
        if bias.numel() != cout:
            raise RuntimeError(f"conv3dx: bias has {bias.numel()} entries for {cout} channels")
        p.bias = fptr(_f32(bias))
    if res is not None:
        _vol(res, "conv3dx: res", cout)
        if tuple(res.shape[:4]) != (b, d, ho, wo):
            raise RuntimeError(f"conv3dx: res holds {tuple(res.shape[:4])} voxels, y {(b, d, ho, wo)}")
        p.res = c_p(res.data_ptr())
        p.r_bstride, p.r_dstride, p.r_ystride, p.r_xstride = res.stride(0), res.stride(1), res.stride(2), res.stride(3)
    p.x_bstride, p.x_dstride, p.x_ystride, p.x_xstride = (x.stride(0) if xb == b else 0), x.stride(1), x.stride(2), x.stride(3)
    p.B, p.D, p.Hi, p.Wi, p.Cin, p.Cout = b, d, hi, wi, cin, cout
    p.y_cstride, p.ksize = y.shape[4], shape[2]
    p.up2, p.relu, p.precision = 1 if up2 else 0, 1 if relu else 0, 1 if f32 else 0
    call("e4s_conv3dx_f32", ctypes.byref(p), stream())
    return y


def avgpool2_into(x, c, y, y_coff=0):
    """nn.AvgPool2d(2) of the first c channels of the contiguous NHWC x into channels y_coff .. y_coff + c of the contiguous NHWC y
    [B,H/2,W/2,C] (AvgPool3d((1, 2, 2)) of a volume: its B D planes as the batch)."""
    b, hi, wi, xc = x.shape
    if x.dtype != torch.float32 or y.dtype != torch.float32 or not x.is_contiguous() or not y.is_contiguous() or xc < c \
            or tuple(y.shape[:3]) != (b, hi // 2, wi // 2) or y.shape[3] < y_coff + c or y_coff % 4 or y_coff < 0 or not x.is_cuda or not y.is_cuda:
        raise RuntimeError(f"avgpool2_into: contiguous fp32 NHWC device maps, y {(b, hi // 2, wi // 2)} pixels with channels {y_coff} .. {y_coff + c}")
    call("e4s_avgpool2s_f32", c_p(x.data_ptr()), c_p(y.data_ptr() + 4 * y_coff), b, hi, wi, c, xc, y.shape[3], stream())
    return y


def bnrelu3d(x, scale, shift, y):
    """y = relu(x * scale[c] + shift[c]): x a volume read through its strides, y the contiguous volume of its shape."""
    _vol(x, "bnrelu3d: x")
    b, d, h, w, c = x.shape
    if tuple(y.shape) != tuple(x.shape) or not y.is_contiguous() or y.dtype != torch.float32 or scale.numel() != c or shift.numel() != c:
        raise RuntimeError("bnrelu3d: y is the contiguous fp32 volume of x's shape; scale and shift have one entry per channel")
    call("e4s_bnrelu3d_f32", c_p(x.data_ptr()), x.stride(0), x.stride(1), x.stride(2), x.stride(3), fptr(_f32(scale)), fptr(_f32(shift)),
         fptr(y), b, d, h, w, c, stream())
    return y


def _kp(kp_source, kp_driving, jac, what):
    n, k = kp_driving.shape[:2]
    if tuple(kp_driving.shape) != (n, k, 3) or kp_source.shape[0] not in (1, n) or tuple(kp_source.shape[1:]) != (k, 3):
        raise RuntimeError(f"{what}: kp_driving [N,K,3] and kp_source [1|N,K,3]")
    if jac is not None and jac.numel() != n * k * 9:
        raise RuntimeError(f"{what}: jac holds [N,K,3,3]")
    return n, k


def kp_jacobian(j_source, j_driving, out=None):
    """J_source [1|N,K,3,3] @ inverse(J_driving [N,K,3,3]) -> [N,K,3,3] (the 3x3 inverse by cofactors)."""
    n, k = j_driving.shape[:2]
    if tuple(j_driving.shape) != (n, k, 3, 3) or j_source.shape[0] not in (1, n) or tuple(j_source.shape[1:]) != (k, 3, 3):
        raise RuntimeError("kp_jacobian: j_driving [N,K,3,3] and j_source [1|N,K,3,3]")
    out = torch.empty(n, k, 3, 3, device=j_driving.device, dtype=torch.float32) if out is None else out
    call("e4s_kp_jacobian_f32", fptr(_f32(j_source)), j_source.shape[0], fptr(_f32(j_driving)), fptr(out), n, k, stream())
    return out


def sparse_warp(feat, kp_source, kp_driving, jac, y, y_coff=0, variance=0.01):
    """DenseMotionNetwork's hourglass input.  feat: the compressed volume [1|N,D,H,W,4] (contiguous); kp_source [1|N,K,3], kp_driving
    [N,K,3]; jac: kp_jacobian's [N,K,3,3] or None -> channels y_coff + 5 g .. + 4 (g = 0 .. K) of the contiguous y [N,D,H,W,C] = [the
    heat-map difference of keypoint g - 1 (0 for g = 0), feat sampled under sparse motion g]."""
    n, k = _kp(kp_source, kp_driving, jac, "sparse_warp")
    fb, d, h, w, c = feat.shape
    if c != 4 or not feat.is_contiguous() or feat.dtype != torch.float32 or fb not in (1, n):
        raise RuntimeError(f"sparse_warp: feat is a contiguous fp32 volume [1|N,D,H,W,4], got {tuple(feat.shape)}")
    if y.dtype != torch.float32 or not y.is_contiguous() or tuple(y.shape[:4]) != (n, d, h, w) or y.shape[4] < y_coff + 5 * (k + 1) or y_coff < 0:
        raise RuntimeError(f"sparse_warp: y is a contiguous fp32 volume {(n, d, h, w)} with {5 * (k + 1)} channels from {y_coff}")
    call("e4s_sparse_warp_f32", fptr(feat), fb, fptr(_f32(kp_source)), kp_source.shape[0], fptr(_f32(kp_driving)),
         fptr(_f32(jac)) if jac is not None else None, c_p(y.data_ptr() + 4 * y_coff), y.shape[4], n, k, d, h, w, c, float(variance), stream())
    return y


def motion_combine(logits, kp_source, kp_driving, jac, mask=None, deformation=None):
    """logits: the first K + 1 channels of a contiguous volume [N,D,H,W,C] -> (mask [N,D,H,W,K + 1] = their softmax, deformation
    [N,D,H,W,3] = sum_g mask_g * sparse motion g).  The sparse motions are recomputed from the keypoints."""
    n, k = _kp(kp_source, kp_driving, jac, "motion_combine")
    if logits.dtype != torch.float32 or logits.dim() != 5 or not logits.is_contiguous() or logits.shape[0] != n or logits.shape[4] < k + 1:
        raise RuntimeError(f"motion_combine: logits is a contiguous fp32 volume [N,D,H,W,>= {k + 1}]")
    _, d, h, w, cs = logits.shape
    mask = torch.empty(n, d, h, w, k + 1, device=logits.device, dtype=torch.float32) if mask is None else mask
    deformation = torch.empty(n, d, h, w, 3, device=logits.device, dtype=torch.float32) if deformation is None else deformation
    if tuple(mask.shape) != (n, d, h, w, k + 1) or tuple(deformation.shape) != (n, d, h, w, 3):
        raise RuntimeError("motion_combine: mask [N,D,H,W,K + 1] and deformation [N,D,H,W,3]")
    call("e4s_motion_combine_f32", fptr(logits), cs, fptr(_f32(kp_source)), kp_source.shape[0], fptr(_f32(kp_driving)),
         fptr(_f32(jac)) if jac is not None else None, fptr(mask), fptr(deformation), n, k, d, h, w, stream())
    return mask, deformation


def warp3d(vol, deformation, y=None):
    """F.grid_sample (trilinear, zero padding, align_corners False) of the ONE volume vol [1,D,H,W,C] (read through its strides)
    under deformation [N,D,H,W,3] -> y NHWC [N,H,W,D * C] with channel d * C + c."""
    _vol(vol, "warp3d: vol")
    one, d, h, w, c = vol.shape
    n = deformation.shape[0]
    if one != 1 or tuple(deformation.shape) != (n, d, h, w, 3) or deformation.dtype != torch.float32:
        raise RuntimeError(f"warp3d: a batch-1 volume and a deformation [N,{d},{h},{w},3] of its (d, h, w), got {tuple(vol.shape)} and {tuple(deformation.shape)}")
    y = torch.empty(n, h, w, d * c, device=vol.device, dtype=torch.float32) if y is None else y
    if tuple(y.shape) != (n, h, w, d * c) or not y.is_contiguous() or y.dtype != torch.float32:
        raise RuntimeError(f"warp3d: y is a contiguous fp32 map {(n, h, w, d * c)}")
    call("e4s_warp3d_f32", c_p(vol.data_ptr()), vol.stride(1), vol.stride(2), vol.stride(3), fptr(deformation), fptr(y), n, d, h, w, c, stream())
    return y


def occlusion_pack(w, depth):
    """DenseMotionNetwork.occlusion's weight [1,C * depth,k,k] (input channel c * depth + d) -> [k,k,depth,C], e4s_occlusion_f32's."""
    one, cd, k, k2 = w.shape
    if one != 1 or k != k2 or cd % depth:
        raise RuntimeError(f"occlusion_pack: a [1, C * {depth}, k, k] weight, got {tuple(w.shape)}")
    return _f32(w).view(cd // depth, depth, k, k).permute(2, 3, 1, 0).contiguous()


def occlusion(x, c, w_pack, bias, out=None):
    """sigmoid(Conv2d(D * c -> 1, k x k, padding k / 2)) of the first c channels of the contiguous volume x [N,D,H,W,C] seen as the
    map [N,c * D,H,W] -> [N,H,W]; w_pack: occlusion_pack's."""
    n, d, h, w, cs = x.shape
    k = w_pack.shape[0]
    if x.dtype != torch.float32 or not x.is_contiguous() or cs < c or tuple(w_pack.shape) != (k, k, d, c) or not w_pack.is_contiguous():
        raise RuntimeError(f"occlusion: x a contiguous fp32 volume with {c} or more channels, w_pack [k,k,{d},{c}]")
    out = torch.empty(n, h, w, device=x.device, dtype=torch.float32) if out is None else out
    if tuple(out.shape) != (n, h, w) or not out.is_contiguous():
        raise RuntimeError(f"occlusion: out is a contiguous fp32 map {(n, h, w)}")
    call("e4s_occlusion_f32", fptr(x), cs, fptr(w_pack), fptr(_f32(bias)) if bias is not None else None, fptr(out), n, d, h, w, c, k, stream())
    return out


def scale_rows(y, m):
    """y [..., C] *= m [...] in place (the occlusion product): both contiguous fp32, C % 4 == 0."""
    c = y.shape[-1]
    if y.dtype != torch.float32 or not y.is_contiguous() or m.numel() * c != y.numel():
        raise RuntimeError("scale_rows: y [..., C] contiguous fp32 and one multiplier per row")
    call("e4s_scale_rows_f32", fptr(y), fptr(_f32(m)), y.numel() // c, c, stream())
    return y


# ---- face-vid2vid SPADE decoder (spade.py) -------------------------------------------------
def _spade_map(t, c, what):
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 4 or t.shape[-1] < c:
        raise RuntimeError(f"{what}: a contiguous fp32 NHWC device buffer of {c} or more channels")
    return fptr(t), t.shape[-1]


def _spade_pack(w_pack, cout, cin, f32, what):
    f32 = sr_f32() if f32 is None else bool(f32)
    if getattr(w_pack, "rconv_shape", None) != (cout, cin, 3) or getattr(w_pack, "rconv_f32", None) != f32:
        raise RuntimeError(f"{what}: w_pack is not rconv_pack's image of a [{cout},{cin},3,3] weight in this precision")
    return f32


def instnorm_stats_into(x, stats, ws, eps=1e-5):
    """e4s_instnorm_stats_f32 on the contiguous NHWC map x into the caller's stats [B,C,2] and fp64 workspace (instnorm_ws_doubles)."""
    b, h, w, c = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous() or tuple(stats.shape) != (b, c, 2) or not stats.is_contiguous() \
            or ws.dtype != torch.float64 or ws.numel() < lib.load().e4s_instnorm_ws_doubles(b, h * w, c):
        raise RuntimeError("instnorm_stats_into: x contiguous fp32 NHWC, stats [B,C,2], ws of e4s_instnorm_ws_doubles doubles")
    call("e4s_instnorm_stats_f32", fptr(x), fptr(stats), None, ptr(ws), b, h * w, c, float(eps), stream())
    return stats


def spade_shared(seg, cin, w_pack, cout, bias, y, *, shift=0, y_coff=0, f32=None):
    """relu(3x3 conv + bias) of the first cin channels of the NHWC map seg [B,h,w,.], read through the nearest upsampling by 2^shift,
    -> channels y_coff .. y_coff + cout of y [B,h << shift,w << shift,.].  w_pack: rconv_pack's image of the [cout,cin,3,3] weight."""
    p = lib.SpadeSharedParams()
    p.seg, p.seg_cstride = _spade_map(seg, cin, "spade_shared(seg)")
    p.y, p.y_cstride = _spade_map(y, y_coff + cout, "spade_shared(y)")
    b, h, w, _ = seg.shape
    if shift not in (0, 1, 2) or tuple(y.shape[:3]) != (b, h << shift, w << shift):
        raise RuntimeError(f"spade_shared: shift 0..2 and y of {(b, h << max(shift, 0), w << max(shift, 0))} pixels, got shift {shift}, {tuple(y.shape[:3])}")
    f32 = _spade_pack(w_pack, cout, cin, f32, "spade_shared")
    if bias is not None and bias.numel() != cout:
        raise RuntimeError(f"spade_shared: bias has {bias.numel()} entries for {cout} channels")
    for name, t in (("w_pack", w_pack), ("y", y), ("bias", bias)):
        if t is not None and t.device != seg.device:
            raise RuntimeError(f"spade_shared: {name} is on {t.device}, seg on {seg.device}")
    p.w, p.bias = fptr(w_pack), fptr(_f32(bias)) if bias is not None else None
    p.B, p.Hs, p.Ws, p.Cin, p.Cout, p.y_coff, p.shift, p.precision = b, h, w, cin, cout, int(y_coff), int(shift), 1 if f32 else 0
    call("e4s_spade_shared_f32", ctypes.byref(p), stream())
    return y


def spade_conv(a, a_coff, cin, w_pack, bias, x, stats, y, *, xs=0, act=True, y_coff=0, f32=None):
    """One SPADE behind its mlp_shared: channels a_coff .. a_coff + cin of the NHWC buffer a [B,H,W,.] -> y[.., y_coff .. y_coff + C)
    = (x - mean) * rstd * (1 + gamma) + beta, LeakyReLU(0.2) with act; x [B,H >> xs,W >> xs,.] (its first C channels) is read through
    a nearest x2 upsampling with xs = 1, stats [B,C,2] are instnorm_stats of x.  w_pack: rconv_pack's image of the interleaved
    [2 C,cin,3,3] weight (row 2 c gamma's, 2 c + 1 beta's), bias [2 C] interleaved the same way."""
    c = stats.shape[1] if stats.dim() == 3 else -1
    p = lib.SpadeConvParams()
    p.a, p.a_cstride = _spade_map(a, a_coff + cin, "spade_conv(a)")
    p.x, p.x_cstride = _spade_map(x, max(c, 1), "spade_conv(x)")
    p.y, p.y_cstride = _spade_map(y, y_coff + max(c, 1), "spade_conv(y)")
    b, h, w, _ = a.shape
    if xs not in (0, 1) or tuple(x.shape[:3]) != (b, h >> xs, w >> xs) or (x.shape[1] << xs, x.shape[2] << xs) != (h, w):
        raise RuntimeError(f"spade_conv: x must hold the output's pixels {(b, h, w)} shifted by xs = {xs}, got {tuple(x.shape[:3])}")
    if tuple(y.shape[:3]) != (b, h, w) or tuple(stats.shape) != (b, c, 2) or stats.dtype != torch.float32 or not stats.is_contiguous():
        raise RuntimeError(f"spade_conv: y of {(b, h, w)} pixels and contiguous fp32 stats [B,C,2]")
    f32 = _spade_pack(w_pack, 2 * c, cin, f32, "spade_conv")
    if bias is None or bias.numel() != 2 * c:
        raise RuntimeError(f"spade_conv: the interleaved bias has {2 * c} entries")
    for name, t in (("w_pack", w_pack), ("bias", bias), ("x", x), ("stats", stats), ("y", y)):
        if t.device != a.device:
            raise RuntimeError(f"spade_conv: {name} is on {t.device}, a on {a.device}")
    p.w, p.bias, p.stats = fptr(w_pack), fptr(_f32(bias)), fptr(stats)
    p.B, p.H, p.W, p.Cin, p.C, p.a_coff, p.xH, p.xW, p.y_coff = b, h, w, cin, c, int(a_coff), x.shape[1], x.shape[2], int(y_coff)
    p.xs, p.act, p.precision = int(xs), 1 if act else 0, 1 if f32 else 0
    call("e4s_spade_conv_f32", ctypes.byref(p), stream())
    return y


def spade_tail_pack(w):
    """conv_img's weight [3,64,3,3] -> [9,3,64] (tap, output, input), e4s_spade_tail_f32's."""
    if tuple(w.shape) != (3, 64, 3, 3):
        raise RuntimeError(f"spade_tail_pack: a [3,64,3,3] weight, got {tuple(w.shape)}")
    return _f32(w).permute(2, 3, 0, 1).reshape(9, 3, 64).contiguous()


def spade_tail(x, wp, bias, *, u8=False, nchw=True, logits=None):
    """sigmoid(conv_img(leaky_relu(x, 0.2))) of the first 64 channels of NHWC x: fp32 (NCHW or NHWC), or with u8 the uint8 NHWC image
    round_half_even(clamp(v, 0, 1) * 255).  logits: an fp32 [B,3,H,W] buffer that receives the conv's output."""
    _spade_map(x, 64, "spade_tail(x)")
    b, h, w, cs = x.shape
    if tuple(wp.shape) != (9, 3, 64) or bias.numel() != 3 or wp.device != x.device or bias.device != x.device:
        raise RuntimeError("spade_tail: wp is spade_tail_pack's [9,3,64] and bias [3], on x's device")
    if logits is not None and (logits.dtype != torch.float32 or tuple(logits.shape) != (b, 3, h, w) or not logits.is_contiguous() or logits.device != x.device):
        raise RuntimeError(f"spade_tail: logits is a contiguous fp32 buffer {(b, 3, h, w)}")
    if u8:
        out = torch.empty(b, h, w, 3, device=x.device, dtype=torch.uint8)
        yf, yu = None, out
    else:
        out = torch.empty((b, 3, h, w) if nchw else (b, h, w, 3), device=x.device, dtype=torch.float32)
        yf, yu = out, None
    call("e4s_spade_tail_f32", fptr(x), cs, fptr(_f32(wp)), fptr(_f32(bias)), fptr(yf), 1 if nchw else 0, ptr(yu), fptr(logits), b, h, w, stream())
    return out


# ---- the joins of the face-swap pipeline (pipeline.py; csrc/pipeline.hip) ----------------------
def _join_arg(t, what, dtype, dims, last=None):
    """Wrong dtype / shape / layout: ValueError; a tensor off the device: RuntimeError."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dims or (last is not None and t.shape[-1] != last):
        got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what}, got {got}")
    if not t.is_cuda:
        raise RuntimeError(f"{what.split(':')[0]} runs on the ROCm device only (no CPU path)")
    if not t.is_contiguous():
        raise ValueError(f"{what}, contiguous")
    return t


def _join_out(out, shape, dtype, like, what):
    if out is None:
        return torch.empty(shape, device=like.device, dtype=dtype)
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"{what} is a contiguous {dtype} buffer {tuple(shape)}")
    if out.device != like.device:
        raise RuntimeError(f"{what} is on {out.device}, the input on {like.device}")
    return out


def resize_aa4(images_u8, out=None):
    """skimage.transform.resize(im / 255.0, (H/4, W/4)) of scikit-image 0.20 for uint8 NHWC images [B,H,W,3] -> fp32 [B,H/4,W/4,3]
    in [0,1]; H and W multiples of 4, at least 8 (a single reflection at the border must suffice)."""
    x = _join_arg(images_u8, "resize_aa4: uint8 NHWC images [B,H,W,3]", torch.uint8, 4, 3)
    b, h, w, _ = x.shape
    if b < 1 or h % 4 or w % 4 or h < 8 or w < 8:
        raise ValueError(f"resize_aa4: H and W must be multiples of 4 and at least 8, got {h} x {w} (batch {b})")
    out = _join_out(out, (b, h // 4, w // 4, 3), torch.float32, x, "resize_aa4: out")
    call("e4s_resize_aa4_u8_f32", ptr(x), fptr(out), b, h, w, stream())
    return out


def driven_seam(pred, enlarge=True, out=None, out_enlarged=None):
    """The decoder's fp32 NCHW prediction [N,3,h,w] in [0,1] -> (uint8 BGR [N,h,w,3] = (pred * 255).astype(uint8), truncated; that
    frame enlarged x4 by cv2.resize's 8-bit INTER_LINEAR arithmetic, uint8 BGR [N,4h,4w,3], or None with enlarge=False)."""
    x = _join_arg(pred, "driven_seam: an fp32 NCHW prediction [N,3,h,w]", torch.float32, 4)
    n, c, h, w = x.shape
    if c != 3 or n < 1 or h < 1 or w < 1:
        raise ValueError(f"driven_seam: an fp32 NCHW prediction [N,3,h,w], got {tuple(x.shape)}")
    out = _join_out(out, (n, h, w, 3), torch.uint8, x, "driven_seam: out")
    big = _join_out(out_enlarged, (n, 4 * h, 4 * w, 3), torch.uint8, x, "driven_seam: out_enlarged") if enlarge else None
    call("e4s_driven_seam_f32", fptr(x), ptr(out), ptr(big), n, h, w, stream())
    return out, big


def face_to_net(faces_u8, bgr=False, rgb=True, net=True, out_rgb=None, out_net=None):
    """uint8 NHWC faces [B,H,W,3] (BGR with bgr) -> (uint8 RGB NHWC, what the parser reads; fp32 NCHW [B,3,H,W] = (v / 255 - 0.5) /
    0.5, the encoder's input, bit for bit torchvision's ToTensor + Normalize(0.5, 0.5)).  rgb / net = False: that output is None.
    out_net may be a slice of a larger buffer (GraphedFaceSwap.static)."""
    x = _join_arg(faces_u8, "face_to_net: uint8 NHWC faces [B,H,W,3]", torch.uint8, 4, 3)
    b, h, w, _ = x.shape
    if b < 1 or h < 1 or w < 1 or not (rgb or net or out_rgb is not None or out_net is not None):
        raise ValueError(f"face_to_net: a non-empty batch and one output or both, got {tuple(x.shape)}")
    o_rgb = _join_out(out_rgb, (b, h, w, 3), torch.uint8, x, "face_to_net: out_rgb") if rgb or out_rgb is not None else None
    o_net = _join_out(out_net, (b, 3, h, w), torch.float32, x, "face_to_net: out_net") if net or out_net is not None else None
    call("e4s_face_to_net_u8", ptr(x), 1 if bgr else 0, ptr(o_rgb), fptr(o_net), b, h, w, stream())
    return o_rgb, o_net


# ---- face editing (edit.py; csrc/edit.hip) -----------------------------------------------------
def texture_mix(src, ref, sel, a0, a1, out=None):
    """scripts/face_edit.py:81-87 for a batch, one launch: out[b,r] = sel[b,r] ? a0[b,r] * src[b|0,r] + a1[b,r] * ref[b|0,r] : src[b|0,r]
    (two products, one sum, a rounding each; unselected rows copied).  src / ref fp32 [1|B,R,C]; sel uint8, a0, a1 fp32 [B,R]."""
    a0 = _join_arg(a0, "texture_mix: a0 is an fp32 [B,R] tensor", torch.float32, 2)
    b, r = a0.shape
    src = _join_arg(src, "texture_mix: src is an fp32 [1|B,R,C] tensor", torch.float32, 3)
    ref = _join_arg(ref, "texture_mix: ref is an fp32 [1|B,R,C] tensor", torch.float32, 3)
    a1 = _join_arg(a1, "texture_mix: a1 is an fp32 [B,R] tensor", torch.float32, 2)
    sel = _join_arg(sel, "texture_mix: sel is a uint8 [B,R] tensor", torch.uint8, 2)
    c = src.shape[2]
    if (b < 1 or r < 1 or c < 1 or tuple(sel.shape) != (b, r) or tuple(a1.shape) != (b, r) or src.shape[0] not in (1, b)
            or ref.shape[0] not in (1, b) or tuple(src.shape[1:]) != (r, c) or tuple(ref.shape[1:]) != (r, c)):
        raise ValueError(f"texture_mix: src {tuple(src.shape)} / ref {tuple(ref.shape)} are [1|B,R,C] and sel {tuple(sel.shape)} / a0 "
                         f"{tuple(a0.shape)} / a1 {tuple(a1.shape)} are [B,R]")
    out = _join_out(out, (b, r, c), torch.float32, src, "texture_mix: out")
    call("e4s_texture_mix_f32", fptr(src), fptr(ref), ptr(sel), fptr(a0), fptr(a1), fptr(out), b, r, c,
         1 if src.shape[0] == 1 and b > 1 else 0, 1 if ref.shape[0] == 1 and b > 1 else 0, stream())
    return out


def labels_to_color(labels, out=None):
    """demo/gradio_utils.py:58-73: uint8 label maps [...] -> uint8 RGB [...,3] in the demo's 19 colours; ids >= 19 black."""
    x = _join_arg(labels, "labels_to_color: a uint8 label map", torch.uint8, labels.dim() if isinstance(labels, torch.Tensor) else 0)
    out = _join_out(out, tuple(x.shape) + (3,), torch.uint8, x, "labels_to_color: out")
    call("e4s_labels_to_color_u8", ptr(x), ptr(out), x.numel(), stream())
    return out


def color_to_labels(rgb, out=None):
    """demo/gradio_utils.py:75-84: uint8 RGB [...,3] -> uint8 label maps [...]; colours outside the table 0."""
    x = _join_arg(rgb, "color_to_labels: a uint8 RGB map [...,3]", torch.uint8, rgb.dim() if isinstance(rgb, torch.Tensor) else 0, 3)
    out = _join_out(out, tuple(x.shape[:-1]), torch.uint8, x, "color_to_labels: out")
    call("e4s_color_to_labels_u8", ptr(x), ptr(out), out.numel(), stream())
    return out


def mask_brush(labels, brush, comp_idx, out=None):
    """demo/gradio_demo.py:126-130: labels[sum(brush[..., :3]) != 0] = comp_idx.  labels uint8 [...], brush uint8 [...,3|4] (gradio's
    sketch is RGBA); out may be labels (in place)."""
    x = _join_arg(labels, "mask_brush: a uint8 label map", torch.uint8, labels.dim() if isinstance(labels, torch.Tensor) else 0)
    br = _join_arg(brush, "mask_brush: a uint8 brush [...,3|4]", torch.uint8, x.dim() + 1)
    if br.shape[-1] not in (3, 4) or tuple(br.shape[:-1]) != tuple(x.shape) or not 0 <= int(comp_idx) <= 255:
        raise ValueError(f"mask_brush: brush {tuple(br.shape)} is the label map's shape {tuple(x.shape)} + (3|4,), comp_idx a byte")
    out = _join_out(out, tuple(x.shape), torch.uint8, x, "mask_brush: out")
    call("e4s_mask_brush_u8", ptr(x), ptr(br), ptr(out), x.numel(), int(br.shape[-1]), int(comp_idx), stream())
    return out
