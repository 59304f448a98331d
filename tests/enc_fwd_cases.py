"""Seeded cases and fp64 yardsticks for the forward glue of the regional style encoder (csrc/encoder.hip: instnorm_stats, the statistics
finalisation, instnorm_apply with and without the fused output statistics, se_gate and the fused finalisation + gate,
resize_bilinear_to_nhwc, conv3x3_small and the tiled stem conv): the yardsticks of tests/test_enc_fwd_cases_host.py and
tests/test_gpu_encoder_forward_kernels.py.  CPU only; the native library is not imported here.

Every reference takes the fp32 operands cast to double and is a plain statement of the operation: F.instance_norm semantics (biased
variance, eps inside the root; eps is the fp32 number the kernel is handed, cast to double), sigmoid(fc2 relu(fc1 p)), bilinear
interpolation with align_corners=False at EXACT RATIONAL source coordinates ((2 o + 1) Hi - Ho) / (2 Ho), and F.conv2d(padding=1).  None
restates a kernel's loop.  The one piece of kernel arithmetic restated here is the split count (instnorm_nsplit and the H W in [16, 1024]
switch of e4s_instnorm_stats_f32), which the batch-independence checks and the path classifier need, as enc_bwd_cases.in_nsplit does.

Two kinds of operand data (gen_bwd_cases.operand):
  random  fp32 normal values, for the statistics shifted and scaled per (b, c): |mean| up to 1e3, standard deviation 1e-2 .. 1e2, with
          |mean| / std limited by the cancellation condition below; channel 0 of sample 0 is the constant 0.3 (no dyadic number; true
          variance 0: the clamp has to yield rsqrt(eps)).
  dyadic  integers in [-4, 4] times 2^-2; chosen statistics (mean a multiple of 2^-2 in [-1/2, 1/2], rstd in {1/2, 1, 2, 4}), gate in
          {1/2, 1, 2}, dyadic slopes, SE weights in multiples of 2^-4 (fc1) and 2^-2 (fc2).  Every product and every partial sum in any
          order is then an fp32 number and the output EQUALS the reference; the host test proves it per case by evaluating the formulas
          in fp32.  Held to the bound instead: rstd (an inverse root), the mean on a map whose H W is no power of two (a quotient), the
          gate (a sigmoid; its pre-activation is exact, which is what isolates the intrinsic below) and the resizes at non-dyadic ratios.

Bounds for random data, u = 2^-24, one line per rounding, from the kernels' operation chains (an FMA contraction only removes roundings):
  mean     s = sum x in double, mean = s / HW in double, one cast:                                                        1   u |mean|
           The double additions add HW 2^-53 mean|x|; the host test asserts that this stays below 2^-10 u |mean| for every random case.
           Where the tensor is a kernel's OUTPUT (the fused statistics of instnorm_apply and of the stem conv), whose mean cannot be
           kept away from 0, the term is carried explicitly instead: u |mean| + (HW + 1) 2^-53 mean|x|  (`mean_bound_sum`).
  rstd     var = q / HW - mean^2 in double (clamped at 0), then rstd = rsqrtf(fl(fl(var) + eps)).  On var + eps, relative:
             the cast of var          u var / (var + eps) <= u                                                            1/2 u on rstd
             the addition of eps      u                                                                                   1/2 u on rstd
             rsqrtf                   RSQRT_U u (allowance, see below)                                                RSQRT_U u on rstd
             the cancellation of q / HW - mean^2 in double: at most about CANCEL = (HW + 2) 2^-53 (q / HW) / (var + eps)      1/2 CANCEL
           |err| <= rstd ((1 + RSQRT_U) u + CANCEL / 2).  The part in u is CAPPED at 8u (RSTD_CAP_U; a condition, not a measurement: an
           unbiased variance moves rstd by >= 1 / (2 4225) ~ 2000 u at these sizes, a lost eps at var ~ 1e-4 by 5 %).  The host test
           asserts CANCEL < u for every random case, so the shifts and scales keep the reference alone inside the bound.
  pooled   (float)((mean - (double)mf) (double)rstd), mf = fl(mean): the reference is the fp64 mean of (x - stats[..., 0]) stats[..., 1]
           formed with the fp32 statistics THE KERNEL RETURNED, so only the following is left:
             the cast                                                                                                      1   u |pooled|
             the product and the difference in double                                                                2^-52 |pooled|
             the double sums of the kernel (HW additions of x) and of the reference (of (x - mf) rstd)
                                                                   (HW + 2) 2^-53 rstd (mean|x| + mean|x - mf|)
           pooled itself is about u |mean| rstd, so this holds it to 1e-3 of its size or better; nothing else in the suite looks at it.
  apply    o = fl(fl(x - mean) rstd) [fl(o gate)] [+ t, t = res or fl(fl(res - rmean) rrstd)] [o > 0 ? o : fl(o slope)]:
             a = (x - mean) rstd gate:   the subtraction, the product, the gate product                                  2 or 3   u |a|
             t:                          the subtraction and the product with res_stats, else a copy                     2 or 0   u |t|
             a + t:                      the addition                                                                    1   u |a + t|
           and one more on each of |a| and |t| for the second-order terms: e = u ((k_a + 1) |a| + (k_t + 1) |t| + |a + t|).  With a
           slope the error in front of it is scaled by max(1, |slope|) (a value whose sign the error flips lands on the other branch;
           both branches are continuous at 0) and the product adds u |y|:  |err| <= max(1, |slope|) e + u |y|.
  gate     hidden_j = relu(sum_c fc1[j, c] p[c]) and a_c = sum_j fc2[c, j] hidden_j are fp32 sums of n products in any order (strided
           lanes, a butterfly, float4 groups): (n + 1) u sum|products| each, the error of hidden carried through |fc2| (relu is
           1-Lipschitz):  A = (Cr + 1) u sum_j |fc2| hidden_j + sum_j |fc2| (C + 1) u sum_c |fc1| |p|.  The sigmoid has slope <= 1/4:
           |err| <= A / 4 + SIGMOID_U u.  SIGMOID_U is an ABSOLUTE allowance for gate = 1 / (1 + __expf(-a)) given a: a relative error
           E(a) u of __expf, which may grow like |a| (the argument is scaled to base 2 in fp32), moves the gate by g (1 - g) E(a) u, and
           |a| g (1 - g) <= 0.23 for every a; the addition and the division add 2u g.
  resize   y = hy (hx p00 + lx p01) + ly (hx p10 + lx p11), hy = fl(1 - ly), hx = fl(1 - lx); ly = fy - y0 is exact in fp32.
             per product chain: hy or hx 1, inner product 1, inner addition 1, outer product 1, outer addition 1: 5, + 1 second order,
             the other of hy / hx 1:                                                                  7 u sum |weights| |p|
             the fp32 coordinate fy = fl(fl((oy + 1/2) sy) - 1/2), sy = fl(Hi / Ho): the quotient u sy (oy + 1/2), the product
             u sy (oy + 1/2), the subtraction u |fy|:  |dfy| <= 3 u sy (oy + 1/2), likewise dfx.  The interpolant is continuous and
             piecewise linear, so the coordinate error moves it by at most |dfy| Dy + |dfx| Dx, Dy (Dx) the largest |difference of
             vertical (horizontal) neighbours| over the segments next to y0 (x0) -- next to, because the error can move the
             coordinate across an integer -- in the columns (rows) used.
           Equal sizes give ly = lx = 0 exactly: torch.equal with the permuted input, both kinds.
  conv     a sum of 9 Cin products in fp32, any order:  (9 Cin + 2) u sum |x| |w|  ((27 + 2) u at Cin = 3).

The two intrinsics.  Neither the project nor the vendor documents on hand give an ulp figure for rsqrtf and __expf on this target, so each
has an allowance: twice the worst residue measured on the MI355X, rounded up to a whole u.
  rsqrtf   residue = |rstd - 1 / sqrt(double(fl(fl(var64) + eps)))| / (u rstd) over every statistics case of both kinds (the reference
           fixes every other step of the chain, so this is the intrinsic's own):  measured worst 1.533 u  ->  RSQRT_U = 4 (the part in u is 5u, inside the cap)
  sigmoid  residue = |gate - sigmoid64(a)| / u over the dyadic SE cases, whose pre-activation a is exact in fp32 (|a| up to 20):
           measured worst 1.397 u  ->  SIGMOID_U = 3

Largest observed error / bound on the MI355X with these allowances (printed by the GPU test at teardown): instnorm_stats mean 0.99, rstd 0.35,
pooled 0.57; instnorm_finalize mean 0.98, rstd 0.38, pooled 0.25; instnorm_apply y 0.70, its fused output statistics mean 0.99, rstd 0.37;
se_gate 0.010 (unit), 0.004 (residue), 0.008 (exact pre-activation) -- the accumulation bound is a worst case over up to 512 terms;
finalize_se gate 0.25; resize 0.32; conv3x3_small 0.21, the tiled stem conv 0.09, their statistics mean 0.96, rstd 0.29.
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import gen_bwd_cases as gc
from enc_bwd_cases import host_stats, is_pow2, split_path  # noqa: F401
from gen_bwd_cases import KINDS, operand  # noqa: F401

U = 2.0 ** -24
EPS = 1e-5
RSQRT_U = 4            # allowance for rsqrtf, in u relative to rstd (module docstring)
SIGMOID_U = 3          # allowance for 1 / (1 + __expf(-a)) given a, in u absolute
RSTD_CAP_U = 8         # the part of the rstd bound that is counted in u may not exceed this
assert 1 + RSQRT_U <= RSTD_CAP_U


def f32(v):
    return float(np.float32(v))


# ---- the split arithmetic of csrc/encoder.hip, restated for the path classifier and the batch-independence checks ------------------------
def instnorm_nsplit(B, HW, C):
    d = B * (C // 64)
    ns = max(2048 // (d if d > 0 else 1), 1)
    if ns > HW // 64:
        ns = max(HW // 64, 1)
    return min(ns, 64)


def stats_is_small(HW):
    """e4s_instnorm_stats_f32 takes the one-launch kernel (one block per (sample, slab), no workspace) on these maps, whatever the batch"""
    return 16 <= HW <= 1024


def stats_path(B, HW, C):
    """"small", or the path of the last split: "single", "even", "ragged" or "empty" """
    return "small" if stats_is_small(HW) else split_path(HW, instnorm_nsplit(B, HW, C))


def small_has_unrolled_pass(HW):
    """some pixel group of the one-launch kernel (16 groups, 8 pixels in flight) takes a whole unrolled pass"""
    return HW > 7 * 16


def small_has_tail(HW):
    return HW % (8 * 16) != 0


# ---- fp64 references ---------------------------------------------------------------------------------------------------------------------
def stats_ref(x, eps=EPS):
    """InstanceNorm statistics of NHWC fp32 x in fp64 with their bounds.  `restated`: 1 / sqrt(double(fl(fl(var) + eps))), the value
    rsqrtf would return were it exact (for the measurement of its residue)."""
    B, H, W, C = x.shape
    HW = H * W
    xd = x.double().reshape(B, HW, C)
    e32 = torch.tensor(eps, dtype=torch.float32)
    mean, var, q = xd.mean(1), xd.var(1, unbiased=False), (xd * xd).mean(1)
    ve = var + e32.double()
    rstd = ve.rsqrt()
    cancel = (HW + 2) * 2.0 ** -53 * q / ve
    mabs = xd.abs().mean(1)
    return dict(mean=mean, var=var, rstd=rstd, cancel=cancel, mabs=mabs, mean_bound=U * mean.abs(),
                mean_bound_sum=U * mean.abs() + (HW + 1) * 2.0 ** -53 * mabs,
                rstd_bound=rstd * (min(1 + RSQRT_U, RSTD_CAP_U) * U + cancel / 2),
                restated=(var.float() + e32).double().rsqrt())


def pooled_ref(x, stats):
    """AdaptiveAvgPool2d(1) of the normalised tensor: the fp64 mean of (x - stats[..., 0]) stats[..., 1] with the fp32 `stats` given."""
    B, H, W, C = x.shape
    HW = H * W
    xd = x.double().reshape(B, HW, C)
    m, r = stats[..., 0].double()[:, None], stats[..., 1].double()[:, None]
    pooled = ((xd - m) * r).mean(1)
    bound = (U + 2.0 ** -52) * pooled.abs() + (HW + 2) * 2.0 ** -53 * r[:, 0] * (xd.abs().mean(1) + (xd - m).abs().mean(1))
    return pooled, bound


def apply_ref(x, stats, gate=None, res=None, res_stats=None, slope=None, rs=1):
    """y = prelu((x - mean) rstd gate + t), t = res[:, ::rs, ::rs] (MaxPool2d(1, rs)), normalised with res_stats if given; (y, bound)."""
    xd = x.double()
    a = (xd - stats[..., 0].double()[:, None, None]) * stats[..., 1].double()[:, None, None]
    ka = 2
    if gate is not None:
        a, ka = a * gate.double()[:, None, None], 3
    pre, e = a, (ka + 1) * a.abs()
    if res is not None:
        t, kt = res.double()[:, ::rs, ::rs], 0
        if res_stats is not None:
            t, kt = (t - res_stats[..., 0].double()[:, None, None]) * res_stats[..., 1].double()[:, None, None], 2
        pre = a + t
        e = e + (kt + 1) * t.abs() + pre.abs()
    e = U * e
    if slope is None:
        return pre, e
    sl = slope.double()
    y = torch.where(pre > 0, pre, pre * sl)
    return y, sl.abs().clamp(min=1.0) * e + U * y.abs()


def se_ref(pooled, fc1, fc2):
    """gate = sigmoid(fc2 relu(fc1 p)); `a` the pre-activation, `a_bound` its fp32 accumulation bound, `bound` the gate's."""
    p, w1, w2 = pooled.double(), fc1.double(), fc2.double()
    Cr, C = w1.shape
    hidden = torch.relu(p @ w1.t())
    h_abs = p.abs() @ w1.abs().t()
    a = hidden @ w2.t()
    a_abs = hidden @ w2.abs().t()
    a_bound = (Cr + 1) * U * a_abs + ((C + 1) * U * h_abs) @ w2.abs().t()
    return dict(gate=torch.sigmoid(a), a=a, a_abs=a_abs, h_abs=h_abs, a_bound=a_bound, bound=a_bound / 4 + SIGMOID_U * U)


def _axis(n_in, n_out):
    """exact rational source coordinate of every output index: i0, i1 (int64) and the weight of i1 (double), + the fp32 coordinate's error bound"""
    o = torch.arange(n_out, dtype=torch.int64)
    num, den = ((2 * o + 1) * n_in - n_out).clamp(min=0), 2 * n_out            # f = num / den, clamped at 0
    i0 = num // den
    lam = (num - i0 * den).double() / den
    i1 = (i0 + 1).clamp(max=n_in - 1)
    df = 3 * U * f32(n_in / n_out) * (o.double() + 0.5)
    return i0, i1, lam, df


def _segmax(p, dim, i0):
    """largest |p[k + 1] - p[k]| along `dim` over the segments k in {i0 - 1, i0, i0 + 1} that exist, gathered per output index"""
    n = p.shape[dim]
    d = (p.narrow(dim, 1, n - 1) - p.narrow(dim, 0, n - 1)).abs() if n > 1 else p.narrow(dim, 0, 0)
    pad = list(p.shape)
    pad[dim] = 2
    d = torch.cat([torch.zeros(pad, dtype=p.dtype), d, torch.zeros(pad, dtype=p.dtype)], dim)          # segment k sits at k + 2
    return torch.stack([d.index_select(dim, (i0 + 2 + j).clamp(0, d.shape[dim] - 1)) for j in (-1, 0, 1)]).amax(0)


def resize_ref(x, ho, wo):
    """F.interpolate(x, (ho, wo), mode="bilinear", align_corners=False) of NCHW x, as NHWC, in fp64 at exact source coordinates; (y, bound)."""
    B, C, Hi, Wi = x.shape
    xd = x.double()
    y0, y1, ly, dfy = _axis(Hi, ho)
    x0, x1, lx, dfx = _axis(Wi, wo)
    ly_, lx_ = ly[:, None], lx[None, :]
    rows0, rows1 = xd[:, :, y0], xd[:, :, y1]
    p00, p01, p10, p11 = rows0[..., x0], rows0[..., x1], rows1[..., x0], rows1[..., x1]
    y = (1 - ly_) * ((1 - lx_) * p00 + lx_ * p01) + ly_ * ((1 - lx_) * p10 + lx_ * p11)
    mag = (1 - ly_) * ((1 - lx_) * p00.abs() + lx_ * p01.abs()) + ly_ * ((1 - lx_) * p10.abs() + lx_ * p11.abs())
    sy = _segmax(xd, 2, y0)                                    # [B, C, ho, Wi]
    dy_ = torch.maximum(sy[..., x0], sy[..., x1])
    sx = _segmax(xd, 3, x0)                                    # [B, C, Hi, wo]
    dx_ = torch.maximum(sx[:, :, y0], sx[:, :, y1])
    bound = 7 * U * mag + dfy[:, None] * dy_ + dfx[None, :] * dx_
    return y.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


def conv_ref(x, w):
    """F.conv2d(padding=1) of NHWC x with w [Cout, Cin, 3, 3] in fp64, as NHWC; (y, bound)."""
    cin = x.shape[-1]
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    y = F.conv2d(xd, wd, padding=1).permute(0, 2, 3, 1).contiguous()
    mag = F.conv2d(xd.abs(), wd.abs(), padding=1).permute(0, 2, 3, 1).contiguous()
    return y, (9 * cin + 2) * U * mag


def slots_of(x, nslots):
    """fp64 [n, nslots, 2] = {sum, sum of squares} of the nslots consecutive (ragged) chunks of every row of fp32 x [n, HW]"""
    return torch.stack([torch.stack([c.sum(1), (c * c).sum(1)], -1) for c in torch.tensor_split(x.double(), nslots, dim=1)], 1)


# ---- case lists --------------------------------------------------------------------------------------------------------------------------
# instnorm_stats.  (1, 1), (3, 5): H W < 16, the split path with one split; (4, 4), (1, 17), (7, 7): the one-launch kernel, tail only;
# (1, 113): one unrolled pass for pixel group 0, tail for the others; (8, 16) = 128: one unrolled pass each, no tail; (31, 33) = 1023: up
# to eight passes and a tail; (32, 32): its largest map; (33, 32) = 1056: the first map of the split path, 16 even splits of 66;
# (35, 31): 16 splits of 68, the last of 65 (ragged); (65, 65) at B = 1, C = 64: 64 splits of 67, the last of 4.
STATS_GRIDS = [(1, 1), (3, 5), (4, 4), (1, 17), (7, 7), (1, 113), (8, 16), (31, 33), (32, 32), (33, 32), (35, 31), (65, 65)]
_STATS_KEYS = ("C", "grid", "B", "eps")
STATS_CASES = [dict(zip(_STATS_KEYS, (C, g, (1, 3)[(i + j) % 2], EPS))) for i, g in enumerate(STATS_GRIDS[:-1]) for j, C in enumerate((64, 128))]
STATS_CASES += [
    dict(C=64, grid=(65, 65), B=1, eps=EPS),                # 64 splits of 67, the last of 4 pixels
    dict(C=64, grid=(65, 65), B=3, eps=EPS),
    dict(C=128, grid=(65, 65), B=1, eps=EPS),
    dict(C=512, grid=(65, 65), B=8, eps=EPS),               # the batch term of instnorm_nsplit decides: 32 splits (64 at B = 1)
    dict(C=64, grid=(7, 7), B=3, eps=1e-3),
    dict(C=64, grid=(35, 31), B=1, eps=1e-3),
]

# e4s_instnorm_finalize_f32 on hand-made slots: rows of 64 values cut into nslots consecutive chunks (7 and 9: ragged, straddling the
# unroll of 8; 64: one value per slot); B C = 192, 256, 300
FINALIZE_CASES = [dict(nslots=ns, B=B, C=C) for ns in (1, 7, 9, 64) for B, C in ((3, 64), (2, 128), (3, 100))]
FINALIZE_HW = 64

# instnorm_apply: every combination of gate x residual x slope per (C, grid); C = 68 is no multiple of 64 (the plain kernel only)
APPLY_OPTIONS = [dict(gate=g, res=r, slope=s) for g in (False, True) for r in (None, "rs1", "rs2", "rs1_stats") for s in (False, True)]
APPLY_CASES = [dict(C=C, grid=g, B=(1, 3)[(i + j) % 2]) for i, C in enumerate((4, 68, 64, 128)) for j, g in enumerate(((1, 1), (5, 7), (33, 31)))]
# with the fused output statistics: (5, 7) one split; (33, 31): 15 splits of 69, the last of 57; (35, 31): 16 of 68, the last of 65;
# (33, 32): 16 even splits; (65, 65), B = 1, C = 64: 64 splits of 67, the last of 4
APPLY_STATS_CASES = [dict(C=C, grid=g, B=(1, 3)[(i + j) % 2]) for i, C in enumerate((64, 128)) for j, g in enumerate(((5, 7), (33, 31), (35, 31), (33, 32)))]
APPLY_STATS_CASES += [dict(C=64, grid=(65, 65), B=1)]

# se_gate: (C, Cr).  (64, 4), (128, 8), (512, 32): the encoder's; (256, 64): the face parser's (tpr = 8); (64, 3), (100, 5): Cr % 4 != 0, the
# scalar fc2 loop, C % 64 != 0; (64, 520): tpr = 1 and a second pass over the rows (520 > 512 threads).  regime "residue": pooled ~ 1e-8 with
# fc1 x 50, fc2 x 1e6; "unit": pooled O(1)
SE_NSLOTS = 7
SE_SHAPES = [(64, 4), (128, 8), (512, 32), (256, 64), (64, 3), (100, 5), (64, 520)]
SE_CASES = [dict(C=C, Cr=Cr, B=(3, 1)[(i + j) % 2], regime=r) for i, (C, Cr) in enumerate(SE_SHAPES) for j, r in enumerate(("residue", "unit"))]

_RS_KEYS = ("src", "dst", "C", "exact")
RESIZE_CASES = [dict(zip(_RS_KEYS, row), B=2) for row in [
    ((8, 8), (8, 8), 3, "copy"),              # torch.equal with the permuted input, both kinds
    ((16, 12), (8, 6), 1, "dyadic"),          # weights of 1/2
    ((32, 32), (8, 8), 3, "dyadic"),          # weights of 1/2, every fourth pair of pixels
    ((5, 7), (10, 14), 1, "dyadic"),          # weights 1/4 and 3/4, both border clamps
    ((7, 5), (16, 9), 3, None),
    ((17, 13), (6, 4), 1, None),
    ((1, 1), (4, 4), 3, None),
    ((1, 9), (3, 9), 1, None),
]]

# the grid-stride stem kernel: maps that are no multiples of 16, or Cin != 3 / Cout != 64.  (257, 256): 257 256 16 = 1052672 work items
# on 4096 x 256 = 1048576 threads: the first 4096 threads take a second lap.  `tiled`: the 16 x 16-tile kernel
_CONV_KEYS = ("B", "grid", "Cin", "Cout", "tiled")
CONV_CASES = [dict(zip(_CONV_KEYS, row)) for row in [
    (1, (1, 1), 3, 64, False),
    (2, (5, 7), 3, 64, False),
    (1, (17, 16), 3, 64, False),
    (2, (9, 6), 1, 4, False),
    (1, (8, 8), 4, 32, False),
    (1, (257, 256), 3, 64, False),
    (2, (16, 16), 3, 64, True),
    (3, (32, 48), 3, 64, True),
]]

CASES = {"stats": STATS_CASES, "finalize": FINALIZE_CASES, "apply": APPLY_CASES, "apply_stats": APPLY_STATS_CASES, "se": SE_CASES,
         "resize": RESIZE_CASES, "conv": CONV_CASES}


def case_id(c):
    return gc.case_id({k: f"{v[0]}x{v[1]}" if isinstance(v, tuple) and k != "grid" else v for k, v in c.items() if v is not None})


def option_id(o):
    return f"gate{int(o['gate'])}-{o['res'] or 'nores'}-slope{int(o['slope'])}"


def kinds_of(name, c):
    """the dyadic SE data are regime-free (exact pre-activation): built once, with the "unit" row"""
    return ("random",) if name == "se" and c["regime"] == "residue" else KINDS


def _gen(name, c, kind):
    return torch.Generator().manual_seed(zlib.crc32(f"encfwd-{name}-{case_id(c)}-{kind}".encode()))


def shifted(shape, g, rows=None):
    """random NHWC (or [n, HW] with rows=True) data with a mean and a standard deviation of its own per (b, c): std log-uniform in
    [1e-2, 1e2], |mean| in [std / 4, 1e3] limited to a quarter of what the cancellation condition of the rstd bound allows at this H W"""
    if rows:
        n, HW = shape
        stat_shape, base = (n, 1), torch.randn(n, HW, generator=g)
    else:
        B, H, W, C = shape
        HW = H * W
        stat_shape, base = (B, 1, 1, C), torch.randn(shape, generator=g)
    std = 10.0 ** (4 * torch.rand(stat_shape, generator=g) - 2)
    if HW == 1:                       # the variance is 0 whatever the value: CANCEL = 3 2^-53 x^2 / eps < u needs |x| < 42
        std, lim = torch.ones(stat_shape), torch.full(stat_shape, 20.0)
    else:
        lim = 0.25 * (2.0 ** 29 / (HW + 2)) ** 0.5 * std
    mag = torch.minimum(1e3 * torch.rand(stat_shape, generator=g), lim).clamp(min=0.25 * std)
    sign = torch.where(torch.rand(stat_shape, generator=g) < 0.5, -1.0, 1.0)
    return base * std + sign * mag


def _dyadic_stats(B, C, g):
    mean = torch.randint(-2, 3, (B, C), generator=g).float() * 0.25
    rstd = 2.0 ** torch.randint(-1, 3, (B, C), generator=g).float()
    return torch.stack([mean, rstd], -1)


@functools.lru_cache(maxsize=None)
def build(name, index, kind):
    """The fp32 operands of case `index` of CASES[name] with `kind` data and the references that do not depend on what a kernel returned,
    built once per session and shared: treat as read-only."""
    c = CASES[name][index]
    g = _gen(name, c, kind)
    out = dict(case=c, exact=kind == "dyadic")
    if name == "stats":
        B, (H, W), C = c["B"], c["grid"], c["C"]
        if kind == "dyadic":
            x = operand((B, H, W, C), kind, g)
        else:
            x = shifted((B, H, W, C), g)
            x[0, :, :, 0] = 0.3
        out.update(x=x, ref=stats_ref(x, c["eps"]), exact_mean=kind == "dyadic" and is_pow2(H * W))
    elif name == "finalize":
        B, C, ns = c["B"], c["C"], c["nslots"]
        rows = operand((B * C, FINALIZE_HW), kind, g) if kind == "dyadic" else shifted((B * C, FINALIZE_HW), g, rows=True)
        x = rows.reshape(B, C, 1, FINALIZE_HW).permute(0, 2, 3, 1).contiguous()          # the NHWC tensor these slots describe
        out.update(rows=rows, x=x, slots=slots_of(rows, ns).contiguous(), ref=stats_ref(x, EPS))
    elif name in ("apply", "apply_stats"):
        B, (H, W), C = c["B"], c["grid"], c["C"]
        sh = (B, H, W, C)
        if kind == "dyadic":
            x, res1, res2 = operand(sh, kind, g), operand(sh, kind, g), operand((B, 2 * H, 2 * W, C), kind, g)
            stats, res_stats = _dyadic_stats(B, C, g), _dyadic_stats(B, C, g)
            gate = 2.0 ** torch.randint(-1, 2, (B, C), generator=g).float()
            slope = operand((C,), kind, g)
        else:
            scale = lambda: 0.25 + 2 * torch.rand((B, 1, 1, C), generator=g)                 # noqa: E731
            shift = lambda: torch.randn((B, 1, 1, C), generator=g)                           # noqa: E731
            x = operand(sh, kind, g) * scale() + shift()
            res1 = operand(sh, kind, g) * scale() + shift()
            res2 = operand((B, 2 * H, 2 * W, C), kind, g) * scale() + shift()
            stats, res_stats = host_stats(x), host_stats(res1)
            gate = 2 * torch.rand((B, C), generator=g) - 0.5
            slope = 0.25 + 0.25 * torch.randn(C, generator=g)
        out.update(x=x, res1=res1, res2=res2, stats=stats, res_stats=res_stats, gate=gate, slope=slope)
    elif name == "se":
        B, C, Cr = c["B"], c["C"], c["Cr"]
        if kind == "dyadic":
            pooled, fc1, fc2 = operand((B, C), kind, g), operand((Cr, C), kind, g) * 0.25, operand((C, Cr), kind, g)
        elif c["regime"] == "residue":
            pooled = 1e-8 * torch.randn(B, C, generator=g)
            fc1, fc2 = 50 * torch.randn(Cr, C, generator=g), 1e6 * torch.randn(C, Cr, generator=g)
        else:
            pooled = torch.randn(B, C, generator=g)
            fc1, fc2 = torch.randn(Cr, C, generator=g) / C ** 0.5, 2 * torch.randn(C, Cr, generator=g) / Cr ** 0.5
        out.update(pooled=pooled, fc1=fc1, fc2=fc2, ref=se_ref(pooled, fc1, fc2), exact=False)
        if kind == "random":           # hand-made slots for e4s_instnorm_finalize_se_f32: its pooled vector is the residue of these rows' means
            rows = shifted((B * C, FINALIZE_HW), g, rows=True)
            out.update(rows=rows, slots=slots_of(rows, SE_NSLOTS).contiguous())
    elif name == "resize":
        (hi, wi), (ho, wo) = c["src"], c["dst"]
        x = operand((c["B"], c["C"], hi, wi), kind, g)
        y, bound = resize_ref(x, ho, wo)
        out.update(x=x, ref=y, bound=bound, exact=c["exact"] == "copy" or (kind == "dyadic" and c["exact"] == "dyadic"))
    elif name == "conv":
        B, (H, W) = c["B"], c["grid"]
        x = operand((B, H, W, c["Cin"]), kind, g)
        w = operand((c["Cout"], c["Cin"], 3, 3), kind, g)
        if kind == "random":
            w = w * 0.3
        y, bound = conv_ref(x, w)
        out.update(x=x, w=w, ref=y, bound=bound)
    else:
        raise KeyError(name)
    return out


def apply_operands(t, o):
    """the keyword operands of K.instnorm_apply for option combination `o` of an apply case built as `t`"""
    res = {None: None, "rs1": t["res1"], "rs1_stats": t["res1"], "rs2": t["res2"]}[o["res"]]
    return dict(gate=t["gate"] if o["gate"] else None, res=res, res_stats=t["res_stats"] if o["res"] == "rs1_stats" else None,
                slope=t["slope"] if o["slope"] else None, rs=2 if o["res"] == "rs2" else 1)
