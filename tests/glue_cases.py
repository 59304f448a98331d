"""Seeded cases and fp64 yardsticks for the small kernels around the convs of the Discriminator, GPEN and the generator forward
(csrc/ops.hip: fused_bias_act, channel_sum and the three upfirdn2d kernels; csrc/gpen.hip: conv1x1_small, noise_half, pixelnorm, add_scale,
minibatch_stddev; the tail of csrc/torgb.hip: const_input, mask_mul_add, noise_bias_act_nhwc; csrc/style.hip: the single-launch rowdot and
weight_sqsum; colsum of csrc/optim.hip; the row plan of csrc/plan.hip): the yardsticks of tests/test_glue_cases_host.py and
tests/test_gpu_glue_kernels.py.  CPU only; the native library is not imported here.

Every reference takes the fp32 operands cast to double and is a plain statement of the operation (zero insertion, pad / crop, F.conv2d with
the flipped kernel and a stride for upfirdn2d; sums, F.linear, F.interpolate(mode="nearest") for a pixel's region; model.py:783-790 for the
minibatch stddev).  None restates a kernel's loop.  Scalars (alpha, gain, scale, noise weight) are rounded to fp32 first, as the C ABI
receives them.  What IS restated here is host logic that the cases must know to say which launch form they reach: the dispatch rule of
e4s_upfirdn2d_f32 (upfirdn_path), the v4 / scalar / grid-stride rule of e4s_fused_bias_act_f32 (fba_form) and the block and level counts
of e4s_colsum_f32 (colsum_levels, constants COLSUM_RPB, COLSUM_MAX_PARTS and RCHUNK, which the host test reads back from optim.hip).

Two kinds of operand data (gen_bwd_cases.operand): random (fp32 normal values; alpha 0.2, gain sqrt(2), noise weight 0.3) and dyadic
(integers in [-4, 4] times 2^-2, alpha 0.5, gain 1, noise weight 0.5, dyadic FIR taps and masks).  With dyadic data every product and, as
long as S_abs / quantum < 2^24 (checked per case by the host test), every partial sum in any order is an fp32 number, so wherever no root,
no quotient and no non-dyadic scale is involved the output EQUALS the reference; each builder says per case where (`exact`).

Bounds for random data, u = 2^-24.  A sum of N terms in any order: (N + 1) u S_abs, S_abs the sum of the terms' absolute values (N - 1
additions and the second order; an FMA contraction only removes roundings).  Elementwise chains: one u |value| per rounding.  build.py
passes no fast-math flag: fp32 division and sqrtf count as correctly rounded.  rsqrtf gets enc_fwd_cases.RSQRT_U u.  Chains that multiply
several first-order terms carry the factor SECOND = 1 + 2^-6.
  fused_bias_act  v = x + b (1 u |v|, with a bias), t = v alpha on the negative branch (1 u), y = t scale (1 u): (nb + na + 1) u |y|.  The
                  branch is taken on the sign of fl(x + b) (or of ref), which is the sign of x + b: no allowance.  Codes 12 and 32: 0.0.
  channel_sum     N = outer step_b terms: (N + 1) u S_abs.
  upfirdn2d       T = the number of taps that meet a real (not inserted, not padded) sample: T products and their sum, (T + 1) u sum |x| |k|.
                  An output that meets none is exactly 0.0.
  conv1x1_small   a = sum of Cin products (Cin + 1) u S, a scale (1 u S scale), + bias (1 u |v|): dv = (Cin + 2) u S |scale| + u |v|, S = sum |x| |w|;
                  y = lrelu(v) gain: gain dv (the slope is <= 1, and a sign that flips inside dv changes y by <= gain dv) + 2 u |y|.
  noise_half      t = nw f + b: u |nw f| + u |t|;  y = lrelu(t) gain: gain dt + 2 u |y|.
  pixelnorm       s = sum of D squares ((D + 1) u s, all terms >= 0, and 1 u for the squares), s / D (1 u), + 1e-8 (1 u): (D + 4) u on the argument,
                  halved by the root; rsqrtf RSQRT_U u; the product 1 u: ((D + 4) / 2 + RSQRT_U + 1) u |y|.  A zero row: 0 x rsqrt(1e-8) = 0.0.
  add_scale       (a + b) scale: u |a + b| |scale| + u |y|;  scale = 1: the fp32 sum a + b, bit for bit (criteria.py relies on it).
  minibatch_stddev per element, G = group, A = mean |x| over the members: mean (G + 2) u A; d = x - mean: dd = dmean + u |d|;
                  var = sum d^2 / G: (2 / G) sum |d| dd + (G + 3) u var; + 1e-8: 1 u; the root halves and adds 1 u.  The mean over HW C elements
                  runs in double (2^-40 relative allowed); the cast 1 u |sd|.  Identical members with exact sums (dyadic data, or G <= 2):
                  d = 0 and the statistic is sqrtf(1e-8f) exactly.  Channels [0, C) are copies, channels above C are 0.0.
  const_input     a permutation: torch.equal.
  mask_mul_add    v = y m: u |v|;  accumulate: + u |out + v|.
  noise_bias_act  v = x + b + nw n in either order: u |nw n| + u (|x| + |b| + |nw n|) + u |v|;  y = lrelu(v) gain: gain dv + 2 u |y|.
  rowdot mode 0   r = a scale + bias, a = sum of K products: (K + 2) u S_abs |scale| + u |r|.
  rowdot mode 1   a = sum_k wsq s^2 (wsq >= 0: relative (K + 2) u, one more for the square), scale^2 (1 u), the product (1 u), + 1e-8 (1 u):
                  (K + 5) u on the argument, halved by the root; rsqrtf RSQRT_U u; the product 1 u: ((K + 5) / 2 + RSQRT_U + 1) u |r|.
  weight_sqsum    taps squares and their sum: (taps + 2) u sum w^2.
  colsum          N = rows terms per column: (N + 1) u S_abs.
  region_plan     no floating point: a structural check (check_plan).

Largest observed error / bound on the MI355X (printed by the GPU test at teardown): fused_bias_act 1.00 and mask_mul_add 1.00 / 0.98
accumulating (chains of one or two roundings reach their bound), add_scale 0.85, conv1x1_small 0.96, channel_sum 0.29, upfirdn2d generic
0.62, fir_nhwc 0.49, fir_nhwc_fixed<4, 4> 0.49, noise_half 0.45, pixelnorm 0.11, minibatch_stddev 0.15, noise_bias_act_nhwc 0.57, rowdot
mode 0 0.61 and mode 1 0.25, weight_sqsum 0.32, colsum 0.02.
"""
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import gen_bwd_cases as gc
from enc_fwd_cases import RSQRT_U
from gen_bwd_cases import CONSTS, KINDS, MAPS, make_labels, operand, region_map  # noqa: F401

U = 2.0 ** -24
SECOND = 1 + 2.0 ** -6
BM = 128                    # the row tile the plan pads its groups to (kernels.BM)


def f32(v):
    return float(np.float32(v))


EPS8 = f32(1e-8)
ROOT_EPS8 = f32(math.sqrt(EPS8))          # sqrtf(1e-8f), correctly rounded (the fp64 root rounded once more: innocuous for a root)


def _gen(name, cid, kind):
    return torch.Generator().manual_seed(zlib.crc32(f"glue-{name}-{cid}-{kind}".encode()))


def _lrelu(v, alpha):
    return torch.where(v > 0, v, v * alpha)


def consts(kind):
    c = CONSTS[kind]
    return f32(c["alpha"]), f32(c["gain"]), f32(c["noise_w"])


def case_id(c):
    return gc.case_id({k: ("x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in c.items()})


# ---- fused_bias_act ------------------------------------------------------------------------------------------------------------------------
FBA_CODES = ((1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2))
FBA_BLOCK, FBA_GRID_CAP = 256, 8192
# shape, offset (floats into the allocation at which the contiguous x / ref views start), codes run, forms expected (with bias, without)
FBA_CASES = [dict(zip(("tag", "shape", "offset", "codes", "forms"), row)) for row in [
    ("v4", (2, 8, 4, 4), 0, FBA_CODES, ("v4", "v4")),
    ("scalar-n105", (1, 3, 5, 7), 0, FBA_CODES, ("scalar", "scalar")),                        # n % 4 != 0
    ("scalar-step9", (4, 2, 3, 3), 0, FBA_CODES, ("scalar", "v4")),                           # step_b % 4 != 0, n % 4 == 0
    ("scalar-misaligned", (2, 4, 4, 4), 1, FBA_CODES, ("scalar", "scalar")),                  # a view 4 bytes into its allocation
    ("2d-step1", (5, 12), 0, FBA_CODES, ("scalar", "v4")),                                    # [B, C]: step_b = 1
    ("v4-gridstride", (2, 4, 1048704), 0, ((3, 0), (3, 1)), ("v4+loop", "v4+loop")),          # 8192 256 4 + 1024 floats
    ("scalar-gridstride", (1, 3, 699061), 0, ((3, 0), (3, 1)), ("scalar+loop", "scalar+loop")),  # 8192 256 + 31 floats, n % 4 = 3
]]


def fba_form(n, step_b, has_bias, offset):
    """the launch form e4s_fused_bias_act_f32 takes (its documented rule): v4 needs n % 4 == 0, step_b % 4 == 0 where there is a bias and
    16-byte aligned pointers; the grid is capped at 8192 blocks of 256, beyond which every thread loops"""
    vec = n % 4 == 0 and (not has_bias or step_b % 4 == 0) and offset % 4 == 0
    items = n // 4 if vec else n
    loop = -(-items // FBA_BLOCK) > FBA_GRID_CAP
    return ("v4" if vec else "scalar") + ("+loop" if loop else "")


def fba_step(shape):
    return int(np.prod(shape[2:])) if len(shape) > 2 else 1


def fba_ref(x, bias, ref, act, grad, alpha, scale):
    """fused_bias_act_kernel.cu:27-47 in fp64; (y, bound)"""
    alpha, scale = f32(alpha), f32(scale)
    v = x.double()
    if bias is not None:
        v = v + bias.double().view((1, -1) + (1,) * (x.ndim - 2))
    code = act * 10 + grad
    neg = torch.zeros_like(v, dtype=torch.bool)
    if code in (12, 32):
        return torch.zeros_like(v), torch.zeros_like(v)
    if code == 30:
        neg = ~(v > 0)
    elif code == 31:
        neg = ~(ref.double() > 0)
    y = torch.where(neg, v * alpha, v) * scale
    return y, U * ((0 if bias is None else 1) + neg.double() + 1) * y.abs() * (1 + 2.0 ** -20)


@functools.lru_cache(maxsize=2)          # the grid-stride cases hold 8 M elements
def fba_case(index, kind):
    c = FBA_CASES[index]
    g = _gen("fba", index, kind)
    shape = c["shape"]
    n = int(np.prod(shape))
    alpha, gain, _ = consts(kind)
    x, ref, bias = operand((n,), kind, g), operand((n,), kind, g), operand((shape[1],), kind, g)
    # the strict `>`: zeros of both signs in x (code 30, no bias) and in ref under a non-zero x (code 31)
    x[:8] = torch.tensor([0.0, -0.0, 0.75, -0.75, 0.75, -0.75, 0.0, -0.0])
    ref[:8] = torch.tensor([1.0, -1.0, 0.0, 0.0, -0.0, -0.0, 0.0, -0.0])
    x, ref = x.view(shape), ref.view(shape)
    xb = x.clone()                       # with a bias: x = -b at the planted zeros, so that x + b is +0.0 there
    step = fba_step(shape)
    flat = xb.view(-1)
    for i in (0, 1, 6, 7):
        flat[i] = -bias[(i // step) % shape[1]]
    out = dict(case=c, n=n, step_b=step, alpha=alpha, scale=gain, x=x, xb=xb, ref=ref, bias=bias, exact=kind == "dyadic", refs={})
    for act, grad in c["codes"]:
        for has_b in (False, True):
            out["refs"][(act, grad, has_b)] = fba_ref(xb if has_b else x, bias if has_b else None, ref, act, grad, alpha, gain)
    return out


# ---- channel_sum ---------------------------------------------------------------------------------------------------------------------------
CSUM_STEPS = (1, 15, 256, 257, 1000)
CSUM_OUTER = (1, 3)
CSUM_C = (1, 3, 64)


def sum_ref(terms, dims):
    """(sum, S_abs, N) of fp64 terms over dims"""
    n = int(np.prod([terms.shape[d] for d in dims]))
    return terms.sum(dims), terms.abs().sum(dims), n


@functools.lru_cache(maxsize=None)
def csum_case(step_b, outer, C, kind):
    g = _gen("csum", f"{step_b}-{outer}-{C}", kind)
    x = operand((outer, C, step_b), kind, g)
    s, sabs, n = sum_ref(x.double(), (0, 2))
    return dict(x=x, ref=s, sabs=sabs, n=n, bound=(n + 1) * U * sabs, exact=kind == "dyadic", quantum=0.25)


# ---- upfirdn2d -----------------------------------------------------------------------------------------------------------------------------
TOH, TOW = 16, 64           # the generic kernel's output tile


def upfirdn_path(c):
    """the kernel e4s_upfirdn2d_f32 dispatches to (its documented rule)"""
    kh, kw = c["k"]
    if c["up"] == (1, 1) and c["down"] == (1, 1) and c["minor"] % 4 == 0 and 8 <= c["minor"] <= 1024 and kh * kw <= 64 and c["major"] <= 65535:
        return "fir_nhwc_fixed44" if (kh, kw) == (4, 4) else "fir_nhwc"
    return "generic"


def _solve(out, k, up, down, p0, p1):
    """the smallest input extent (and the far pad, reduced where needed) whose output extent is exactly `out`"""
    n = max(1, -(-((out - 1) * down + k - p0 - p1) // up))
    excess = n * up + p0 + p1 - k - (out - 1) * down
    assert excess >= 0
    if excess > down - 1:
        p1 -= excess - (down - 1)
    assert (n * up + p0 + p1 - k) // down + 1 == out and n * up + p0 + p1 - k >= 0
    return n, p1


def _ufd(tag, major, minor, k, up, down, pad, out):
    """up = (x, y), down = (x, y), pad = (x0, x1, y0, y1) as wanted, out = (h, w): the input size is solved for"""
    in_h, py1 = _solve(out[0], k[0], up[1], down[1], pad[2], pad[3])
    in_w, px1 = _solve(out[1], k[1], up[0], down[0], pad[0], pad[1])
    return dict(tag=tag, major=major, minor=minor, k=k, up=up, down=down, pad=(pad[0], px1, pad[2], py1), size=(in_h, in_w), out=out)


UFD_GENERIC = [
    _ufd("generic-1tile", 6, 1, (4, 4), (1, 1), (1, 1), (1, 1, 1, 1), (16, 64)),
    _ufd("generic-multitile", 6, 1, (4, 4), (1, 1), (1, 1), (2, 1, 2, 1), (17, 65)),
    _ufd("generic-multitile-up2", 2, 3, (3, 3), (2, 2), (1, 1), (2, 1, 2, 1), (33, 130)),
    _ufd("generic-multitile-down2", 1, 6, (4, 4), (1, 1), (2, 2), (1, 1, 1, 1), (33, 130)),
    _ufd("generic-multitile-up2-down2", 2, 3, (2, 2), (2, 2), (2, 2), (0, 0, 0, 0), (17, 65)),
    _ufd("generic-multitile-up3-down2", 1, 6, (5, 3), (3, 3), (2, 2), (2, 2, 1, 3), (33, 130)),
    _ufd("generic-up2-down3-k16", 6, 1, (16, 16), (2, 2), (3, 3), (8, 7, 8, 7), (16, 64)),
    _ufd("generic-minor4", 1, 4, (4, 4), (1, 1), (1, 1), (2, 1, 2, 1), (17, 65)),                         # minor < 8: falls back
    _ufd("generic-minor1028", 1, 1028, (3, 3), (1, 1), (1, 1), (1, 1, 1, 1), (5, 6)),                     # minor > 1024: falls back
    _ufd("generic-65taps", 2, 8, (5, 13), (1, 1), (1, 1), (6, 6, 2, 2), (17, 65)),                        # 65 taps: falls back
    _ufd("generic-1x1", 2, 3, (1, 1), (1, 1), (1, 1), (0, 0, 0, 0), (1, 1)),
    _ufd("generic-1x1-of-k16", 1, 3, (16, 16), (1, 1), (1, 1), (0, 0, 0, 0), (1, 1)),
    _ufd("generic-negative-pads", 2, 3, (3, 3), (1, 1), (1, 1), (-1, -2, -2, -1), (16, 64)),
    _ufd("generic-one-negative-pad-up2", 2, 3, (4, 4), (2, 2), (1, 1), (-1, 3, 3, -1), (17, 65)),
    _ufd("generic-multitile-upx2-downy2", 2, 3, (4, 4), (2, 1), (1, 2), (2, 1, 0, 1), (33, 130)),         # up_x != up_y, down_x != down_y
    _ufd("generic-multitile-upy3-downx2", 1, 6, (5, 3), (1, 3), (2, 1), (1, 0, 3, 2), (17, 65)),
]
_FIR_GEOM = [          # tag, major, minor, k, pad, out;  ppb = 256 // (minor / 4) pixels per block
    ("ppb128-whole", 1, 8, (1, 1), (0, 0, 0, 0), (4, 128)),
    ("ppb85-idle-lane", 3, 12, (3, 3), (1, 1, 1, 1), (5, 86)),
    ("ppb42-whole", 1, 24, (2, 5), (2, 2, 0, 1), (7, 42)),
    ("ppb1-544", 3, 544, (8, 8), (4, 3, 4, 3), (5, 3)),
    ("ppb1-1024-negative-pads", 1, 1024, (3, 3), (-1, -1, -2, -1), (3, 2)),
    ("ppb128-two-blocks-negative-pad", 3, 8, (8, 8), (3, -1, -1, 4), (9, 130)),
]
UFD_FIR = [_ufd("fir_nhwc-" + t, ma, mi, k, (1, 1), (1, 1), p, o) for t, ma, mi, k, p, o in _FIR_GEOM]
UFD_FIXED = [_ufd("fir_nhwc_fixed44-" + t, ma, mi, (4, 4), (1, 1), (1, 1), p, o) for t, ma, mi, k, p, o in _FIR_GEOM]
UFD_CASES = UFD_GENERIC + UFD_FIR + UFD_FIXED
UFD_EXPECT = ["generic"] * len(UFD_GENERIC) + ["fir_nhwc"] * len(UFD_FIR) + ["fir_nhwc_fixed44"] * len(UFD_FIXED)


def upfirdn_ref(x, k, up, down, pad):
    """x [major, H, W, minor] fp32, k [kh, kw]: zero insertion, pad / crop, F.conv2d with the flipped kernel in fp64, stride;
    (y [major, Ho, Wo, minor], S_abs, T) with T the number of taps that meet a real sample."""
    major, H, W, minor = x.shape
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    kd = torch.flip(k.double(), [0, 1])[None, None]

    def run(t, kk):
        z = t.new_zeros(t.shape[0], 1, H * uy, W * ux)
        z[:, :, ::uy, ::ux] = t
        z = F.pad(z, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
        z = z[:, :, max(-py0, 0): z.shape[2] - max(-py1, 0), max(-px0, 0): z.shape[3] - max(-px1, 0)]
        o = F.conv2d(z, kk)[:, :, ::dy, ::dx]
        return o.reshape(major, minor, o.shape[2], o.shape[3]).permute(0, 2, 3, 1).contiguous()

    xd = x.double().permute(0, 3, 1, 2).reshape(major * minor, 1, H, W)
    return run(xd, kd), run(xd.abs(), kd.abs()), run(torch.ones_like(xd[:1].expand(major * minor, 1, H, W)), torch.ones_like(kd))


@functools.lru_cache(maxsize=None)
def ufd_case(index, kind):
    c = UFD_CASES[index]
    g = _gen("ufd", c["tag"], kind)
    x = operand((c["major"], c["size"][0], c["size"][1], c["minor"]), kind, g)
    k = operand(c["k"], kind, g)
    if kind == "dyadic":
        k[0, 0] = 0.75              # never all zero
    y, sabs, T = upfirdn_ref(x, k, c["up"], c["down"], c["pad"])
    assert tuple(y.shape[1:3]) == c["out"], (c["tag"], y.shape)
    return dict(case=c, x=x, k=k, ref=y, sabs=sabs, taps=T, bound=(T + 1) * U * sabs, exact=kind == "dyadic", quantum=2.0 ** -4)


# ---- conv1x1_small -------------------------------------------------------------------------------------------------------------------------
C1_CIN, C1_COUT, C1_HW, C1_B = (1, 3, 4), (4, 32, 36), ((1, 1), (7, 9), (1, 257)), 3


def conv1x1_ref(x, w, bias, scale, act, alpha, gain):
    """x NCHW, w [Cout, Cin]: act(x . w scale + bias) as NHWC in fp64; (y, bound)"""
    scale, alpha, gain = f32(scale), f32(alpha), f32(gain)
    cin = x.shape[1]
    a = torch.einsum("bchw,oc->bhwo", x.double(), w.double())
    S = torch.einsum("bchw,oc->bhwo", x.double().abs(), w.double().abs())
    v = a * scale + (0 if bias is None else bias.double())
    dv = U * ((cin + 2) * S * abs(scale) + v.abs())
    if not act:
        return v, dv * SECOND
    y = _lrelu(v, alpha) * gain
    return y, (gain * dv + 2 * U * y.abs()) * SECOND


@functools.lru_cache(maxsize=None)
def c1_case(cin, cout, hw, kind):
    g = _gen("c1", f"{cin}-{cout}-{hw}", kind)
    alpha, gain, _ = consts(kind)
    x, w, bias = operand((C1_B, cin, hw[0], hw[1]), kind, g), operand((cout, cin), kind, g), operand((cout,), kind, g)
    scale = f32(1 / math.sqrt(cin))
    t = dict(x=x, w=w, bias=bias, scale=scale, alpha=alpha, gain=gain, exact=kind == "dyadic" and cin in (1, 4), refs={})
    for has_b in (False, True):
        for act in (0, 1):
            t["refs"][(has_b, act)] = conv1x1_ref(x, w, bias if has_b else None, scale, act, alpha, gain)
    return t


# ---- noise_half ----------------------------------------------------------------------------------------------------------------------------
NH_C = (4, 36)
NH_SHAPE = (2, 3, 5)


def nh_layouts(C):
    """(Cy, coff): the second half of a 2C tensor, and the first channels of a wider one"""
    return ((2 * C, C), (2 * C + 8, 0))


@functools.lru_cache(maxsize=None)
def nh_case(C, kind):
    g = _gen("nh", C, kind)
    alpha, gain, nw = consts(kind)
    feat, bias = operand(NH_SHAPE + (C,), kind, g), operand((C,), kind, g)
    p = nw * feat.double()
    t = p + bias.double()
    y = _lrelu(t, alpha) * gain
    dt = U * (p.abs() + t.abs())
    return dict(feat=feat, bias=bias, nw=nw, alpha=alpha, gain=gain, ref=y, bound=(gain * dt + 2 * U * y.abs()) * SECOND, exact=kind == "dyadic")


# ---- pixelnorm -----------------------------------------------------------------------------------------------------------------------------
PN_B, PN_D = (1, 4, 5), (1, 63, 64, 65, 512, 1000)


@functools.lru_cache(maxsize=None)
def pn_case(B, D, kind):
    g = _gen("pn", f"{B}-{D}", kind)
    x = operand((B, D), kind, g)
    x[:, 0] = 0.75
    if B > 1:
        x[B - 1] = 0.0              # an all-zero row
    xd = x.double()
    y = xd * torch.rsqrt(xd.pow(2).mean(1, keepdim=True) + EPS8)
    return dict(x=x, ref=y, bound=((D + 4) / 2 + RSQRT_U + 1) * U * y.abs() * SECOND, zero_row=B - 1 if B > 1 else None)


# ---- add_scale -----------------------------------------------------------------------------------------------------------------------------
AS_N = (4, 1020, 2 ** 20 + 4)
AS_SCALE = f32(1 / math.sqrt(2))


@functools.lru_cache(maxsize=None)
def as_case(n, kind):
    g = _gen("as", n, kind)
    a, b = operand((n,), kind, g), operand((n,), kind, g)
    s = a.double() + b.double()
    y = s * AS_SCALE
    return dict(a=a, b=b, ref1=s, ref=y, bound=U * (s.abs() * AS_SCALE + y.abs()) * (1 + 2.0 ** -20))


# ---- minibatch_stddev ----------------------------------------------------------------------------------------------------------------------
MS_GROUPS = ((4, 4), (8, 4), (6, 2), (1, 1))
MS_HW, MS_C = ((1, 1), (4, 4)), (4, 20)


def ms_widths(C):
    return (C + 1, (C + 1 + 31) // 32 * 32)


def ms_ref(x, group):
    """model.py:783-790 (stddev_feat = 1) for NHWC x in fp64: (statistic per sample [B], bound [B])"""
    B, H, W, C = x.shape
    M = B // group
    xs = x.double().view(group, M, H, W, C)
    mean = xs.mean(0)
    d = xs - mean
    var = d.pow(2).mean(0)
    sd = torch.sqrt(var + EPS8)
    A = xs.abs().mean(0)
    dd = (group + 2) * U * A + U * d.abs()
    dvar = (2 / group) * (d.abs() * dd).sum(0) + (group + 3) * U * var
    dsd = (dvar + U * (var + EPS8)) / (2 * sd) + U * sd
    stat = sd.mean((1, 2, 3))
    bound = SECOND * dsd.mean((1, 2, 3)) + (U + 2.0 ** -40) * stat
    return stat.repeat(group), bound.repeat(group)


@functools.lru_cache(maxsize=None)
def ms_case(B, group, hw, C, kind, identical=False):
    g = _gen("ms", f"{B}-{group}-{hw}-{C}-{int(identical)}", kind)
    x = operand((B, hw[0], hw[1], C), kind, g)
    if identical:
        x = x[:B // group].repeat(group, 1, 1, 1).contiguous()
    stat, bound = ms_ref(x, group)
    return dict(x=x, stat=stat, bound=bound)


def ms_identical_exact(group, kind):
    """the sums of identical members are exact: dyadic data, or at most 2 members (x + x and its half are exact)"""
    return kind == "dyadic" or group <= 2


# ---- const_input ---------------------------------------------------------------------------------------------------------------------------
CI_B, CI_C, CI_GRIDS = (1, 3), (4, 33, 512), ((4, 4), (5, 7))


# ---- mask_mul_add --------------------------------------------------------------------------------------------------------------------------
MM_GRIDS = ((5, 7), (13, 37))
MM_B, MM_C, MM_R = 2, 3, 3


@functools.lru_cache(maxsize=None)
def mm_case(grid, rel, channels_last, kind):
    g = _gen("mm", f"{grid}-{rel}-{int(channels_last)}", kind)
    H, W = grid
    hm, wm = MAPS[grid][rel]
    shape = (MM_B, H, W, MM_C) if channels_last else (MM_B, MM_C, H, W)
    y, acc = operand(shape, kind, g), operand(shape, kind, g)
    mask = operand((MM_B, MM_R, hm, wm), kind, g).abs() if kind == "dyadic" else torch.rand(MM_B, MM_R, hm, wm, generator=g)      # soft
    near = F.interpolate(mask, size=(H, W), mode="nearest").double()                       # [B, R, H, W]
    refs = {}
    for r in (0, MM_R - 1):
        m = near[:, r, :, :, None] if channels_last else near[:, r, None]
        v = y.double() * m
        refs[r] = (v, U * v.abs(), acc.double() + v, U * (v.abs() + (acc.double() + v).abs()))
    return dict(y=y, acc=acc, mask=mask, refs=refs, exact=kind == "dyadic")


# ---- noise_bias_act_nhwc -------------------------------------------------------------------------------------------------------------------
NB_C = (3, 4, 36)
NB_SHAPE = (3, 5, 7)
NB_NOISE = ("none", "shared", "per-sample")


@functools.lru_cache(maxsize=None)
def nb_case(C, kind):
    g = _gen("nb", C, kind)
    alpha, gain, nw = consts(kind)
    B, H, W = NB_SHAPE
    x, bias, noise = operand((B, H, W, C), kind, g), operand((C,), kind, g), operand((B, H, W), kind, g)
    t = dict(x=x, bias=bias, noise=noise, nw=nw, alpha=alpha, gain=gain, exact=kind == "dyadic", refs={})
    for mode in NB_NOISE:
        nz = torch.zeros(1, 1, 1, 1, dtype=torch.float64) if mode == "none" else nw * (noise[:1] if mode == "shared" else noise).double()[..., None]
        v = x.double() + bias.double() + nz
        dv = U * (nz.abs() + (x.double().abs() + bias.double().abs() + nz.abs()) + v.abs())
        y = _lrelu(v, alpha) * gain
        t["refs"][mode] = (y, (gain * dv + 2 * U * y.abs()) * SECOND)
    return t


# ---- rowdot (single launch) and weight_sqsum -----------------------------------------------------------------------------------------------
RD_G, RD_O, RD_K = (1, 8, 9, 24), (1, 3, 4, 5), (4, 252, 256, 260, 512)
RD_LATENT = (2, 3, 3)          # B, R, L of the strided latent of `modulate`
RD_CONV_SCALE = {"dyadic": 0.25, "random": f32(1 / math.sqrt(512 * 9))}


def rd_scale(K):
    return f32(1 / math.sqrt(K))


def rowdot0_ref(style, M, bias, scale):
    """r = (style . M^T) scale + bias in fp64; (r, bound, S_abs)"""
    K = style.shape[-1]
    a, S = style.double() @ M.double().t(), style.double().abs() @ M.double().abs().t()
    r = a * scale + bias.double()
    return r, U * ((K + 2) * S * abs(scale) + r.abs()) * (1 + 2.0 ** -20), S


def rowdot1_ref(s, wsq, scale):
    """r = scale rsqrt(scale^2 sum_k wsq s^2 + 1e-8) in fp64 (scale an fp32 number, scale^2 formed in double); (r, bound)"""
    K = s.shape[-1]
    a = s.double().pow(2) @ wsq.double().t()
    r = scale * torch.rsqrt(scale * scale * a + EPS8)
    return r, ((K + 5) / 2 + RSQRT_U + 1) * U * r.abs() * SECOND


@functools.lru_cache(maxsize=None)
def rd_case(G, O, K, kind):
    g = _gen("rd", f"{G}-{O}-{K}", kind)
    style, M, bias = operand((G, K), kind, g), operand((O, K), kind, g), operand((O,), kind, g)
    wsq = M.pow(2) * 2.0             # >= 0, dyadic where M is
    cs = RD_CONV_SCALE[kind]
    r0, b0, S = rowdot0_ref(style, M, bias, rd_scale(K))
    return dict(style=style, M=M, bias=bias, wsq=wsq, conv_scale=cs, mode0=(r0, b0), sabs=S, mode1=rowdot1_ref(style, wsq, cs),
                exact0=kind == "dyadic" and K in (4, 256), quantum=2.0 ** -4)


@functools.lru_cache(maxsize=None)
def rd_latent_case(K, O, kind):
    """latent [B, R, L, K]: layer l of every (sample, region) (masked) or of region 0 of every sample"""
    g = _gen("rdl", f"{K}-{O}", kind)
    B, R, L = RD_LATENT
    latent, M, bias = operand((B, R, L, K), kind, g), operand((O, K), kind, g), operand((O,), kind, g)
    refs = {}
    for layer in range(L):
        for masked in (False, True):
            st = latent[:, :, layer].reshape(B * R, K) if masked else latent[:, 0, layer]
            refs[(layer, masked)] = rowdot0_ref(st, M, bias, rd_scale(K))[:2]
    return dict(latent=latent, M=M, bias=bias, refs=refs, exact0=kind == "dyadic" and K in (4, 256))


WS_SHAPES, WS_TAPS = ((3, 4), (64, 32), (1, 257)), (1, 9)


@functools.lru_cache(maxsize=None)
def ws_case(shape, taps, kind):
    g = _gen("ws", f"{shape}-{taps}", kind)
    k = 1 if taps == 1 else 3
    w = operand(shape + (k, k), kind, g)
    s = w.double().pow(2).sum((2, 3))
    return dict(w=w, ref=s, bound=(taps + 2) * U * s, exact=kind == "dyadic", terms=w.pow(2).reshape(shape + (taps,)))


# ---- colsum --------------------------------------------------------------------------------------------------------------------------------
COLSUM_RPB, COLSUM_MAX_PARTS, RCHUNK = 2048, 1024, 64          # csrc/optim.hip: colsum_rpb and reduce_chunks (read back by the host test)
COLSUM_DIRECT = 64                                             # kernels.colsum: up to 64 rows go to batch_sum


def colsum_levels(rows, C):
    """(path, rows per block, parts, reduction levels) of kernels.colsum"""
    if rows <= COLSUM_DIRECT or C % 4 or C > 1024:
        return "batch_sum", rows, 1, 0
    rpb = COLSUM_RPB
    while -(-rows // rpb) > COLSUM_MAX_PARTS:
        rpb *= 2
    parts = -(-rows // rpb)
    return "colsum", rpb, parts, 2 if parts > RCHUNK else 1


COLSUM_CASES = [dict(zip(("tag", "rows", "C"), row)) for row in [
    ("batch_sum-64rows", 64, 36), ("batch_sum-C6", 65, 6),
    ("first-colsum", 65, 4), ("first-colsum", 65, 36), ("first-colsum", 65, 1024),
    ("one-block", COLSUM_RPB, 4), ("one-block", COLSUM_RPB, 36), ("one-block", COLSUM_RPB, 1024), ("two-blocks", COLSUM_RPB + 1, 36),
    ("one-level-64-parts", RCHUNK * COLSUM_RPB, 4),
    ("second-level", RCHUNK * COLSUM_RPB + 1, 4), ("second-level", RCHUNK * COLSUM_RPB + 1, 36),
    ("rpb-doubles", COLSUM_MAX_PARTS * COLSUM_RPB + 1, 4),
]]


@functools.lru_cache(maxsize=4)
def colsum_case(index, kind):
    c = COLSUM_CASES[index]
    g = _gen("colsum", index, kind)
    x = operand((c["rows"], c["C"]), kind, g)
    s, sabs, n = sum_ref(x.double(), (0,))
    return dict(case=c, x=x, ref=s, sabs=sabs, n=n, bound=(n + 1) * U * sabs, exact=kind == "dyadic", quantum=0.25)


# ---- region_plan ---------------------------------------------------------------------------------------------------------------------------
PLAN_ANCHORS = ((5, 7), (13, 37))
PLAN_CASES = [dict(anchors=a, rel=rel, nphase=nph, B=B, R=R) for a in PLAN_ANCHORS for rel in ("larger", "equal", "smaller")
              for nph in (1, 4) for B, R in ((1, 3), (3, 12))]


def plan_out_grid(c):
    os_ = 2 if c["nphase"] == 4 else 1
    return c["anchors"][0] * os_, c["anchors"][1] * os_


def plan_labels(c, pattern):
    hm, wm = MAPS[plan_out_grid(c)][c["rel"]]
    return make_labels(pattern, c["B"], hm, wm, c["R"], seed=zlib.crc32(f"plan-{case_id(c)}-{pattern}".encode()) & 0xffff)


def plan_groups(labels, B, R, ha, wa, nphase):
    """{key: set of anchors}: key = (sample R + region) nphase + phase, the region that of the row's OUTPUT pixel -- (ay, ax) for nphase 1,
    (2 ay + (phase >> 1), 2 ax + (phase & 1)) of the doubled grid for nphase 4 -- by F.interpolate nearest"""
    os_ = 2 if nphase == 4 else 1
    reg = region_map(labels, ha * os_, wa * os_).numpy()
    groups = {}
    for b in range(B):
        for ay in range(ha):
            for ax in range(wa):
                for ph in range(nphase):
                    r = int(reg[b, ay * os_ + (ph >> 1), ax * os_ + (ph & 1)])
                    groups.setdefault((b * R + r) * nphase + ph, set()).add((b * ha + ay) * wa + ax)
    return groups


def check_plan(rows, tiles, meta, labels, B, R, ha, wa, nphase, bm=BM):
    """Raises AssertionError unless (rows, tiles, meta) -- int arrays as e4s_region_plan leaves them -- is a plan of `labels`: every
    (anchor, phase) exactly once, in the group of its output pixel's region; the groups at the tile table's offsets, padded to bm with -1;
    tile entries [row offset, group, phase, live count] whose counts add up to the histogram; meta[0], meta[1] the tile and padded-row
    totals; no tile for an absent region.  The order of the rows within a group is not part of the contract."""
    rows, tiles, meta = (np.asarray(v).astype(np.int64) for v in (rows, tiles, meta))
    want = plan_groups(labels, B, R, ha, wa, nphase)
    ntiles, nrows = int(meta[0]), int(meta[1])
    need = sum(-(-len(v) // bm) for v in want.values())
    assert ntiles == need, f"meta[0] = {ntiles}, the histogram needs {need} tiles"
    assert nrows == need * bm, f"meta[1] = {nrows}, not {need} tiles of {bm} rows"
    assert nrows <= rows.size and ntiles * 4 <= tiles.size
    t = tiles[:ntiles * 4].reshape(ntiles, 4)
    assert sorted(t[:, 0].tolist()) == list(range(0, nrows, bm)), "the tiles' row offsets do not tile [0, meta[1])"
    got, live = {}, {}
    for off, grp, ph, cnt in t.tolist():
        assert 0 <= ph < nphase and 0 <= grp < B * R and 1 <= cnt <= bm, f"tile entry {[off, grp, ph, cnt]}"
        key = grp * nphase + ph
        assert key in want, f"a tile for the absent group {grp} phase {ph}"
        seg = rows[off:off + bm]
        assert (seg[:cnt] >= 0).all() and (seg[cnt:] == -1).all(), f"tile at {off}: {cnt} live rows, then -1"
        got.setdefault(key, []).extend(seg[:cnt].tolist())
        live.setdefault(key, []).append((off, cnt))
    assert (rows[nrows:] == -1).all(), "rows past meta[1] are not -1"
    assert set(got) == set(want), "groups with rows but without a tile"
    for key, anchors in want.items():
        offs = sorted(live[key])
        assert [o for o, _ in offs] == list(range(offs[0][0], offs[0][0] + bm * len(offs), bm)), f"group {key}: its tiles are not consecutive"
        assert all(c == bm for _, c in offs[:-1]), f"group {key}: a tile before the last is not full"
        assert sum(c for _, c in offs) == len(anchors), f"group {key}: {sum(c for _, c in offs)} rows, the histogram has {len(anchors)}"
        assert len(set(got[key])) == len(got[key]), f"group {key}: an anchor twice"
        assert set(got[key]) == anchors, f"group {key}: not the anchors of its region"


def plan_numpy(labels, B, R, ha, wa, nphase, bm=BM, rows_cap=None):
    """a correct plan, built from plan_groups in key order (the host test's positive control)"""
    groups = plan_groups(labels, B, R, ha, wa, nphase)
    nkeys = B * R * nphase
    rows_cap = B * ha * wa * nphase + nkeys * bm if rows_cap is None else rows_cap
    rows, tiles = np.full(rows_cap, -1, dtype=np.int32), []
    off = 0
    for key in sorted(groups):
        a = sorted(groups[key])
        for t in range(0, len(a), bm):
            part = a[t:t + bm]
            rows[off:off + len(part)] = part
            tiles.append([off, key // nphase, key % nphase, len(part)])
            off += bm
    tl = np.full(((rows_cap + bm - 1) // bm) * 4, -7, dtype=np.int32)
    tl[:len(tiles) * 4] = np.asarray(tiles, dtype=np.int32).reshape(-1)
    return rows, tl, np.asarray([len(tiles), off, 0, 0], dtype=np.int32)
