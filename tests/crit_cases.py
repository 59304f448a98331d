"""Seeded cases and fp64 yardsticks for the loss networks' glue (csrc/criteria.hip: adaptive_pool and its gradient, the stem convs
conv_smallcin / conv_smallcin_bwd / col2im, maxpool3s2, maxpool2 and their gradients, relu_bwd, lpips_layer and its gradient, cosine and
its gradient, norm_bwd_frozen): the yardsticks of tests/test_crit_cases_host.py and tests/test_gpu_criteria_kernels.py.  CPU only; the
native library is not imported here.

Every reference takes the fp32 operands cast to double and is a plain statement of the operation: F.adaptive_avg_pool2d of the crop and
the affine, F.conv2d, F.fold (col2im), F.max_pool2d(return_indices=True), fp64 autograd of those for the gradients, and the written
formulas of the LPIPS distance (lpips.py:32-33 with normalize_activation), of the cosine terms and of the frozen normalisation.  None
restates a kernel's loop.  The one piece of kernel arithmetic restated here is the chunk length of the cosine partial sums (cos_chunk),
which the workspace check and the path classifier need.  `bins` is the definition of F.adaptive_avg_pool2d's bins (start = floor(o in /
out), end = ceil((o + 1) in / out)); it gives the bin areas and the number of bins over a pixel that the bounds count with.

Two kinds of operand data (gen_bwd_cases.operand): random (fp32 normal values) and dyadic (integers in [-4, 4] times 2^-2, with dyadic
scales, gates and weights).  With dyadic data every product and every partial sum in any order is an fp32 number wherever no quotient by
a non-power of two and no root is involved, and the output EQUALS the reference; each builder says per case where (`exact`), and the host
test proves it by evaluating the same formula in fp32.

Bounds for random data, u = 2^-24, one line per rounding, from the kernels' operation chains (an FMA contraction only removes roundings).
build.py passes no fast-math flag: fp32 division and sqrtf count as correctly rounded, with no allowance.
  pool     acc = the fp32 sum of the n = |bin| pixels, v = acc / n, y = v scale + shift.  A = mean |x| over the bin:
             the sum of n terms in any order      (n + 1) u A
             the quotient                          1 u A                                   no affine: (n + 2) u A
             the product with scale                1 u A |scale|
             the addition of shift                 1 u |y|      + 1 u A |scale| second order:  (n + 4) u A |scale| + u |y|
           n = 1 and no affine: 0 + x and x / 1 are exact, torch.equal in both kinds (identity and integer up-sampling).
  pool_bwd dx = (sum over the m bins that contain the pixel of fl(dy / |bin|)) scale.  T = |scale| sum |dy| / |bin|:
             each quotient                         1 u T
             the sum of m terms                    (m + 1) u T
             the product with scale                1 u T                                    (m + 3) u T;  0 outside the crop
           one bin of a power-of-two area and no scale: exact in both kinds.
  conv     acc = bias, then n = k k Cin fused multiply-adds: a sum of n + 1 terms, (n + 2) u (|bias| + sum |x| |w|); ReLU is 1-Lipschitz.
           Outputs whose window lies wholly in the padding equal the bias (its ReLU) exactly.
  conv_bwd a sum of N = ceil(k / stride)^2 Cout products in some order -- four products at a time in the per-pixel kernel, Cout at a
           time on the MFMA and then <= ceil(k / stride)^2 of those in col2im: (N + 1) u sum |dy| |w|.  Image pixels no output sees: 0.
  col2im   on a hand-made fp32 z: the reference is the fp64 F.fold of THAT z; a sum of n <= ceil(k / stride)^2 terms: (n + 1) u sum |z|.
  maxpool  values and window codes: no arithmetic, torch.equal.  maxpool3s2_bwd: a sum of <= 4 terms, 5 u sum |dy|; maxpool2_bwd: a copy.
  relu_bwd no arithmetic but the accumulation, one correctly rounded addition: torch.equal with dy [y > 0] (+ acc in fp32).
  lpips    per pixel s = sum f^2 (C terms, fp32, lanes then a butterfly), r = sqrtf(s), i = 1 / (r + eps), n = f i, t = nx - ny,
           d = sum_c w t t.  Relative to i:
             s: C squares and their sum            (C + 1) u, halved by the root
             the root, the addition of eps, the quotient                      3 u          rho = ((C + 1) / 2 + 3) u
           dt = (rho + u)(|nx| + |ny|) + u |t|   (the two products; the subtraction)
           d: |w| (2 |t| dt + 2 u t^2) per channel (two products), the sum of C terms (C + 1) u sum |w| t^2.
           out = (float)(sum_p d in double x (double)fl(1 / HW)): 2 u |out| and (HW + 2) 2^-53 mean_p sum |w| t^2.
  lpips_bwd g = fl(gout fl(gmul / HW)), dn = 2 w t g, dot = sum dn fx, k2 = dot i i / r, dfx = dn i - fx k2:
             dn: |2 w g| dt + 5 u |dn|             (two products, the two roundings of g, one second order)
             dot: (C + 1) u sum |dn fx| + sum ddn |fx|
             k2: (ddot + |dot| (3 rho + 3 u)) i^2 / r     (i twice, r, three operations);  r = 0: k2 = 0
             dfx: ddn i + |dn| i (rho + u) + |fx| dk2 + u |fx k2| + u |dfx|
           Both lpips bounds are multiplied by 1 + 2^-6 for the products of these terms (rho is up to 260 u).
           At a pixel whose fx is all zero the kernel returns dn / eps, the limit of the closed form; torch autograd returns NaN there
           (the derivative of the root at 0).  The reference is the closed form; the host test shows that it is autograd's value at
           every other pixel.
  cosine   the three sums in double (fp32 x fp32 products are exact in double), finalised in double, cast once.  eD = (D + 8) 2^-53:
             cos    u |cos|   + eD (sum |a b| / (|a| |b|) + 2 |cos|)
             alpha  u alpha   + 2 eD alpha
             beta   u |beta|  + eD (sum |a b| / (|a|^3 |b|) + 4 |beta|)
  cosine_bwd da = g (alpha b + beta a), g = fl(gout gmul), with the fp32 coefficients THE KERNEL RETURNED:
             the two products, the addition (1 u each on |alpha b| + |beta a|, doubled for the second order)   2 u |g| (|alpha b| + |beta a|)
             g and the last product, one second order                                                            3 u |da|
  norm_bwd dx = rstd (gate dy + extra): the product and the addition u (|gate dy| + |gate dy + extra|) |rstd|, the last product and one
           second order 2 u |dx|.
  accumulate forms: got = fl(acc + v) where v is the plain form before its last rounding if the compiler contracts the last product
           into the addition: |got - (acc + plain)| <= u |acc + plain| + u |plain|; torch.equal where the plain form is exact (dyadic).

No case showed a residue of fp32 division or sqrtf on the MI355X: the bounds carry no allowance for either and hold (the pool, whose chain
is a sum and one quotient by a bin area that is mostly no power of two, reaches 0.78 of its bound; the LPIPS chain with its root 0.14).

Largest observed error / bound on the MI355X (printed by the GPU test at teardown; also MEASURED_RATIOS below): adaptive_pool 0.78, its
gradient 0.48, the adjoint identity 0.012; conv_smallcin 0.33, its gradient per pixel 0.06 and as GEMM + col2im 0.003, col2im on a hand-made z
0.23; maxpool3s2_bwd 0.32; lpips_layer 0.14, its gradient 0.09 (worst-case term counts over up to 512 channels); cosine 0.98 (the one cast),
its gradient 0.54; norm_bwd_frozen 0.60; the accumulate forms 0.94 .. 1.00 (one rounding).
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import gen_bwd_cases as gc
from gen_bwd_cases import KINDS, operand  # noqa: F401

U = 2.0 ** -24
SECOND = 1 + 2.0 ** -6          # lpips: the products of the first-order terms


def f32(v):
    return float(np.float32(v))


LP_EPS = f32(1e-10)             # the fp32 number the kernel adds to the norm
LP_MAX_C = 512

# worst error / bound per kernel output measured on the MI355X with the bounds above (module docstring)
MEASURED_RATIOS = {
    "adaptive_pool": 0.776, "adaptive_pool_bwd": 0.476, "adaptive_pool adjoint": 0.012,
    "conv_smallcin": 0.326, "conv_smallcin_bwd (per pixel)": 0.058, "conv_smallcin_bwd (GEMM + col2im)": 0.003, "conv_smallcin_col2im": 0.228,
    "maxpool3s2_bwd": 0.322, "lpips_layer": 0.141, "lpips_layer_bwd": 0.089, "cosine": 0.977, "cosine_bwd": 0.537, "norm_bwd_frozen": 0.595,
    # accumulate forms against acc + plain: one rounding, so the ratio reaches 1
    "adaptive_pool_bwd (accumulate)": 1.000, "lpips_layer_bwd (accumulate)": 0.999, "cosine_bwd (accumulate)": 0.999, "norm_bwd_frozen (accumulate)": 0.943,
}


def _gen(name, cid, kind):
    return torch.Generator().manual_seed(zlib.crc32(f"crit-{name}-{cid}-{kind}".encode()))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


# ---- adaptive pooling ----------------------------------------------------------------------------------------------------------------------
def bins(n_in, n_out):
    """[(start, end)] of F.adaptive_avg_pool2d's bins along one axis: start = floor(o in / out), end = ceil((o + 1) in / out)"""
    return [((o * n_in) // n_out, -((-(o + 1) * n_in) // n_out)) for o in range(n_out)]


def bins_over(n_in, n_out):
    """per input index, the bins that contain it, by search over every bin"""
    bs = bins(n_in, n_out)
    return [[o for o, (s, e) in enumerate(bs) if s <= i < e] for i in range(n_in)]


POOL_B = 2
POOL_C = (1, 3, 4)
AFFINES = ("scale_shift", "scale", "none")
_POOL_KEYS = ("src", "crop", "dst")
POOL_CASES = [dict(zip(_POOL_KEYS, row)) for row in [
    ((8, 12), None, (8, 12)),                  # identity: exact in both kinds
    ((16, 24), None, (4, 6)),                  # integer ratio: 4 x 4 bins, dyadic exact
    ((13, 10), None, (5, 7)),                  # overlapping bins
    ((64, 66), (9, 8, 47, 47), (28, 28)),      # the 188 -> 112 ratio in miniature
    ((40, 42), (3, 5, 31, 29), (17, 18)),      # crop with non-integer bins
    ((20, 22), (7, 9, 13, 13), (5, 4)),        # crop flush with the far corner of the image
    ((6, 6), None, (12, 12)),                  # x2 up-sampling
    ((5, 7), None, (8, 11)),                   # ratio 1.6
    ((3, 5), None, (9, 10)),                   # x3 and x2 mixed
    ((4, 4), None, (16, 16)),                  # x4 up-sampling
    ((1, 1), None, (3, 5)),                    # the smallest pair at which the gradient dropped bins
]]


def pool_crop(c):
    return c["crop"] if c["crop"] is not None else (0, 0) + c["src"]


def pool_geom(c):
    """bin areas [Ho, Wo] and the number of bins over every crop pixel [Hc, Wc], both int64"""
    _, _, hc, wc = pool_crop(c)
    ho, wo = c["dst"]
    ay = torch.tensor([e - s for s, e in bins(hc, ho)])
    ax = torch.tensor([e - s for s, e in bins(wc, wo)])
    my = torch.tensor([len(v) for v in bins_over(hc, ho)])
    mx = torch.tensor([len(v) for v in bins_over(wc, wo)])
    return ay[:, None] * ax[None, :], my[:, None] * mx[None, :]


def pool_exact(c, kind, affine, bwd=False):
    area, m = pool_geom(c)
    pow2 = all(is_pow2(int(a)) for a in area.flatten())
    if kind == "dyadic" and pow2:
        return True
    if bwd:
        return affine == "none" and pow2 and int(m.max()) == 1
    return affine == "none" and int(area.max()) == 1


def _affine(t, affine):
    return (t["scale"] if affine != "none" else None), (t["shift"] if affine == "scale_shift" else None)


def pool_ref(x, c, scale=None, shift=None):
    """F.adaptive_avg_pool2d of the crop of NCHW fp32 x, then the affine, in fp64, as NHWC; (y, bound)."""
    y0, x0, hc, wc = pool_crop(c)
    xc = x.double()[:, :, y0:y0 + hc, x0:x0 + wc]
    m, A = F.adaptive_avg_pool2d(xc, c["dst"]), F.adaptive_avg_pool2d(xc.abs(), c["dst"])
    area = pool_geom(c)[0].double()
    if scale is None:
        return _nhwc(m), _nhwc(U * (area + 2) * A)
    s = scale.double().view(1, -1, 1, 1)
    y = m * s if shift is None else m * s + shift.double().view(1, -1, 1, 1)
    return _nhwc(y), _nhwc(U * ((area + 4) * A * s.abs() + y.abs()))


def pool_bwd_ref(dy, c, scale=None):
    """fp64 autograd of pool_ref's forward w.r.t. the NCHW image for the NHWC fp32 upstream gradient dy; (dx, bound, inside), NCHW."""
    B, C = dy.shape[0], dy.shape[3]
    H, W = c["src"]
    y0, x0, hc, wc = pool_crop(c)

    def grad(g, s):
        xg = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
        y = F.adaptive_avg_pool2d(xg[:, :, y0:y0 + hc, x0:x0 + wc], c["dst"])
        if s is not None:
            y = y * s.view(1, -1, 1, 1)
        return torch.autograd.grad((y * _nchw(g)).sum(), xg)[0]

    sd = None if scale is None else scale.double()
    dx = grad(dy.double(), sd)
    T = grad(dy.double().abs(), None if sd is None else sd.abs())
    m = torch.zeros(H, W, dtype=torch.float64)
    m[y0:y0 + hc, x0:x0 + wc] = pool_geom(c)[1].double()
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[y0:y0 + hc, x0:x0 + wc] = True
    return dx, U * (m + 3) * T, inside


@functools.lru_cache(maxsize=None)
def pool_case(index, kind, C):
    """operands of POOL_CASES[index] with C channels (x and acc NCHW, dy NHWC) and the references of the three affine forms; read-only."""
    c = POOL_CASES[index]
    g = _gen("pool", f"{index}-C{C}", kind)
    (H, W), (ho, wo) = c["src"], c["dst"]
    x, dy, acc = operand((POOL_B, C, H, W), kind, g), operand((POOL_B, ho, wo, C), kind, g), operand((POOL_B, C, H, W), kind, g)
    if kind == "dyadic":
        scale = torch.tensor([-1.5, 0.5, 2.0, 1.0])[torch.randint(0, 4, (C,), generator=g)]
        shift = operand((C,), kind, g)
    else:
        scale, shift = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
        scale[0] = -scale[0]
    t = dict(case=c, x=x, dy=dy, acc=acc, scale=scale, shift=shift, fwd={}, bwd={})
    for a in AFFINES:
        t["fwd"][a] = pool_ref(x, c, *_affine(t, a))
        if a != "scale_shift":          # the gradient does not see the shift
            t["bwd"][a] = pool_bwd_ref(dy, c, _affine(t, a)[0])
    t["bwd"]["scale_shift"] = t["bwd"]["scale"]
    return t


# ---- stem convs ------------------------------------------------------------------------------------------------------------------------------
_CONV_KEYS = ("B", "Hi", "Wi", "Cin", "Cout", "k", "stride", "pad")
CONV_CASES = [dict(zip(_CONV_KEYS, row)) for row in [
    (1, 5, 7, 1, 16, 1, 1, 0),                 # smallest shape
    (2, 9, 11, 3, 64, 3, 1, 1),                # plain 3 x 3 stem
    (1, 16, 19, 3, 64, 11, 4, 2),              # 92.9 KB of weights in LDS: the opt-in path above 64 KB; the GEMM + col2im gradient
    (2, 12, 9, 4, 80, 5, 2, 1),                # 5 channel groups on 4 waves: wave 0 loops twice
    (1, 33, 36, 3, 16, 5, 2, 1),               # one group, three idle waves, 272 = 4 x 64 + 16 output pixels
    (1, 8, 8, 2, 32, 3, 4, 0),                 # stride > k: image pixels no output sees
    (1, 6, 6, 3, 16, 3, 1, 3),                 # pad = k: border outputs wholly in the padding
]]
# the gradient alone, with a hand-made dy: Cout = 20 is no multiple of 16 (no forward), only the per-pixel kernel takes it
CONV_BWD_ONLY = [dict(zip(_CONV_KEYS, (2, 7, 9, 3, 20, 3, 2, 1)))]
CONV_WAVES = 4
LDS_OPT_IN = 64 * 1024
LDS_LIMIT = 160 * 1024 - 512


def conv_out(c):
    return (c["Hi"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1, (c["Wi"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1


def conv_lds_bytes(c):
    return c["k"] * c["k"] * c["Cin"] * c["Cout"] * 4


def conv_gemm_route(c):
    """K.conv_smallcin_bwd takes the GEMM + col2im form (k k Cin >= 128 columns, Cout a multiple of 32), else the per-pixel kernel"""
    return c["k"] * c["k"] * c["Cin"] >= 128 and c["Cout"] % 32 == 0


def conv_npos(c):
    return (-(-c["k"] // c["stride"])) ** 2


def conv_ref(x, w, bias, c, relu):
    """F.conv2d of NHWC fp32 x with w [Cout, Cin, k, k] in fp64, as NHWC; (y, bound, pad_only): pad_only marks the outputs whose window
    holds no image pixel."""
    xd, wd = _nchw(x.double()), w.double()
    bd = None if bias is None else bias.double()
    y = F.conv2d(xd, wd, bd, stride=c["stride"], padding=c["pad"])
    mag = F.conv2d(xd.abs(), wd.abs(), None if bd is None else bd.abs(), stride=c["stride"], padding=c["pad"])
    seen = F.conv2d(torch.ones_like(xd[:, :1]), torch.ones_like(wd[:1, :1]), stride=c["stride"], padding=c["pad"])
    if relu:
        y = torch.relu(y)
    n = c["k"] * c["k"] * c["Cin"]
    return _nhwc(y), _nhwc((n + 2) * U * mag), _nhwc((seen == 0).expand_as(y))


def conv_bwd_ref(dy, w, c):
    """fp64 autograd of F.conv2d w.r.t. the image for the NHWC fp32 upstream gradient dy, as NHWC; (dx, bound)."""
    def grad(g, wt):
        xg = torch.zeros(c["B"], c["Cin"], c["Hi"], c["Wi"], dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xg, wt, stride=c["stride"], padding=c["pad"])
        return _nhwc(torch.autograd.grad((y * _nchw(g)).sum(), xg)[0])

    N = conv_npos(c) * c["Cout"]
    return grad(dy.double(), w.double()), (N + 1) * U * grad(dy.double().abs(), w.double().abs())


def conv_z(dy, w, c, zc):
    """the GEMM image of the gradient, z[b, oy, ox, (ky k + kx) Cin + ci] = dy[b, oy, ox, :] . w[:, ci, ky, kx], rounded to fp32, in rows
    of zc >= k k Cin columns whose tail is NaN (col2im may not read it)"""
    ncol = c["k"] * c["k"] * c["Cin"]
    wp = w.double().permute(2, 3, 1, 0).reshape(ncol, c["Cout"])
    z = torch.full(dy.shape[:3] + (zc,), float("nan"))
    z[..., :ncol] = (dy.double() @ wp.t()).float()
    return z


def col2im_ref(z, c):
    """F.fold of the fp32 z given, in fp64, as NHWC; (dx, bound)."""
    B, Ho, Wo, _ = z.shape
    k, cin = c["k"], c["Cin"]
    cols = z[..., :k * k * cin].double().reshape(B, Ho * Wo, k, k, cin).permute(0, 4, 2, 3, 1).reshape(B, cin * k * k, Ho * Wo)
    fold = lambda t: _nhwc(F.fold(t, (c["Hi"], c["Wi"]), k, stride=c["stride"], padding=c["pad"]))          # noqa: E731
    return fold(cols), (conv_npos(c) + 1) * U * fold(cols.abs())


@functools.lru_cache(maxsize=None)
def conv_case(index, kind, bwd_only=False):
    c = (CONV_BWD_ONLY if bwd_only else CONV_CASES)[index]
    g = _gen("conv", f"{index}-{int(bwd_only)}", kind)
    ho, wo = conv_out(c)
    x = operand((c["B"], c["Hi"], c["Wi"], c["Cin"]), kind, g)
    w = operand((c["Cout"], c["Cin"], c["k"], c["k"]), kind, g)
    bias, dy = operand((c["Cout"],), kind, g), operand((c["B"], ho, wo, c["Cout"]), kind, g)
    if kind == "random":
        w = w * 0.3
    t = dict(case=c, x=x, w=w, bias=bias, dy=dy, exact=kind == "dyadic", fwd={}, bwd=conv_bwd_ref(dy, w, c))
    if not bwd_only:
        for has_bias in (False, True):
            for relu in (False, True):
                t["fwd"][(has_bias, relu)] = conv_ref(x, w, bias if has_bias else None, c, relu)
    zc = (c["k"] * c["k"] * c["Cin"] + 31) // 32 * 32
    t["z"] = conv_z(dy, w, c, zc)
    t["col2im"] = col2im_ref(t["z"], c)
    return t


# ---- max pools -----------------------------------------------------------------------------------------------------------------------------
MP_KINDS = ("relu", "equal", "negative", "dyadic")
MP3_CASES = [dict(zip(("B", "H", "W", "C"), row)) for row in [(1, 3, 3, 4), (2, 8, 9, 4), (2, 7, 6, 12), (1, 15, 15, 64)]]
MP2_CASES = [dict(zip(("B", "H", "W", "C"), row)) for row in [(1, 2, 2, 4), (2, 5, 7, 8), (1, 8, 6, 64)]]
MP_GEOM = {"maxpool3s2": (3, 2), "maxpool2": (2, 2)}
MP_CASES = {"maxpool3s2": MP3_CASES, "maxpool2": MP2_CASES}


def maxpool_ref(x, name):
    """F.max_pool2d(return_indices=True) of NHWC fp32 x in fp64, as NHWC: values, and ATen's first maximum as the window-local code
    (row in the window) k + (column in the window)."""
    k, s = MP_GEOM[name]
    W = x.shape[2]
    y, idx = F.max_pool2d(_nchw(x.double()), k, s, return_indices=True)
    oy = torch.arange(y.shape[2]).view(1, 1, -1, 1)
    ox = torch.arange(y.shape[3]).view(1, 1, 1, -1)
    code = (idx // W - s * oy) * k + (idx % W - s * ox)
    return _nhwc(y), _nhwc(code).to(torch.uint8)


def maxpool_bwd_ref(x, dy, name):
    """fp64 autograd of F.max_pool2d w.r.t. NHWC x; (dx, bound) as NHWC"""
    k, s = MP_GEOM[name]

    def grad(g):
        xg = _nchw(x.double()).clone().requires_grad_(True)
        return _nhwc(torch.autograd.grad((F.max_pool2d(xg, k, s) * _nchw(g)).sum(), xg)[0])

    return grad(dy.double()), 5 * U * grad(dy.double().abs())


@functools.lru_cache(maxsize=None)
def maxpool_case(name, index, kind):
    c = MP_CASES[name][index]
    g = _gen(name, index, kind)
    sh = (c["B"], c["H"], c["W"], c["C"])
    k, s = MP_GEOM[name]
    if kind == "relu":
        x = torch.relu(torch.randn(sh, generator=g))                 # exact ties at 0, like a ReLU output
    elif kind == "equal":
        x = torch.full(sh, 0.3)
    elif kind == "negative":
        x = -torch.rand(sh, generator=g) - 0.1
    else:
        x = operand(sh, "dyadic", g)
    ho, wo = (c["H"] - k) // s + 1, (c["W"] - k) // s + 1
    dy = operand((c["B"], ho, wo, c["C"]), "dyadic" if kind == "dyadic" else "random", g)
    y, code = maxpool_ref(x, name)
    dx, bound = maxpool_bwd_ref(x, dy, name)
    return dict(case=c, x=x, dy=dy, y=y, code=code, dx=dx, bound=bound, exact_bwd=kind == "dyadic" or name == "maxpool2")


# ---- relu_bwd --------------------------------------------------------------------------------------------------------------------------------
RELU_CASES = [4, 4 * 257]


@functools.lru_cache(maxsize=None)
def relu_case(index, kind):
    n = RELU_CASES[index]
    g = _gen("relu", index, kind)
    y, dy, acc = torch.relu(operand((n,), kind, g)), operand((n,), kind, g), operand((n,), kind, g)
    y[1], y[2] = 0.0, -0.0
    if n > 4:
        y[5::7] = -0.0
        y[6::11] = -1.5                      # not a ReLU output: the gradient is 0 there all the same
    ref = torch.where(y > 0, dy, torch.zeros_like(dy))
    return dict(n=n, y=y, dy=dy, acc=acc, ref=ref, ref_acc=acc + ref)


# ---- LPIPS distance layer ------------------------------------------------------------------------------------------------------------------
LPIPS_CASES = [dict(zip(("B", "h", "w", "C"), row)) for row in
               [(2, 1, 1, 4), (1, 3, 5, 64), (2, 1, 17, 68), (1, 4, 4, 192), (1, 3, 11, 256), (2, 5, 5, 512)]]
LPIPS_GOUT, LPIPS_GMUL = 0.7, 1.25


def lpips_special(hw):
    """the pixels planted in every sample of a case with H W >= 3: (fx all zero, fy all zero, both all zero)"""
    return (0, hw // 2, hw - 1) if hw >= 3 else None


def _lp_parts(fx, fy, w):
    B, H, W, C = fx.shape
    x, y, wd = fx.double().reshape(B, H * W, C), fy.double().reshape(B, H * W, C), w.double().view(1, 1, C)
    rx, ry = x.pow(2).sum(-1, keepdim=True).sqrt(), y.pow(2).sum(-1, keepdim=True).sqrt()
    ix, iy = 1 / (rx + LP_EPS), 1 / (ry + LP_EPS)
    nx, ny = x * ix, y * iy
    t = nx - ny
    rho = ((C + 1) / 2 + 3) * U
    dt = (rho + U) * (nx.abs() + ny.abs()) + U * t.abs()
    return x, wd, rx, ix, t, rho, dt


def lpips_ref(fx, fy, w):
    """out[b] = mean over the pixels of sum_c w_c (fx_c / (|fx| + eps) - fy_c / (|fy| + eps))^2 in fp64; (out, bound)"""
    B, H, W, C = fx.shape
    _, wd, _, _, t, _, dt = _lp_parts(fx, fy, w)
    mag = (wd.abs() * t * t).sum(-1)
    out = (wd * t * t).sum(-1).mean(1)
    pix = (wd.abs() * (2 * t.abs() * dt + 2 * U * t * t)).sum(-1) + (C + 1) * U * mag
    return out, SECOND * pix.mean(1) + 2 * U * out.abs() + (H * W + 2) * 2.0 ** -53 * mag.mean(1)


def lpips_bwd_ref(fx, fy, w, gout, gmul):
    """d(gout gmul sum_b out[b]) / d(fx) by the closed form of the kernel's header comment in fp64; (dfx, bound).  gout, gmul: fp32 numbers."""
    B, H, W, C = fx.shape
    x, wd, rx, ix, t, rho, dt = _lp_parts(fx, fy, w)
    g = f32(gout) * f32(gmul) / (H * W)
    dn = 2 * wd * t * g
    ddn = (2 * wd * g).abs() * dt + 5 * U * dn.abs()
    dot = (dn * x).sum(-1, keepdim=True)
    ddot = (C + 1) * U * (dn * x).abs().sum(-1, keepdim=True) + (ddn * x.abs()).sum(-1, keepdim=True)
    live = rx > 0
    q = torch.where(live, ix * ix / rx.clamp(min=1e-300), torch.zeros_like(rx))
    k2, dk2 = dot * q, (ddot + dot.abs() * (3 * rho + 3 * U)) * q
    v = dn * ix - x * k2
    dv = ddn * ix + dn.abs() * ix * (rho + U) + x.abs() * dk2 + U * (x * k2).abs() + U * v.abs()
    return v.reshape(B, H, W, C), (SECOND * dv).reshape(B, H, W, C)


def lpips_autograd(fx, fy, w, gout, gmul):
    """the same derivative by fp64 autograd of the written formula (NaN at a pixel whose fx is all zero)"""
    xg = fx.double().clone().requires_grad_(True)
    nrm = lambda t: t / (t.pow(2).sum(-1, keepdim=True).sqrt() + LP_EPS)          # noqa: E731
    d = ((nrm(xg) - nrm(fy.double())).pow(2) * w.double()).sum(-1).mean((1, 2))
    return torch.autograd.grad(d.sum() * (f32(gout) * f32(gmul)), xg)[0]


@functools.lru_cache(maxsize=None)
def lpips_case(index, kind):
    c = LPIPS_CASES[index]
    g = _gen("lpips", index, kind)
    sh = (c["B"], c["h"], c["w"], c["C"])
    fx, fy, acc = operand(sh, kind, g), operand(sh, kind, g), operand(sh, kind, g)
    fx[..., 0] = 0.75                        # no pixel is zero by chance (dyadic data at C = 4)
    fy[..., 1] = -0.5
    w = operand((c["C"],), kind, g).abs()
    w[::3] = 0.0
    sp = lpips_special(c["h"] * c["w"])
    if sp is not None:
        fxf, fyf = fx.view(c["B"], -1, c["C"]), fy.view(c["B"], -1, c["C"])
        fxf[:, sp[0]] = 0.0
        fyf[:, sp[1]] = 0.0
        fxf[:, sp[2]] = 0.0
        fyf[:, sp[2]] = 0.0
    return dict(case=c, fx=fx, fy=fy, w=w, acc=acc, special=sp, fwd=lpips_ref(fx, fy, w),
                bwd=lpips_bwd_ref(fx, fy, w, LPIPS_GOUT, LPIPS_GMUL))


# ---- cosine terms ----------------------------------------------------------------------------------------------------------------------------
COS_CASES = [dict(B=B, D=D, special=s) for B, D, s in
             [(1, 1, None), (3, 255, None), (2, 4096, "orthogonal"), (2, 4097, None), (3, 10000, "opposite"), (1, 1048900, None)]]
COS_GOUT, COS_GMUL = 1.3, -0.5


def cos_chunk(D):
    """elements per block of cosine_partial_kernel: 4096, grown so that a row never needs more than 256 partial slots"""
    c = (D + 255) // 256
    c = (c + 255) // 256 * 256
    return max(c, 4096)


def cos_nchunk(D):
    return -(-D // cos_chunk(D))


def cosine_ref(a, b):
    """{cos, alpha, beta} per row from fp64 sums: cos = <a, b> / (|a| |b|), d(cos) / da = alpha b + beta a; (vals [B, 3], bounds [B, 3])"""
    ad, bd = a.double(), b.double()
    D = a.shape[1]
    ab, mag = (ad * bd).sum(1), (ad * bd).abs().sum(1)
    na, nb = ad.pow(2).sum(1).sqrt(), bd.pow(2).sum(1).sqrt()
    cos, alpha, beta = ab / (na * nb), 1 / (na * nb), -ab / (na ** 3 * nb)
    eD = (D + 8) * 2.0 ** -53
    bounds = [U * cos.abs() + eD * (mag / (na * nb) + 2 * cos.abs()), (U + 2 * eD) * alpha, U * beta.abs() + eD * (mag / (na ** 3 * nb) + 4 * beta.abs())]
    return torch.stack([cos, alpha, beta], 1), torch.stack(bounds, 1)


def cosine_autograd(a, b):
    ag = a.double().clone().requires_grad_(True)
    return torch.autograd.grad(F.cosine_similarity(ag, b.double(), dim=1, eps=0.0).sum() * (f32(COS_GOUT) * f32(COS_GMUL)), ag)[0]


def cosine_bwd_ref(a, b, coef, gout, gmul):
    """da = gout gmul (alpha b + beta a) in fp64 with the fp32 coefficients given; (da, bound)"""
    g = f32(gout) * f32(gmul)
    p1, p2 = coef[:, 1:2].double() * b.double(), coef[:, 2:3].double() * a.double()
    da = g * (p1 + p2)
    return da, U * (2 * abs(g) * (p1.abs() + p2.abs()) + 3 * da.abs())


@functools.lru_cache(maxsize=None)
def cosine_case(index, kind):
    c = COS_CASES[index]
    g = _gen("cosine", index, kind)
    a, acc = operand((c["B"], c["D"]), kind, g), operand((c["B"], c["D"]), kind, g)
    a[:, 0] = 0.75                           # no row is zero by chance
    if c["special"] == "orthogonal":         # a = (p, q), b = (q, -p): <a, b> = 0 in exact arithmetic
        h = c["D"] // 2
        b = torch.cat([a[:, h:], -a[:, :h]], 1)
    elif c["special"] == "opposite":
        b = -a
    else:
        b = operand((c["B"], c["D"]), kind, g)
        b[:, 0] = -0.5
    vals, bounds = cosine_ref(a, b)
    return dict(case=c, a=a, b=b, acc=acc, vals=vals, bounds=bounds)


# ---- frozen-statistics normalisation backward ------------------------------------------------------------------------------------------------
NORM_CASES = [dict(zip(("B", "HW", "C"), row)) for row in [(1, 1, 4), (3, 7, 12), (2, 30, 64)]]
NORM_OPTIONS = [(gate, extra) for gate in (False, True) for extra in (False, True)]


def norm_ref(dy, stats, gate, extra):
    """dx = rstd (gate dy + extra), rstd = stats[..., 1], per (b, c), in fp64; (dx, bound)"""
    r = stats[..., 1].double()[:, None, None]
    p = dy.double() if gate is None else gate.double()[:, None, None] * dy.double()
    inner = p if extra is None else p + extra.double()[:, None, None]
    dx = r * inner
    return dx, U * (r.abs() * (p.abs() + inner.abs()) + 2 * dx.abs())


@functools.lru_cache(maxsize=None)
def norm_case(index, kind):
    c = NORM_CASES[index]
    g = _gen("norm", index, kind)
    B, HW, C = c["B"], c["HW"], c["C"]
    dy, acc = operand((B, 1, HW, C), kind, g), operand((B, 1, HW, C), kind, g)
    if kind == "dyadic":
        rstd = 2.0 ** torch.randint(-1, 3, (B, C), generator=g).float()
        gate = 2.0 ** torch.randint(-1, 2, (B, C), generator=g).float()
        extra = operand((B, C), kind, g)
    else:
        rstd, gate, extra = torch.rand(B, C, generator=g) + 0.5, torch.rand(B, C, generator=g), torch.randn(B, C, generator=g)
    stats = torch.stack([torch.randn(B, C, generator=g), rstd], -1).contiguous()          # the kernel has no use for the mean
    t = dict(case=c, dy=dy, acc=acc, stats=stats, gate=gate, extra=extra, exact=kind == "dyadic", ref={})
    for og, oe in NORM_OPTIONS:
        t["ref"][(og, oe)] = norm_ref(dy, stats, gate if og else None, extra if oe else None)
    return t


def case_id(c):
    return gc.case_id({k: (f"{v[0]}x{v[1]}" if isinstance(v, tuple) and len(v) == 2 else "x".join(map(str, v)) if isinstance(v, tuple) else v)
                       for k, v in c.items()})
