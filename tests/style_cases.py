"""Seeded cases and fp64 yardsticks for the StyleLoss kernels (csrc/gram.hip: style_prep and its adjoint, gram, gram_mse, gram_grad): the
yardsticks of tests/test_style_cases_host.py and tests/test_gpu_style_kernels.py.  CPU only; the native library is not imported here.

Every reference takes the fp32 operands cast to double and is a plain statement of the operation: F.interpolate(mode="bilinear") of the
image and of the mask, the written normalisation and the product (style_loss.py:143-170); torch.mm on the [N C, H W] view divided by
N H W C (style_loss.py:213-221); F.mse_loss; fp64 autograd of those for the two gradients.  None restates a kernel's loop.  The pieces of
launch geometry restated here are the pixel-slice plan of the Gram kernel (gram_slices) and the block count of the MSE (mse_blocks): the
bounds count roundings with them, and the GPU test checks both against the library's workspace queries.

Two kinds of operand data (gen_bwd_cases.operand): random (fp32 normal values) and dyadic (integers in [-4, 4] times 2^-2).  With dyadic
data every product and every partial sum in any order is an fp32 number wherever no quotient by a non-power of two is involved, and the
output EQUALS the reference; `*_exact` says per case where, and the host test proves it by evaluating the same formula in fp32.

Bounds for random data, u = 2^-24, gamma_n = n u / (1 - n u), from the kernels' operation chains (an FMA only removes roundings):
  gram     a wave adds the products of ONE slice of `chunk` pixels into its accumulator through the fp32 MFMA, two products per
           instruction: every product enters the sum through at most one rounding of its own and one per later addition, a chain of at
           most chunk additions.  The S slices are then added in slice order in fp64 (nothing at this scale), cast once, and divided by
           N HW C once:
             gamma_{chunk + 3} sum_p |a||b| / (N HW C)                                      c = 3 - (K - chunk) in gamma_{K + c}
           Dyadic data: the sum is exact (multiples of 2^-4 below 2^20); equality where N HW C is a power of two, else the one quotient,
           u |G|.  G == G^T bit for bit whatever the data (both entries are written from one sum).
  gram_mse d = gx - gy is one rounding, u |d| (none on dyadic data: equality).  term: a thread adds m = ceil(chunk / 256) squares in fp32,
           everything above is fp64, one cast: (m + 3) u term.  acc (+)= weight term: the product and the addition, 2 u (|acc| + |weight term|).
           Dyadic data with a power-of-two count: equality, and a second launch into the same accumulator adds exactly.
  grad     s = fl(coef gloss); a chain of NC fused multiply-adds through the MFMA, then the product with s:
             gamma_{NC + 3} |s| sum_j |a||d|                                                 equality on dyadic data with dyadic coef, gloss
           The accumulate form is one more addition: |got - (acc + plain)| <= u |acc + plain| + u |plain|.
  prep     the source coordinate is computed in fp32 as ATen's float path does: scale = fl(in / out), src = fl(fl(scale (d + 0.5)) - 0.5): three
           roundings, |dsrc| <= 3 u (src + 1).  A shift of the sampling position by dsrc moves the bilinear value by at most dsrc times the
           largest difference of neighbouring pixels along that axis (the interpolant is continuous and piecewise linear, also across a
           cell border).  Then lambda0 = fl(1 - lambda1) (1 u), four products, two sums, two products, one sum: 6 u A with A the bilinear
           value of |x|.  In all
             e_r = 6 u A + dsy Ly + dsx Lx
           normalise: fl(r + 1), the exact halving, the subtraction of the mean, the quotient by std:
             e_n = (e_r / 2 + u |r + 1| / 2 + u |t|) / std + u |n|,  t = (r + 1) / 2 - mean
           mask: e_m as e_r on the mask; the product: |m| e_n + |n| e_m + u |y|.  Without a mask and without normalisation: e_r alone.
           Power-of-two ratios both ways on dyadic data without normalisation: weights and values are dyadic, equality.
  prep_bwd dx = k sum over the outputs that read the pixel of wy wx m dy, k = fl(0.5 / std) or 1.  Per term: wy wx, the product with m, the
           product with dy (3 u, + 1 u for lambda0 on each axis), the mask's own error e_m, the coordinate error on each weight
           (|dw| <= dsrc); the sum of T terms (T u); k's rounding and the last product (2 u):
             k [ (T + 7) u W|dy| + dsy (Iy^T |m dy| Wx) + dsx (Wy^T |m dy| Ix) + W (e_m |dy|) ]
           with W the transposed map with the exact weights and Iy / Ix the 0-1 patterns of the 1-D weight matrices; T <= the number of
           outputs that read the pixel.  The 1-D matrices are F.interpolate applied to an identity, not a restated loop.

Largest observed error / bound on the MI355X (printed by the GPU test at teardown): gram 0.93, gram_grad 0.05, its accumulate form 1.00
(one rounding), gram_mse D 1.00 (one rounding), term 0.04, style_prep 0.09, style_prep_bwd 0.08, the adjoint identity below 0.001.
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from gen_bwd_cases import KINDS, operand  # noqa: F401

U = 2.0 ** -24
VGG_MEAN = torch.tensor(np.array([0.485, 0.456, 0.406]).astype(np.float32)).double()       # style_loss.py:11-12: fp32 constants
VGG_STD = torch.tensor(np.array([0.229, 0.224, 0.225]).astype(np.float32)).double()


def gamma(n):
    return n * U / (1 - n * U)


def f32(v):
    return float(np.float32(v))


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def _gen(name, cid, kind):
    return torch.Generator().manual_seed(zlib.crc32(f"style-{name}-{cid}-{kind}".encode()))


# ---- Gram matrix ----------------------------------------------------------------------------------------------------------------------
# (N, H, W, C): one partly filled tile; a pixel count that is no multiple of 8 plus cross-sample blocks; an ODD pixel count (the upper half
# of the last k-pair is empty); NC = 192, three tiles per side; 128 channels; many output tiles and few pixels; many pixel slices
GRAM_SHAPES = [(1, 4, 4, 64), (2, 6, 5, 64), (1, 3, 5, 64), (3, 8, 8, 64), (2, 16, 16, 128), (1, 32, 32, 512), (2, 64, 64, 64)]
GRAM_REFUSED = [(1, 4, 4, 96), (2, 4, 4, 32)]
GT = 64


def shape_id(s):
    return "x".join(str(v) for v in s)


def gram_slices(N, HW, C):
    """(tiles of the upper block triangle, pixel slices, pixels per slice) of e4s_gram_f32's launch."""
    T = N * C // GT
    ntile = T * (T + 1) // 2
    want = min(-(-1024 // ntile), max(HW // 32, 1))
    chunk = (-(-HW // want) + 1) & ~1
    return ntile, -(-HW // chunk), chunk


def gram_ws_floats(N, HW, C):
    ntile, nsplit, _ = gram_slices(N, HW, C)
    return ntile * nsplit * GT * GT


def _rows(f):
    """NHWC [N,H,W,C] -> the reference's [N C, H W] view of the NCHW tensor"""
    n, h, w, c = f.shape
    return f.permute(0, 3, 1, 2).reshape(n * c, h * w)


def gram_ref(f64):
    n, h, w, c = f64.shape
    x = _rows(f64)
    return torch.mm(x, x.t()) / (n * h * w * c)


def gram_exact(shape, kind):
    n, h, w, c = shape
    return kind == "dyadic" and is_pow2(n * h * w * c)


@functools.lru_cache(maxsize=None)
def gram_case(index, kind):
    shape = GRAM_SHAPES[index]
    n, h, w, c = shape
    g = _gen("gram", index, kind)
    f = operand(shape, kind, g)
    if kind == "random":
        f = f.abs()                                                    # taps are ReLU outputs
    ref = gram_ref(f.double())
    mag = gram_ref(f.double().abs())
    _, nsplit, chunk = gram_slices(n, h * w, c)
    bound = U * ref.abs() if kind == "dyadic" else gamma(chunk + 3) * mag
    # gram_grad operands: a symmetric D, a device scalar, a host coefficient, an addend
    nc = n * c
    d0 = operand((nc, nc), kind, g)
    d = (d0 + d0.t()) * (1.0 if kind == "dyadic" else 0.5)
    gloss = torch.tensor([0.5]) if kind == "dyadic" else torch.randn(1, generator=g)
    coef = 2.0 ** -10 if kind == "dyadic" else f32(1e-3)
    acc = operand(shape, kind, g)
    s = float(gloss.double()) * coef
    a = _rows(f.double())                                                  # [NC, HW]
    back = lambda m: m.reshape(n, c, h, w).permute(0, 2, 3, 1).contiguous()
    gref = back(torch.mm(d.double(), a)) * s
    gbound = back(torch.mm(d.double().abs(), a.abs())) * abs(s) * gamma(nc + 3)
    return dict(f=f, ref=ref, bound=bound, d=d, gloss=gloss, coef=coef, acc=acc, grad=gref, grad_bound=gbound)


def gram_grad_autograd(f, d, s):
    """the same gradient from fp64 autograd: L = s/2 <D, A^T A> with D symmetric has dL/dF = s A D"""
    x = f.double().clone().requires_grad_(True)
    r = _rows(x)
    (0.5 * s * (d.double() * torch.mm(r, r.t())).sum()).backward()
    return x.grad


# ---- MSE of two Gram matrices -------------------------------------------------------------------------------------------------------------
MSE_SIZES = [64, 192, 1024]                  # NC: one block, a count that is no power of two, the largest layer (256 blocks)


def mse_blocks(n):
    return min(max(-(-n // 4096), 1), 1024)


@functools.lru_cache(maxsize=None)
def mse_case(index, kind):
    nc = MSE_SIZES[index]
    g = _gen("mse", index, kind)
    gx, gy = operand((nc, nc), kind, g), operand((nc, nc), kind, g)
    d = gx.double() - gy.double()
    term = float((d * d).mean())
    n = nc * nc
    m = -(-(-(-n // mse_blocks(n))) // 256)
    weight = 0.25
    return dict(gx=gx, gy=gy, d=d, d_bound=U * d.abs(), term=term, term_bound=(m + 3) * U * term, weight=weight,
                exact=kind == "dyadic" and is_pow2(n))


# ---- prep ----------------------------------------------------------------------------------------------------------------------------------
# image (H, W) -> out (oh, ow), mask (Hm, Wm): up x2, down x2 (exact weights), non-integer scales both ways, not square; the masks have
# another size than the image
PREP_B = 2
PREP_CASES = [dict(src=(8, 8), dst=(16, 16), mask=(32, 32)), dict(src=(32, 32), dst=(16, 16), mask=(8, 8)),
              dict(src=(20, 12), dst=(16, 16), mask=(12, 20)), dict(src=(40, 28), dst=(16, 16), mask=(9, 21))]
PREP_MODES = [(n, m) for n in (False, True) for m in (False, True)]          # (normalize, mask)


def prep_id(c):
    return f"{c['src'][0]}x{c['src'][1]}-to-{c['dst'][0]}x{c['dst'][1]}"


def prep_exact(c, kind, normalize, mask):
    pw = lambda a, b: is_pow2(a // b) and a % b == 0 if a >= b else is_pow2(b // a) and b % a == 0
    ok = all(pw(c["src"][i], c["dst"][i]) for i in (0, 1)) and (not mask or all(pw(c["mask"][i], c["dst"][i]) for i in (0, 1)))
    return kind == "dyadic" and not normalize and ok


def prep_ref(x, mask, dst, normalize):
    """style_loss.py:143-170 in the dtype of x"""
    r = F.interpolate(x, size=dst, mode="bilinear")
    if normalize:
        r = ((r + 1) / 2 - VGG_MEAN.to(x.dtype).view(1, 3, 1, 1)) / VGG_STD.to(x.dtype).view(1, 3, 1, 1)
    if mask is not None:
        r = r * F.interpolate(mask, size=dst, mode="bilinear")
    return r


def _axis(n_in, n_out):
    """1-D bilinear matrix [n_out, n_in] (F.interpolate of an identity), its 0-1 pattern, and the fp32 coordinate error per output"""
    eye = torch.eye(n_in, dtype=torch.float64).view(1, n_in, n_in, 1)               # channel j = unit vector j along H
    wm = F.interpolate(eye, size=(n_out, 1), mode="bilinear")[0, :, :, 0].t().contiguous()
    src = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5).clamp(min=0)
    return wm, (wm > 0).double(), 3 * U * (src + 1)


def _interp_err(v, dst):
    """e_r of the module docstring for a map v [B,C,H,W] (fp64) resized to dst"""
    _, _, h, w = v.shape
    _, _, dsy = _axis(h, dst[0])
    _, _, dsx = _axis(w, dst[1])
    ly = (v[:, :, 1:] - v[:, :, :-1]).abs().amax((2, 3), keepdim=True) if h > 1 else torch.zeros_like(v[:, :, :1, :1])
    lx = (v[:, :, :, 1:] - v[:, :, :, :-1]).abs().amax((2, 3), keepdim=True) if w > 1 else torch.zeros_like(v[:, :, :1, :1])
    amp = F.interpolate(v.abs(), size=dst, mode="bilinear")
    return 6 * U * amp + dsy.view(1, 1, -1, 1) * ly + dsx.view(1, 1, 1, -1) * lx


def prep_fwd_bound(x, mask, dst, normalize):
    """(the elementwise bound of the module docstring on style_prep's output [B,3,oh,ow], e_m, the resized mask) for fp64 x, mask"""
    std = VGG_STD.view(1, 3, 1, 1)
    r = F.interpolate(x, size=dst, mode="bilinear")
    e = _interp_err(x, dst)
    n = r
    if normalize:
        t = (r + 1) / 2 - VGG_MEAN.view(1, 3, 1, 1)
        n = t / std
        e = (e / 2 + U * (r + 1).abs() / 2 + U * t.abs()) / std + U * n.abs()
    em = torch.zeros_like(r[:, :1])
    mres = torch.ones_like(r[:, :1])
    if mask is not None:
        mres = F.interpolate(mask, size=dst, mode="bilinear")
        em = _interp_err(mask, dst)
        e = mres.abs() * e + n.abs() * em + U * (n * mres).abs()
    return e, em, mres


@functools.lru_cache(maxsize=None)
def prep_case(index, kind):
    c = PREP_CASES[index]
    g = _gen("prep", index, kind)
    x = operand((PREP_B, 3) + c["src"], kind, g)
    # a 0-1 mask with a ragged blob: all-0 and all-1 areas and a border that the resize turns into fractions
    hm, wm = c["mask"]
    yy, xx = torch.meshgrid(torch.arange(hm), torch.arange(wm), indexing="ij")
    blob = ((yy - hm * 0.45) ** 2 / (hm * 0.3) ** 2 + (xx - wm * 0.55) ** 2 / (wm * 0.33) ** 2 < 1.0) ^ ((yy * 7 + xx * 3) % 11 == 0)
    mask = torch.stack([blob, blob.flip(1)]).float()[:, None].contiguous()
    dy = operand((PREP_B, 3) + c["dst"], kind, g)
    acc = {}
    std = VGG_STD.view(1, 3, 1, 1)
    wy, iy, dsy = _axis(c["src"][0], c["dst"][0])
    wx, ix, dsx = _axis(c["src"][1], c["dst"][1])
    for normalize, use_mask in PREP_MODES:
        xd = x.double().clone().requires_grad_(True)
        md = mask.double() if use_mask else None
        ref = prep_ref(xd, md, c["dst"], normalize)
        ref.backward(dy.double())
        with torch.no_grad():
            e, em, mres = prep_fwd_bound(x.double(), md, c["dst"], normalize)
            # adjoint bound
            k = (0.5 / std) if normalize else torch.ones_like(std)
            adj = lambda g_, a, b: torch.einsum("oy,bcop,px->bcyx", a, g_, b)
            T = (iy.sum(0).view(-1, 1) * ix.sum(0).view(1, -1)).view(1, 1, *c["src"])
            gm = (mres * dy.double()).abs()
            db = k * ((T + 7) * U * adj(gm, wy, wx) + adj(gm * dsy.view(1, 1, -1, 1), iy, wx) + adj(gm * dsx.view(1, 1, 1, -1), wy, ix)
                      + adj(em * dy.double().abs(), wy, wx))
        acc[(normalize, use_mask)] = dict(fwd=ref.detach(), fwd_bound=e, bwd=xd.grad.clone(), bwd_bound=db)
    return dict(x=x, mask=mask, dy=dy, modes=acc)


# ---- the three recorded StyleLoss cases (tests/golden/make_style_golden.py, tests/test_gpu_style.py) ---------------------------------------
# inputs are regenerated from the seed on both sides; VGG16's 30 MB of weights likewise (e4s_amd.synth.synth_vgg16_state_dict(seed=0))
GOLDEN_CASES = [
    dict(name="coach", B=2, size=(64, 64), mask=(32, 32), normalize=True, taps=[3, 8, 15, 22]),           # the call of coach.py:446-450
    dict(name="plain", B=1, size=(64, 64), mask=None, normalize=False, taps=[3, 8, 15, 22]),
    dict(name="rect", B=1, size=(96, 80), mask=None, normalize=True, taps=[8, 22]),
]


def golden_inputs(case):
    """(x, x_hat, mask or None): images in [-1, 1] (a smooth part plus pixel noise), a 0-1 mask with a ragged blob per sample"""
    g = _gen("golden", case["name"], "img")
    b, (h, w) = case["B"], case["size"]

    def image():
        low = F.interpolate(torch.randn(b, 3, 6, 5, generator=g), size=(h, w), mode="bicubic", align_corners=False)
        return (0.6 * low + 0.25 * torch.randn(b, 3, h, w, generator=g)).clamp(-1, 1).contiguous()
    x, x_hat = image(), image()
    mask = None
    if case["mask"] is not None:
        hm, wm = case["mask"]
        yy, xx = torch.meshgrid(torch.arange(hm), torch.arange(wm), indexing="ij")
        blobs = []
        for i in range(b):
            cy, cx = hm * (0.45 + 0.1 * i), wm * (0.55 - 0.1 * i)
            blob = ((yy - cy) ** 2 / (hm * 0.3) ** 2 + (xx - cx) ** 2 / (wm * 0.33) ** 2 < 1.0) ^ ((yy * 7 + xx * 3 + i) % 11 == 0)
            blobs.append(blob)
        mask = torch.stack(blobs).float()[:, None].contiguous()
    return x, x_hat, mask


def gram_sample_index(nc):
    """16 rows x 16 columns of a [nc, nc] Gram matrix, spread over all samples (so cross-sample blocks are among them)"""
    rows = torch.linspace(0, nc - 1, 16).round().long()
    cols = torch.linspace(0, nc - 1, 16).flip(0).add(-3).clamp(min=0).round().long()
    return rows, cols
