"""Seeded cases and fp64 yardsticks for the streaming kernels of the generator backward (csrc/bwd_misc.hip, csrc/dgrad_scatter.hip,
scale_dot of csrc/optim.hip): the yardsticks of tests/test_gen_bwd_cases_host.py and tests/test_gpu_gen_backward_kernels.py.  CPU only; the
native library is not imported here.

The region of a pixel is what F.interpolate(labels as fp32, size=(H, W), mode="nearest") gives on the CPU (how the model resizes its masks,
model.py:391), never a restatement of the kernels' nearest_src.  Every reference takes the fp32 operands cast to double; alpha, gain and the
noise weight are rounded to fp32 first, as the C ABI receives them.

Two kinds of operand data:
  random  fp32 normal values; alpha 0.2, gain sqrt(2), noise weight 0.3.
  dyadic  integers in [-4, 4] times 2^-2 with gain 1, alpha 0.5 and noise weight 0.5: every product and, as long as S_abs / quantum < 2^24
          (checked per case by the host test), every partial sum in any order is exactly representable in fp32, so a kernel's output has to
          EQUAL the fp64 reference.

S_abs of a summed output is the fp64 sum of the absolute values of its terms.  The demodulation term gz * (z - nw noise - bias) is itself a
sum: its absolute value is taken term by term, |gz| (|z| + |nw noise| + |bias|), because the roundings of z, of nw noise and of the two
subtractions are relative to those magnitudes and not to their (possibly cancelling) difference; with |gz (z - nw noise - bias)| the bound
(N + 4) 2^-24 S_abs would not be a bound for a region of one pixel.
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

PATTERNS = ("blocks", "noise", "absent", "one")
KINDS = ("dyadic", "random")
CONSTS = {"dyadic": dict(alpha=0.5, gain=1.0, noise_w=0.5), "random": dict(alpha=0.2, gain=2 ** 0.5, noise_w=0.3)}

# label-map sizes per pixel grid: larger with non-integer ratios, equal, smaller with non-integer ratios.  The doubled grids are the OUTPUT
# grids of the phase-major (ncls = 4) forms, whose regions are those of the output pixels.
MAPS = {
    (5, 7): {"larger": (12, 20), "equal": (5, 7), "smaller": (3, 4)},
    (16, 24): {"larger": (64, 64), "equal": (16, 24), "smaller": (6, 10)},
    (13, 37): {"larger": (32, 50), "equal": (13, 37), "smaller": (10, 9)},
    (33, 50): {"larger": (80, 64), "equal": (33, 50), "smaller": (12, 17)},
    (41, 51): {"larger": (64, 64), "equal": (41, 51), "smaller": (12, 17)},
    (10, 14): {"larger": (24, 40), "equal": (10, 14), "smaller": (3, 4)},
    (32, 48): {"larger": (64, 64), "equal": (32, 48), "smaller": (6, 10)},
    (26, 74): {"larger": (64, 100), "equal": (26, 74), "smaller": (10, 9)},
    (66, 100): {"larger": (80, 128), "equal": (66, 100), "smaller": (12, 17)},
}


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def absent_regions(R):
    """(region missing from sample 0, region missing from the last sample) of the "absent" pattern.  R - 1 is where the clamping kernels
    would file an out-of-range label, 0 is the region every thread of act_bwd_demod_kernel starts in."""
    return R - 1, 0


def make_labels(pattern, B, Hm, Wm, R, seed):
    """uint8 [B, Hm, Wm] with values < R."""
    rs = np.random.RandomState(seed)
    if pattern == "one":
        lab = np.full((B, Hm, Wm), R - 1, dtype=np.int64)
    elif pattern == "noise":
        lab = rs.randint(0, R, size=(B, Hm, Wm))
    elif pattern in ("blocks", "absent"):
        gy, gx = min(Hm, 4), min(Wm, 5)
        cells = rs.randint(0, R, size=(B, gy, gx))
        yy, xx = np.arange(Hm) * gy // Hm, np.arange(Wm) * gx // Wm
        lab = cells[:, yy[:, None], xx[None, :]].copy()
        if pattern == "absent":
            if R < 3:
                raise ValueError("the absent pattern needs R >= 3")
            first, last = absent_regions(R)
            lab[0][lab[0] == first] = (first + 1) % R
            lab[-1][lab[-1] == last] = (last + 1) % R
    else:
        raise ValueError(pattern)
    assert lab.min() >= 0 and lab.max() < R
    return torch.from_numpy(lab.astype(np.uint8))


def region_map(labels, H, W):
    """int64 [B, H, W]: the region of every pixel of an H x W grid."""
    return F.interpolate(labels[:, None].float(), size=(H, W), mode="nearest")[:, 0].long()


def operand(shape, kind, gen):
    if kind == "dyadic":
        return torch.randint(-4, 5, tuple(shape), generator=gen).float() * 0.25
    return torch.randn(tuple(shape), generator=gen)


def _f32c(v):
    return float(np.float32(v))


# ---- fp64 references -----------------------------------------------------------------------------------------------------------------
def region_sums(reg, R, terms):
    """reg int64 [B, P] (None: one group per sample), terms fp64 [B, P, ...] -> [B * R, ...]."""
    B = terms.shape[0]
    if reg is None:
        return terms.sum(1)
    onehot = F.one_hot(reg, R).double()                                 # [B, P, R]
    flat = terms.reshape(B, terms.shape[1], -1)
    return torch.einsum("bpr,bpk->brk", onehot, flat).reshape(B * R, *terms.shape[2:])


def region_counts(reg, R, B, P):
    if reg is None:
        return torch.full((B,), P, dtype=torch.int64)
    return F.one_hot(reg, R).sum(1).reshape(B * R)


def act_ref(dy, y, noise, noise_w, bias, alpha, gain, reg, R, gz=None):
    """gz = dy * (y > 0 ? gain : gain alpha);  dd[b, r, c] = sum_{p in r} gz (z - nw noise[b or 0, p] - bias[c]),  z = y / gain for y > 0,
    else y / (gain alpha).  `gz` given: the demodulation sums of that gz (demod_grad's contract).  reg int64 [B, H, W] or None."""
    B, H, W, C = y.shape
    alpha, gain = _f32c(alpha), _f32c(gain)
    y = y.double().reshape(B, H * W, C)
    slope = torch.where(y > 0, torch.full_like(y, gain), torch.full_like(y, gain * alpha))
    gz = dy.double().reshape(B, H * W, C) * slope if gz is None else gz.double().reshape(B, H * W, C)
    z = y / slope
    nz = torch.zeros(1, 1, 1, dtype=torch.float64)
    if noise is not None:
        nz = (_f32c(noise_w) * noise.double()).reshape(noise.shape[0], H * W, 1)
    bs = torch.zeros(1, 1, 1, dtype=torch.float64) if bias is None else bias.double().reshape(1, 1, C)
    flat = None if reg is None else reg.reshape(B, H * W)
    return dict(gz=gz.reshape(B, H, W, C), dd=region_sums(flat, R, gz * (z - nz - bs)),
                dd_abs=region_sums(flat, R, gz.abs() * (z.abs() + nz.abs() + bs.abs())), n=region_counts(flat, R, B, H * W))


def torgb_ref(drgb, x, ws, reg, R, dx_acc=None):
    """dws[b R + r, ch, ci] = sum_{p in r} drgb[b, ch, p] x[p, ci];  dx[p, ci] = (dx_acc +) sum_ch drgb[b, ch, p] ws[b R + r(p), ch, ci];
    unmasked (reg None, R = 1) the group is b."""
    B, H, W, C = x.shape
    P = H * W
    g, xd = drgb.double().reshape(B, 3, P).transpose(1, 2), x.double().reshape(B, P, C)          # g [B, P, 3]
    flat = None if reg is None else reg.reshape(B, P)
    outer = g[:, :, :, None] * xd[:, :, None, :]                                                   # [B, P, 3, C]
    wpix = ws.double().reshape(B, R, 3, C)[torch.arange(B)[:, None], torch.zeros(B, P, dtype=torch.int64) if flat is None else flat]
    terms = g[:, :, :, None] * wpix                                                                # [B, P, 3, C]
    dx, dx_abs = terms.sum(2), terms.abs().sum(2)
    if dx_acc is not None:
        dx, dx_abs = dx + dx_acc.double().reshape(B, P, C), dx_abs + dx_acc.double().abs().reshape(B, P, C)
    return dict(dws=region_sums(flat, R, outer), dws_abs=region_sums(flat, R, outer.abs()), n=region_counts(flat, R, B, P),
                dx=dx.reshape(B, H, W, C), dx_abs=dx_abs.reshape(B, H, W, C))


def scale_dot_ref(u, x, s):
    """ds[b, c] = sum_p x u;  u_out = u s[b]."""
    B, H, W, C = u.shape
    t = (u.double() * x.double()).reshape(B, H * W, C)
    return dict(ds=t.sum(1), ds_abs=t.abs().sum(1), u=u.double() * s.double().reshape(B, 1, 1, C))


def _pix(tab, reg, R):
    """tab [B * R, C], reg [B, Ho, Wo] -> the row of every pixel's region, [B, Ho, Wo, C]."""
    B = reg.shape[0]
    return tab.reshape(B, R, -1)[torch.arange(B)[:, None, None], reg]


def conv_fwd(x, spix, Wt, ncls):
    """The masked StyledConv before demodulation.  x [B, H, W, Ci]; spix [B, Ho, Wo, Ci] the style row of the region of every OUTPUT pixel;
    Wt [ncls, 9, Co, Ci].  ncls 1: c[m] = sum_t sum_ci x[m + t - 1] s[r(m)] W[t] with zero padding.  ncls 4 (Ho = 2H):
    y[2a + ph] = sum_e sum_ci x[a + e - 1] s[r(2a + ph)] Weff[ph][e]."""
    B, H, W, _ = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))

    def taps(sp, w9):
        return sum(torch.einsum("bhwc,oc->bhwo", xp[:, t // 3:t // 3 + H, t % 3:t % 3 + W] * sp, w9[t]) for t in range(9))

    if ncls == 1:
        return taps(spix, Wt[0])
    out = x.new_zeros(B, 2 * H, 2 * W, Wt.shape[2])
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        out[:, py::2, px::2] = taps(spix[:, py::2, px::2], Wt[ph])
    return out


def scatter_form(x, spix, G, ncls):
    """sum_ph sum_m sum_t sum_ci x[m + t - 1, ci] spix[m_ph, ci] G[ph, m, t, ci]: the loss as a bilinear form of the scatter products; its
    derivatives with absolute values in the other two slots are the S_abs of dx and ds."""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    os_ = 2 if ncls == 4 else 1
    G = G.reshape(ncls, B, H, W, 9, C)
    tot = 0
    for ph in range(ncls):
        sp = spix[:, (ph >> 1)::os_, (ph & 1)::os_] if ncls == 4 else spix
        for t in range(9):
            tot = tot + (xp[:, t // 3:t // 3 + H, t % 3:t % 3 + W] * sp * G[ph, :, :, :, t]).sum()
    return tot


def dgrad_ref(gz, d, x, s, Wt, reg, R, ncls):
    """(dL/dx, dL/ds) of L = sum gz d[r(m), co] c by fp64 autograd through conv_fwd, the scatter products G [ncls, B, H, W, 9 Ci]
    (G[ph, b, m, t Ci + ci] = sum_co (gz d[r])[m_ph, co] W[ph][t][co][ci]) in fp64, S_abs and the term counts of dx and ds.
    gz [B, Ho, Wo, Co]; d [B R, Co]; x [B, H, W, Ci]; s [B R, Ci]; reg int64 [B, Ho, Wo] the regions of the OUTPUT pixels."""
    B, H, W, C = x.shape
    gz, d, Wt = gz.double(), d.double(), Wt.double()
    xg, sg = x.double().requires_grad_(True), s.double().requires_grad_(True)
    u = gz * _pix(d, reg, R)
    L = (u * conv_fwd(xg, _pix(sg, reg, R), Wt, ncls)).sum()
    dx, ds = torch.autograd.grad(L, (xg, sg))
    os_ = 2 if ncls == 4 else 1
    G = torch.stack([torch.einsum("bhwo,toc->bhwtc", u[:, (ph >> 1)::os_, (ph & 1)::os_], Wt[ph]) for ph in range(ncls)])
    G = G.reshape(ncls, B, H, W, 9 * C)
    xa = x.double().abs().requires_grad_(True)
    ones = torch.ones(B * R, C, dtype=torch.float64, requires_grad=True)
    dx_abs, = torch.autograd.grad(scatter_form(xa, _pix(s.double().abs(), reg, R), G.abs(), ncls), xa)
    ds_abs, = torch.autograd.grad(scatter_form(x.double().abs(), _pix(ones, reg, R), G.abs(), ncls), ones)
    n_ds = 9 * F.one_hot(reg.reshape(B, -1), R).sum(1).reshape(B * R)          # taps that fall outside the image are zero terms
    return dict(dx=dx, ds=ds, G=G, dx_abs=dx_abs, ds_abs=ds_abs, n_dx=9 * ncls, n_ds=n_ds, u=u)


def phase_major(u):
    """[B, 2H, 2W, C] -> [4, B, H, W, C]: output pixel (oy, ox) of phase ph = (oy & 1) 2 + (ox & 1) lands at [ph, b, oy >> 1, ox >> 1]."""
    return torch.stack([u[:, (ph >> 1)::2, (ph & 1)::2] for ph in range(4)])


# ---- case lists ----------------------------------------------------------------------------------------------------------------------
# Every row is met with every label pattern.  Between them the rows hold every C of the kernel's set, the four grids (5x7: fewer pixels
# than lanes; 13x37 and 33x50: several splits whose length is no multiple of the lane count), the three map sizes, R in {1, 5, 12, 16} and
# B in {1, 3}.  The "absent" pattern needs R >= 3: it runs the R = 1 rows with R = 3.
def _cross(rows, keys):
    out = []
    for pattern in PATTERNS:
        for row in rows:
            c = dict(zip(keys, row), pattern=pattern)
            if pattern == "absent" and c["R"] < 3:
                c["R"] = 3
            out.append(c)
    return out


_ACT_KEYS = ("C", "grid", "rel", "R", "B", "noise", "bias")
# noise: "per" [B, 1, H, W], "shared" [1, 1, H, W], None
_ACT_ROWS = [
    (8, (5, 7), "larger", 5, 1, "per", True),
    (8, (33, 50), "smaller", 12, 3, "shared", False),
    (8, (16, 24), "equal", 16, 3, None, True),
    (32, (13, 37), "equal", 16, 3, None, True),
    (32, (33, 50), "larger", 5, 1, "per", True),
    (32, (16, 24), "smaller", 1, 1, "shared", False),
    (64, (16, 24), "larger", 12, 3, "shared", True),
    (64, (13, 37), "smaller", 16, 1, "per", False),
    (64, (33, 50), "equal", 5, 3, None, False),
    (1024, (5, 7), "smaller", 16, 3, "per", True),
    (1024, (5, 7), "equal", 1, 1, "shared", True),
]
# act_bwd_demod's channel set is {C : C % 4 == 0, 256 % (C / 4) == 0}
ACT_CASES = _cross(_ACT_ROWS, _ACT_KEYS) + [
    dict(C=64, grid=(13, 37), rel=None, R=1, B=3, noise="per", bias=True, pattern=None),
    dict(C=8, grid=(33, 50), rel=None, R=1, B=1, noise=None, bias=False, pattern=None),
    dict(C=32, grid=(5, 7), rel=None, R=1, B=3, noise="shared", bias=True, pattern=None),
]
# demod_grad's is C % 32 == 0 (C > 64: C % 64 == 0): 192 = three slabs, 32 = the cw < 64 path
_DEMOD_ROWS = [(192 if row[0] == 8 else row[0],) + row[1:] for row in _ACT_ROWS]
DEMOD_CASES = _cross(_DEMOD_ROWS, _ACT_KEYS) + [
    dict(C=64, grid=(13, 37), rel=None, R=1, B=3, noise="per", bias=True, pattern=None),
    dict(C=192, grid=(33, 50), rel=None, R=1, B=1, noise=None, bias=False, pattern=None),
    dict(C=32, grid=(5, 7), rel=None, R=1, B=3, noise="shared", bias=True, pattern=None),
]

_TORGB_KEYS = ("C", "grid", "rel", "R", "B", "acc")
_TORGB_ROWS = [
    (32, (5, 7), "larger", 5, 1, True),
    (32, (33, 50), "smaller", 12, 3, False),
    (32, (13, 37), "equal", 16, 3, True),
    (64, (16, 24), "larger", 12, 3, False),
    (64, (13, 37), "smaller", 16, 1, True),
    (64, (33, 50), "equal", 1, 3, True),
    (192, (16, 24), "equal", 16, 1, False),
    (192, (33, 50), "larger", 5, 3, True),
    (192, (13, 37), "smaller", 12, 1, False),
    (1024, (5, 7), "smaller", 16, 3, True),
    (1024, (5, 7), "equal", 1, 1, False),
]
TORGB_CASES = _cross(_TORGB_ROWS, _TORGB_KEYS) + [
    dict(C=64, grid=(13, 37), rel=None, R=1, B=3, acc=True, pattern=None),
    dict(C=192, grid=(33, 50), rel=None, R=1, B=1, acc=False, pattern=None),
    dict(C=32, grid=(5, 7), rel=None, R=1, B=3, acc=False, pattern=None),
    dict(C=32, grid=(16, 24), rel=None, R=1, B=1, acc=True, pattern=None),
]

# region_scale and col2im_region: `grid` is the INPUT grid (the pixel grid of x and of G); with ncls = 4 gz and the regions live on 2H x 2W
_DGRAD_KEYS = ("C", "Cy", "grid", "rel", "R", "B", "ncls")
_DGRAD_ROWS = [
    (8, 8, (5, 7), "larger", 5, 1, 1),
    (8, 32, (33, 50), "smaller", 12, 3, 1),
    (8, 8, (16, 24), "equal", 16, 3, 4),
    (32, 32, (13, 37), "equal", 16, 3, 1),
    (32, 8, (33, 50), "larger", 5, 1, 4),
    (32, 32, (16, 24), "smaller", 1, 1, 4),
    (64, 32, (16, 24), "larger", 12, 3, 1),
    (64, 8, (13, 37), "smaller", 16, 1, 4),
    (64, 8, (33, 50), "equal", 5, 3, 1),
    (1024, 8, (5, 7), "smaller", 16, 3, 4),
    (1024, 8, (5, 7), "equal", 1, 1, 1),
]
DGRAD_CASES = _cross(_DGRAD_ROWS, _DGRAD_KEYS)

# scale_dot has no label map; 41x51 > 2048 pixels is the smallest grid of this family with two row blocks, the second one short
SCALE_DOT_CASES = [dict(C=c, grid=g, B=b) for (c, g, b) in [
    (8, (5, 7), 1), (8, (33, 50), 3), (8, (41, 51), 3), (32, (13, 37), 3), (32, (16, 24), 1), (32, (41, 51), 1), (64, (5, 7), 3),
    (64, (33, 50), 1), (64, (13, 37), 1), (64, (41, 51), 3), (1024, (5, 7), 1), (1024, (5, 7), 3)]]

CASES = {"act": ACT_CASES, "demod": DEMOD_CASES, "torgb": TORGB_CASES, "dgrad": DGRAD_CASES, "scale_dot": SCALE_DOT_CASES}


def case_id(c):
    parts = []
    for k, v in c.items():
        if k == "grid":
            parts.append(f"{v[0]}x{v[1]}")
        elif isinstance(v, bool):
            parts.append(k if v else f"no{k}")
        elif isinstance(v, str):
            parts.append(v)
        elif v is None:
            parts.append(f"no{k}")
        else:
            parts.append(f"{k}{v}")
    return "-".join(parts)


def _labels_of(c, out_grid, seed):
    if c.get("pattern") is None:
        return None, None
    hm, wm = MAPS[out_grid][c["rel"]]
    labels = make_labels(c["pattern"], c["B"], hm, wm, c["R"], seed)
    return labels, region_map(labels, *out_grid)


def _gen(name, c, kind):
    seed = zlib.crc32(f"{name}-{case_id(c)}-{kind}".encode())
    return torch.Generator().manual_seed(seed), seed & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def build(name, index, kind):
    """The fp32 operands of case `index` of CASES[name] with `kind` data and their fp64 references, built once per session and shared:
    treat as read-only."""
    c = CASES[name][index]
    k = CONSTS[kind]
    g, seed = _gen(name, c, kind)
    B, (H, W), C = c["B"], c["grid"], c["C"]
    out = dict(case=c, **k)
    if name in ("act", "demod"):
        labels, reg = _labels_of(c, (H, W), seed)
        dy, y = operand((B, H, W, C), kind, g), operand((B, H, W, C), kind, g)
        noise = None if c["noise"] is None else operand((B if c["noise"] == "per" else 1, 1, H, W), kind, g)
        bias = operand((C,), kind, g) if c["bias"] else None
        ref = act_ref(dy, y, noise, k["noise_w"], bias, k["alpha"], k["gain"], reg, c["R"])
        out.update(dy=dy, y=y, noise=noise, bias=bias, labels=labels, reg=reg, ref=ref)
        if name == "demod":                   # demod_grad takes gz as an operand: the fp32 rounding of the exact one
            gz = ref["gz"].float()
            out.update(gz=gz, ref=act_ref(dy, y, noise, k["noise_w"], bias, k["alpha"], k["gain"], reg, c["R"], gz=gz))
    elif name == "torgb":
        labels, reg = _labels_of(c, (H, W), seed)
        drgb, x = operand((B, 3, H, W), kind, g), operand((B, H, W, C), kind, g)
        ws = operand((B * c["R"], 3, C), kind, g)
        acc = operand((B, H, W, C), kind, g) if c["acc"] else None
        out.update(drgb=drgb, x=x, ws=ws, acc=acc, labels=labels, reg=reg, ref=torgb_ref(drgb, x, ws, reg, c["R"], acc))
    elif name == "dgrad":
        os_ = 2 if c["ncls"] == 4 else 1
        labels, reg = _labels_of(c, (H * os_, W * os_), seed)
        gz, d = operand((B, H * os_, W * os_, c["Cy"]), kind, g), operand((B * c["R"], c["Cy"]), kind, g)
        x, s = operand((B, H, W, C), kind, g), operand((B * c["R"], C), kind, g)
        Wt = operand((c["ncls"], 9, c["Cy"], C), kind, g)
        ref = dgrad_ref(gz, d, x, s, Wt, reg, c["R"], c["ncls"])
        out.update(gz=gz, d=d, x=x, s=s, Wt=Wt, labels=labels, reg=reg, ref=ref, G=ref["G"].float())
    elif name == "scale_dot":
        u, x, s = operand((B, H, W, C), kind, g), operand((B, H, W, C), kind, g), operand((B, C), kind, g)
        out.update(u=u, x=x, s=s, ref=scale_dot_ref(u, x, s))
    else:
        raise KeyError(name)
    return out


# (output, S_abs, log2 of 1 / quantum of its terms on dyadic data) of every summed output
SUMMED = {
    "act": [("dd", "dd_abs", 6)],              # gz in 2^-3, z - nw noise - bias in 2^-3
    "demod": [("dd", "dd_abs", 6)],
    "torgb": [("dws", "dws_abs", 4), ("dx", "dx_abs", 4)],
    "dgrad": [("dx", "dx_abs", 8), ("ds", "ds_abs", 8)],          # G = sum_co (gz d) W in 2^-6, times s or x in 2^-2
    "scale_dot": [("ds", "ds_abs", 4)],
}
