"""Seeded cases and fp64 yardsticks for the exact-fp32 dgrad kernel (conv_bwd_kernel of csrc/conv_bwd.hip, reached through
e4s_conv_bwd_mfma_f32 and K.conv_bwd) and for three small kernels next to it (e4s_reduce_parts_f32, e4s_pack_taps_bwd_f32,
e4s_shift_scale_f32): the yardsticks of tests/test_conv_bwd_cases_host.py and tests/test_gpu_conv_bwd_kernel.py.  CPU only; the native
library is not imported here.  Label generators, region lookup, label-map sizes and operand data are those of tests/gen_bwd_cases.py.

The yardstick is the FORWARD definition in fp64, differentiated by autograd with s and d as independent leaves:
    out_pre[p, co] = d[r(p), co] sum_{tap, ci} W[cls][tap][co][ci] s[r(p), ci] x[src(p, tap), ci],   loss = sum gz out_pre,
    dx = d loss / d x,   ds = d loss / d s
ncls = 1: src(p, tap) = p + tap - 1 (zero padding).  ncls = 4: output pixel (2a + py, 2a' + px) of phase cls = 2 py + px reads
x[a + tap - 1], one arbitrary 3x3 weight set per phase.  r(p) is gen_bwd_cases.region_map on the OUTPUT grid (F.interpolate, nearest),
never a restatement of the kernel's lookup.  All operands are the fp32 values cast to double; an absent s or d is 1.

Two kinds of operand data:
  random  fp32 normal values.
  dyadic  x, W, gz integers in [-4, 4] times 2^-2; s and d signed powers of two in {1/2, 1, 2}, which add no mantissa bits.  A term
          s W d gz of dx is a multiple of 2^-1 2^-2 2^-1 2^-2 = 2^-6, a term x W d gz of ds a multiple of 2^-7 (QUANTUM_LOG2).  As long
          as S_abs / quantum < 2^24 (checked per output element by the host test) every product and every partial sum, in any order, is
          an fp32 number: the kernel's dx and ds have to EQUAL the reference.

Bounds on random data (derived here, not measured).  With u = 2^-24 and S_abs the fp64 sum of the absolute values of the terms of one
output element (|s W d gz| for dx, |x W d gz| for ds; computed by running the yardstick on the absolute values of the operands),
    |got - ref| <= (N + c) u S_abs   elementwise.
An fp32 evaluation multiplies every term by (1 + delta_1) .. (1 + delta_k), |delta| <= u, one factor per rounding the term passes
through: c roundings inside the term and one per addition of two non-zero partial sums on its way to the output (adding an exact 0.0 --
the start of an accumulator, a tap outside the image, a block without a tap group -- rounds nothing).  In a sum of N terms in ANY order a
term passes through at most N - 1 such additions, so k <= N - 1 + c and the error is at most ((1 + u)^k - 1) S_abs <= k u / (1 - k u)
S_abs <= (k + 1) u S_abs = (N + c) u S_abs as long as k (k + 1) u <= 1, i.e. k <= 4095; the largest N + c used here is below 500.
Both sums are nested, which is what puts the third rounding inside a term: s[r(p)] and x[q] multiply T, the sum over the Cy output
channels of one (pixel, tap), so that sum is complete before anything else is added.  A sum of n_1 terms whose results are summed n_2 at
a time takes a term through at most (n_1 - 1) + (n_2 - 1) additions, each level in any order; N is the smaller of the number of terms and
the sum of the level sizes, and both bound k - c + 1.
  dx  c = 3: gz d on the A fragment on its way into the MFMA, the product with W inside the MFMA (counted although the matrix core may
      fuse it into the addition), s T when the tap group's T enters the final accumulator.  Levels: the Cy channels, then the 9 ncls tap
      groups (in one block or as the ordered parts of a split: the same additions).  N = min(9 ncls Cy, Cy + 9 ncls).
  ds  c = 3: gz d, the product with W, x T in the tap-group epilogue.  The number of terms of a row is 9 Cy times the number of output
      pixels of the region, which reaches 10^6.  Levels: the Cy channels, the <= 128 rows of an 8 x 16 tile, the <= 9 ncls tap groups of a
      block, the P = tiles-per-sample x gsplit ordered parts.  N = min(9 Cy pixels(region), Cy + 128 + 9 ncls + P).

Restated launch rule (bwd_gsplit of csrc/conv_bwd.hip; `geometry`): the tile is 8 x 16 input pixels, a block owns 64 columns of Cx where
Cx % 64 == 0 and 32 otherwise, blocks = B tiles-per-sample column-tiles; blocks >= 256 -> gsplit 1, else min(512 // blocks, 9 ncls).
Block gs of a tile owns tap groups [gs gper, min((gs + 1) gper, 9 ncls)), gper = ceil(9 ncls / gsplit): the trailing blocks may own
none.  ds takes P = tiles-per-sample x gsplit parts of B R Cx floats, dx (gsplit > 1) gsplit parts of B Hx Wx Cx; a reduction over n
parts keeps ceil(n / 64) chunk sums behind the parts and uses them where n > 64 (`ws_floats`, `ws_used`).
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import gen_bwd_cases as gc
from gen_bwd_cases import PATTERNS, make_labels, operand, region_map  # noqa: F401

KINDS = ("dyadic", "random")
FORMS = ("sd", "d", "s", "none")          # which of s and d the call gets; ds exists where s does
TH, TW, RCHUNK = 8, 16, 64
U = 2.0 ** -24
C_DX = C_DS = 3
QUANTUM_LOG2 = {"dx": 6, "ds": 7}         # dyadic terms of dx are multiples of 2^-6, of ds of 2^-7

# label-map sizes of the output grids gen_bwd_cases.MAPS does not hold (one full tile; the 256-block case)
MAPS = dict(gc.MAPS)
MAPS.update({
    (8, 16): {"larger": (20, 36), "equal": (8, 16), "smaller": (3, 5)},
    (64, 128): {"larger": (100, 150), "equal": (64, 128), "smaller": (12, 17)},
})


# ---- the restated launch rule ----------------------------------------------------------------------------------------------------------
def geometry(c, B=None):
    """tiles, column tiles, split and parts of case `c` (at batch size B if given)."""
    B = c["B"] if B is None else B
    H, W = c["grid"]
    per_img = -(-H // TH) * (-(-W // TW))
    bn = 64 if c["Cx"] % 64 == 0 else 32
    ntn = c["Cx"] // bn
    blocks = B * per_img * ntn
    ngroups = 9 * c["ncls"]
    gsplit = 1 if blocks >= 256 else max(1, min(512 // blocks, ngroups))
    gper = -(-ngroups // gsplit)
    groups = [max(0, min((g + 1) * gper, ngroups) - g * gper) for g in range(gsplit)]
    if gsplit == 1:
        situation = "one"
    elif gsplit == ngroups:
        situation = "all"
    elif 0 in groups:
        situation = "idle"
    else:
        situation = "uneven" if len(set(groups)) > 1 else "even"
    R = c["R"] if c["pattern"] is not None else 1
    return dict(per_img=per_img, BN=bn, ntn=ntn, blocks=blocks, ngroups=ngroups, gsplit=gsplit, gper=gper, groups=groups,
                situation=situation, nchunk=c["Cy"] // 32, P=per_img * gsplit, two_level=per_img * gsplit > RCHUNK,
                nds=B * R * c["Cx"], ndx=B * H * W * c["Cx"], ragged=bool(H % TH or W % TW))


def reduce_ws_floats(nparts, n):
    return nparts * n + -(-nparts // RCHUNK) * n


def ws_floats(c, want_ds, B=None):
    """what e4s_conv_bwd_ws_floats has to answer"""
    g = geometry(c, B)
    n = reduce_ws_floats(g["P"], g["nds"]) if want_ds else 0
    if g["gsplit"] > 1:
        n += reduce_ws_floats(g["gsplit"], g["ndx"])
    return n


def ws_used(c, want_ds, B=None):
    """[(first, last + 1)] float ranges of the workspace that a call writes: all parts, the chunk sums only where a reduction has two
    levels (the dx parts never do: gsplit <= 36)."""
    g = geometry(c, B)
    out, off = [], 0
    if want_ds:
        out.append((0, g["P"] * g["nds"] + (-(-g["P"] // RCHUNK) * g["nds"] if g["two_level"] else 0)))
        off = reduce_ws_floats(g["P"], g["nds"])
    if g["gsplit"] > 1:
        out.append((off, off + g["gsplit"] * g["ndx"]))
    return out


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------
def _pix(tab, reg):
    """tab [B, R, C], reg int64 [B, Ho, Wo] -> the row of every pixel's region, [B, Ho, Wo, C]"""
    return tab[torch.arange(reg.shape[0])[:, None, None], reg]


def _shift(x, t):
    """x[m + t - 1] on the grid of m, zero outside"""
    H, W = x.shape[1:3]
    return F.pad(x, (0, 0, 1, 1, 1, 1))[:, t // 3:t // 3 + H, t % 3:t % 3 + W]


def forward(x, W, s, d, reg, ncls, mutate=None):
    """out_pre of the module docstring.  x [B, H, W, Ci]; W [ncls, 9, Co, Ci]; s [B R, Ci] or None; d [B R, Co] or None; reg int64
    [B, Ho, Wo].  `mutate` builds the two deliberate mistakes the host test has to tell from the truth:
      "region_of_q"  s and d taken at the region of the un-shifted pixel (the pixel of x, for ncls = 4 its own output pixel of the phase)
                     instead of the tap-shifted output pixel p
      "drop_tap"     phase 0, tap (+1, 0): the term that reads the last row of x is dropped"""
    B, H, Wd, Ci = x.shape
    os_ = 2 if ncls == 4 else 1
    spix = None if s is None else _pix(s.reshape(B, -1, Ci), reg)
    dpix = None if d is None else _pix(d.reshape(B, -1, W.shape[2]), reg)
    phases = []
    for ph in range(ncls):
        sl = (slice(None), slice(ph >> 1, None, os_), slice(ph & 1, None, os_))
        sp, dp = None if spix is None else spix[sl], None if dpix is None else dpix[sl]
        acc = 0
        for t in range(9):
            if mutate == "region_of_q":
                term = torch.einsum("bhwc,oc->bhwo", _shift(x if sp is None else x * sp, t), W[ph, t])
                if dp is not None:
                    term = term * _shift(dp, t)
            else:
                xs = _shift(x, t)
                if mutate == "drop_tap" and ph == 0 and t == 7:
                    keep = torch.ones(1, H, 1, 1, dtype=x.dtype)
                    keep[:, H - 2] = 0                       # output row H - 2 reads x row H - 1 through tap (+1, 0)
                    xs = xs * keep
                term = torch.einsum("bhwc,oc->bhwo", xs if sp is None else xs * sp, W[ph, t])
            acc = acc + term
        if mutate != "region_of_q" and dp is not None:
            acc = acc * dp
        phases.append(acc)
    if ncls == 1:
        return phases[0]
    out = torch.stack(phases, 0).reshape(2, 2, B, H, Wd, -1).permute(2, 3, 0, 4, 1, 5)        # [B, H, py, W, px, Co]
    return out.reshape(B, 2 * H, 2 * Wd, -1)


def grads(gz, W, x, s, d, reg, ncls, dtype=torch.float64, mutate=None):
    """(dx, ds) by autograd in `dtype`; ds is None without s."""
    cast = lambda t: None if t is None else t.to(dtype)                                       # noqa: E731
    xg = cast(x).requires_grad_(True)
    sg = None if s is None else cast(s).requires_grad_(True)
    loss = (cast(gz) * forward(xg, cast(W), sg, cast(d), reg, ncls, mutate)).sum()
    if sg is None:
        return torch.autograd.grad(loss, xg)[0], None
    return torch.autograd.grad(loss, (xg, sg))


def pack_bwd_ref(W):
    """forward pack [ncls, 9, Co, Ci] -> the kernel's [ncls, 9, Ci, Co] with the taps flipped"""
    return W.flip(1).transpose(2, 3).contiguous()


# ---- small companions ------------------------------------------------------------------------------------------------------------------
def reduce_parts_ref(parts, scale):
    """fp32 numpy [nparts, n] -> [n]: the parts added in index order from 0.0, in chunks of 64 first where nparts > 64 and then the chunk
    sums in order, then one product with scale."""
    parts = np.asarray(parts, dtype=np.float32)

    def in_order(rows):
        acc = np.zeros(rows.shape[1], dtype=np.float32)
        for row in rows:
            acc = (acc + row).astype(np.float32)
        return acc

    if parts.shape[0] > RCHUNK:
        parts = np.stack([in_order(parts[i:i + RCHUNK]) for i in range(0, parts.shape[0], RCHUNK)])
    return (in_order(parts) * np.float32(scale)).astype(np.float32)


def shift_scale_ref(x, tab, labels, R, anchors, istride, dy, dx, os_, py, px):
    """out[b, a, c] = tab[group][c] x[b, a istride + (dy, dx), c], exactly 0 outside the image: one fp32 product.  The group is b R + the
    region of output pixel a os + (py, px) on the [Ha os, Wa os] grid with labels, b without."""
    B, Hi, Wi, C = x.shape
    Ha, Wa = anchors
    iy, ix = torch.arange(Ha) * istride + dy, torch.arange(Wa) * istride + dx
    ok = ((iy >= 0) & (iy < Hi))[:, None] & ((ix >= 0) & (ix < Wi))[None, :]
    v = x[:, iy.clamp(0, Hi - 1)][:, :, ix.clamp(0, Wi - 1)]
    if labels is None:
        scale = tab.reshape(B, 1, 1, C)
    else:
        reg = region_map(labels, Ha * os_, Wa * os_)[:, py::os_, px::os_]
        scale = _pix(tab.reshape(B, R, C), reg)
    return torch.where(ok[None, :, :, None], v * scale, torch.zeros(()))


# ---- case list -------------------------------------------------------------------------------------------------------------------------
# `grid` is the INPUT grid (x and dx); with ncls = 4 gz and the regions live on 2H x 2W.  pattern None: no label map, R = 1.
_KEYS = ("grid", "Cx", "Cy", "B", "ncls", "R", "pattern", "rel", "form")
_ROWS = [
    ((8, 16), 64, 32, 1, 1, 3, "blocks", "equal", "sd"),          # one full tile
    ((5, 7), 64, 32, 3, 1, 12, "noise", "larger", "sd"),          # one partial tile
    ((13, 37), 64, 32, 1, 1, 16, "absent", "smaller", "sd"),      # 2 x 3 tiles, ragged both ways
    ((5, 7), 32, 32, 3, 1, 3, "absent", "equal", "sd"),           # BN = 32
    ((13, 37), 96, 32, 1, 1, 12, "blocks", "larger", "sd"),       # BN = 32, three column tiles
    ((16, 24), 128, 32, 1, 1, 16, "noise", "smaller", "sd"),      # BN = 64, two column tiles
    ((5, 7), 64, 64, 1, 1, 12, "one", "equal", "sd"),             # two K chunks per tap group
    ((16, 24), 32, 64, 1, 4, 3, "noise", "larger", "sd"),         # two K chunks, BN = 32, polyphase
    ((5, 7), 64, 32, 3, 4, 12, "blocks", "larger", "sd"),
    ((16, 24), 64, 32, 1, 4, 16, "absent", "equal", "sd"),
    ((13, 37), 64, 32, 1, 4, 12, "noise", "smaller", "sd"),
    ((16, 24), 64, 32, 3, 1, 12, "noise", "equal", "s"),
    ((13, 37), 64, 32, 1, 1, 12, "blocks", "smaller", "d"),
    ((5, 7), 64, 32, 1, 4, 16, "one", "larger", "d"),
    ((5, 7), 32, 32, 3, 4, 12, "noise", "equal", "s"),
    ((16, 24), 64, 32, 1, 1, 16, "one", "larger", "sd"),
    ((8, 16), 64, 32, 3, 1, 1, None, None, "sd"),                 # no label map: one group per sample
    ((5, 7), 32, 32, 1, 4, 1, None, None, "sd"),
    ((13, 37), 128, 64, 3, 1, 1, None, None, "none"),             # the encoder's call
    ((5, 7), 32, 32, 1, 1, 1, None, None, "none"),
    ((64, 128), 128, 32, 2, 1, 16, "noise", "larger", "sd"),      # 256 blocks: gsplit = 1
    ((33, 50), 64, 32, 1, 4, 12, "blocks", "larger", "sd"),       # 20 blocks, gsplit = 25: blocks 18 .. 24 of a tile own no tap group
    ((33, 50), 64, 32, 4, 1, 12, "noise", "smaller", "sd"),       # 80 blocks, gsplit = 6: block 5 of a tile owns no tap group
    ((33, 50), 64, 32, 3, 4, 12, "absent", "equal", "sd"),        # 60 blocks, gsplit = 8: 5, 5, 5, 5, 5, 5, 5, 1 groups
    ((33, 50), 64, 32, 5, 1, 3, "blocks", "equal", "s"),          # 100 blocks, gsplit = 5: 2, 2, 2, 2, 1 groups
]
CASES = [dict(zip(_KEYS, row)) for row in _ROWS]


def case_id(c):
    return gc.case_id(c)


def _pow2(shape, gen):
    """signed powers of two in {1/2, 1, 2}"""
    mag = torch.randint(-1, 2, tuple(shape), generator=gen).float()
    sign = torch.randint(0, 2, tuple(shape), generator=gen).float() * 2 - 1
    return sign * torch.exp2(mag)


def operands(c, kind):
    """the fp32 operands of a case: gz, W (forward pack), x, s, d (None where the form leaves them out), labels, reg"""
    seed = zlib.crc32(f"conv_bwd-{case_id(c)}-{kind}".encode())
    g = torch.Generator().manual_seed(seed)
    B, (H, Wd), os_ = c["B"], c["grid"], 2 if c["ncls"] == 4 else 1
    masked = c["pattern"] is not None
    R = c["R"] if masked else 1
    labels = None
    reg = torch.zeros(B, H * os_, Wd * os_, dtype=torch.int64)
    if masked:
        hm, wm = MAPS[(H * os_, Wd * os_)][c["rel"]]
        labels = make_labels(c["pattern"], B, hm, wm, R, seed & 0x7FFFFFFF)
        reg = region_map(labels, H * os_, Wd * os_)
    gz, x = operand((B, H * os_, Wd * os_, c["Cy"]), kind, g), operand((B, H, Wd, c["Cx"]), kind, g)
    W = operand((c["ncls"], 9, c["Cy"], c["Cx"]), kind, g)
    tab = _pow2 if kind == "dyadic" else (lambda shape, gen: torch.randn(tuple(shape), generator=gen))
    s = tab((B * R, c["Cx"]), g) if "s" in c["form"] else None
    d = tab((B * R, c["Cy"]), g) if "d" in c["form"] else None
    return dict(gz=gz, W=W, x=x, s=s, d=d, labels=labels, reg=reg, R=R)


@functools.lru_cache(maxsize=None)
def build(index, kind):
    """The operands of CASES[index] with `kind` data, the kernel's weight layout wt, and the fp64 reference: dx, ds (None without s),
    their S_abs, the term counts N of the bounds and the number of output pixels of every (sample, region).  Built once per session and
    shared: treat as read-only."""
    c = CASES[index]
    t = operands(c, kind)
    g = geometry(c)
    ab = lambda v: None if v is None else v.abs()                                             # noqa: E731
    dx, ds = grads(t["gz"], t["W"], t["x"], t["s"], t["d"], t["reg"], c["ncls"])
    # S_abs: the same sums over the absolute values of the terms.  dx does not depend on x, ds not on s.
    dx_abs, ds_abs = grads(ab(t["gz"]), ab(t["W"]), ab(t["x"]), ab(t["s"]), ab(t["d"]), t["reg"], c["ncls"])
    count = F.one_hot(t["reg"].reshape(c["B"], -1), t["R"]).sum(1).reshape(-1)               # output pixels per (sample, region)
    depth = c["Cy"] + TH * TW + g["ngroups"] + g["P"]
    t.update(case=c, geom=g, wt=pack_bwd_ref(t["W"]), dx=dx, ds=ds, dx_abs=dx_abs, ds_abs=ds_abs, count=count,
             n_dx=min(9 * c["ncls"] * c["Cy"], c["Cy"] + g["ngroups"]), n_ds=(9 * c["Cy"] * count).clamp(max=depth))
    return t


def bound(sabs, n, c):
    """(N + c) 2^-24 S_abs; n an int or one count per leading row of sabs"""
    if torch.is_tensor(n):
        n = n.double().reshape(-1, *([1] * (sabs.dim() - 1)))
    return (n + c) * U * sabs


# ---- the small kernels' cases ----------------------------------------------------------------------------------------------------------
REDUCE_NPARTS = (1, 7, 8, 9, 64, 65, 130)
REDUCE_N = (4, 1000, 1003)                 # 1003 is no multiple of 4: the scalar path
REDUCE_SCALES = (1.0, 0.5)
PACK_SHAPES = [(1, 64, 32), (4, 32, 96), (1, 48, 40), (4, 48, 40)]          # (ncls, Cout, Cin): two tiled, two scalar


def reduce_parts_data(nparts, n, kind):
    g = torch.Generator().manual_seed(zlib.crc32(f"reduce-{nparts}-{n}-{kind}".encode()))
    return operand((nparts, n), kind, g)


# x is [2, 9, 11, 8]; labels [2, 7, 5] with 5 regions
SHIFT_X, SHIFT_MAP, SHIFT_R = (2, 9, 11, 8), (7, 5), 5
SHIFT_CASES = [dict(labels=lab, os=os_, py=py, px=px, istride=st, dy=dy, dx=dx, anchors=(9, 11) if st == 1 else (5, 6))
               for lab in (True, False) for (os_, py, px) in ((1, 0, 0), (2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1))
               for (st, dy, dx) in ((1, -1, 1), (1, 1, -1), (2, -1, -1), (2, 1, 1), (2, 0, 0))]
