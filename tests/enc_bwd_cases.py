"""Seeded cases and fp64 yardsticks for the streaming kernels of the encoder backward (csrc/encoder_bwd.hip: instnorm_bwd, instnorm_bwd_sums,
prelu, prelu_bwd, strided_scatter, strided_place, pixel_unshuffle2, region_mean_bwd) and the unmasked torgb_bwd_w wrapper: the yardsticks
of tests/test_enc_bwd_cases_host.py and tests/test_gpu_encoder_backward_kernels.py.  CPU only; the native library is not imported here.

The region of a pixel is what F.interpolate(labels as fp32, size=(H, W), mode="nearest") gives on the CPU (gen_bwd_cases.region_map), never
a restatement of the kernels' nearest_src.  Every reference takes the fp32 operands cast to double.

Two kinds of operand data (gen_bwd_cases.operand):
  random  fp32 normal values.  InstanceNorm: x is scaled and shifted differently per (b, c) and `stats` are the fp32 ones the caller got
          from K.instnorm_stats (the host tests use host_stats), so in_ref is evaluated by the caller.
  dyadic  integers in [-4, 4] times 2^-2.  InstanceNorm takes `stats` as an input, so they are chosen: mean a multiple of 2^-2 in
          [-1/2, 1/2], rstd in {1/2, 1, 2, 4}, gate in {1/2, 1, 2}.  Every output that does not involve 1 / (a number that is no power of
          two) then has to EQUAL the reference; the host test proves this per case by evaluating the formulas in fp32.  The two outputs
          that do involve such a quotient are held to the random bound instead and are named by the builders (`exact` False):
            dx of instnorm_bwd on a grid whose H W is no power of two (A / N and Bq / N), whose sums are still exact;
            dfeat of region_mean_bwd with a region whose pixel count is no power of two (only the hand-built "pow2" maps are exact).

Bounds for random data, u = 2^-24, derived from the kernels' operation chains (recounted in csrc/encoder_bwd.hip; an FMA contraction only
removes roundings):
  sums[..., 0] = A   in_bwd_partial_kernel adds (double)dy in double, in_bwd_finalize_kernel adds the splits in double and casts once:
                     u |A| for the cast plus N 2^-53 sum|dy| for the double additions.  The bound is 2u |A|; it is a bound as long as
                     N 2^-53 sum|dy| <= u |A|, which the host test checks for every random case.
  sums[..., 1] = Bq  xh = fl(fl(x - mean) rstd) carries two fp32 roundings; (double)dy (double)xh is exact in double (24 + 24 bits), the
                     additions are in double and the cast is one rounding: (2u + u^2) S_abs + u |Bq| + N 2^-53 S_abs < 4u S_abs,
                     S_abs = sum_p |dy| |xhat|.  The bound is 4u S_abs (three roundings counted, one to spare).
  dx                 in_bwd_apply_kernel: o = fl(fl(rstd gate) fl(fl(dy - a) - t)), a = fl(s0 invn), t = fl(fl(xh s1) invn),
                     invn = fl(1 / N), s0 = A (1 + 2u), s1 = Bq + e with |e| <= 4u S_abs (above).  Roundings that reach each term:
                       dy:              the two subtractions, rstd gate, the final product                              4
                       A / N:           s0 2, invn 1, s0 invn 1, and the same 4                                         8
                       xhat Bq / N:     xh 2, xh s1 1, invn 1, (..) invn 1, second subtraction, rstd gate, product      8
                       xhat S_abs / N:  the error e of s1, which is relative to S_abs and NOT to |Bq|                   4
                     one more each for the second-order terms of (1 + u)^k:
                       |err| <= u rstd |gate| (5 |dy| + 9 |A| / N + 9 |xhat| |Bq| / N + 4 |xhat| S_abs / N)   (+ u |result| accumulating).
                     This differs from c = 12 on the first three terms alone: that form has no term for the error of s1, which does not
                     shrink with |Bq| when the products dy xhat cancel.  The GPU test asserts the form above and prints the ratio to
                     the 12 u form next to it.
  prelu y, du        one product: u |ref|; positions with u > 0 are copies and exact.
  dslope, dws        an fp32 sum of N terms in any order plus one rounding per term: (N + 4) u S_abs, the bound of
                     tests/test_gpu_gen_backward_kernels.py, N the number of terms (pixels with u <= 0 of that channel; H W for dws).
  region_mean_bwd    inv = fl(1 / count) (count < 2^24 is exact in fp32) and one product: 3u |dcodes / count| (two roundings and their
                     second-order term), + u |result| for the addition when accumulating.
  strided_scatter (accumulate) is one fp32 addition, correctly rounded on the CPU too: torch.equal with the fp32 sum.  The zero-insert
  scatter, strided_place and pixel_unshuffle2 are copies: torch.equal.
"""
import functools
import zlib

import torch

import gen_bwd_cases as gc
from gen_bwd_cases import KINDS, MAPS, make_labels, operand, region_map, torgb_ref  # noqa: F401

U = 2.0 ** -24
EPS = 1e-5


# ---- the split arithmetic of csrc/encoder_bwd.hip, restated for the host test and for the batch-independence checks ---------------------
def in_nsplit(B, HW, C):
    d = B * (C // 64)
    ns = max(2048 // (d if d > 0 else 1), 1)
    return ns if ns <= HW // 64 else max(HW // 64, 1)


def prelu_nsplit(npix, C):
    ns = 2048 // max(C // 64, 1)
    return max(ns if ns <= npix // 64 else max(npix // 64, 1), 1)


def split_path(n, nsplit):
    """which of the paths the last split of n pixels cut into nsplit takes: "single", "even", "ragged" (shorter than the others) or "empty" """
    if nsplit == 1:
        return "single"
    per = -(-n // nsplit)
    last = n - (nsplit - 1) * per
    return "empty" if last <= 0 else "ragged" if last < per else "even"


# ---- fp64 references ---------------------------------------------------------------------------------------------------------------------
def host_stats(x, eps=EPS):
    """fp32 [B, C, 2] = {mean, 1 / sqrt(var + eps)} of NHWC x, from fp64 (what K.instnorm_stats returns up to its own rounding)."""
    xd = x.double()
    mean, var = xd.mean((1, 2)), xd.var((1, 2), unbiased=False)
    return torch.stack([mean, (var + eps).rsqrt()], -1).float()


def in_ref(dy, x, stats, gate=None, acc=None):
    """A = sum_p dy, Bq = sum_p dy xhat, xhat = (x - mean) rstd;  dx = rstd gate (dy - A / N - xhat Bq / N) (+ acc), with their bounds."""
    B, H, W, C = x.shape
    N = H * W
    dyd, xd = dy.double().reshape(B, N, C), x.double().reshape(B, N, C)
    mean, rstd = stats[..., 0].double()[:, None], stats[..., 1].double()[:, None]
    xhat = (xd - mean) * rstd
    A, Bq = dyd.sum(1, keepdim=True), (dyd * xhat).sum(1, keepdim=True)
    A_abs, S_abs = dyd.abs().sum(1, keepdim=True), (dyd.abs() * xhat.abs()).sum(1, keepdim=True)
    gt = torch.ones_like(rstd) if gate is None else gate.double()[:, None]
    dx = rstd * gt * (dyd - A / N - xhat * Bq / N)
    scale = U * rstd.abs() * gt.abs()
    bound = scale * (5 * dyd.abs() + 9 * A.abs() / N + 9 * xhat.abs() * Bq.abs() / N + 4 * xhat.abs() * S_abs / N)
    bound12 = 12 * scale * (dyd.abs() + A.abs() / N + xhat.abs() * Bq.abs() / N)
    if acc is not None:
        dx = dx + acc.double().reshape(B, N, C)
        bound, bound12 = bound + U * dx.abs(), bound12 + U * dx.abs()
    sh = (B, H, W, C)
    return dict(dx=dx.reshape(sh), dx_bound=bound.reshape(sh), dx_bound12=bound12.reshape(sh), sums=torch.cat([A, Bq], 1).transpose(1, 2),
                sums_bound=torch.cat([2 * U * A.abs(), 4 * U * S_abs], 1).transpose(1, 2), A_abs=A_abs[:, 0], S_abs=S_abs[:, 0])


def prelu_ref(dy, u, slope):
    """y = u > 0 ? u : u slope[c];  du = u > 0 ? dy : dy slope[c];  dslope[c] = sum over {u <= 0} of dy u.  n[c]: the number of those."""
    C = u.shape[-1]
    ud, dyd, a = u.double().reshape(-1, C), dy.double().reshape(-1, C), slope.double()
    pos = ud > 0
    terms = torch.where(pos, torch.zeros_like(ud), dyd * ud)
    y, du = torch.where(pos, ud, ud * a), torch.where(pos, dyd, dyd * a)
    zero = torch.zeros_like(ud)
    return dict(y=y.reshape(u.shape), du=du.reshape(u.shape), y_bound=torch.where(pos, zero, U * y.abs()).reshape(u.shape),
                du_bound=torch.where(pos, zero, U * du.abs()).reshape(u.shape), dslope=terms.sum(0), dslope_abs=terms.abs().sum(0),
                n=(~pos).sum(0))


def scatter_ref(src, s, prior=None):
    """fp32 [B, H s, W s, C]: src at the positions (y s, x s); elsewhere 0, or `prior`, which the hit positions add to in fp32."""
    B, H, W, C = src.shape
    out = torch.zeros(B, H * s, W * s, C) if prior is None else prior.clone()
    out[:, ::s, ::s] += src
    hit = torch.zeros(H * s, W * s, dtype=torch.bool)
    hit[::s, ::s] = True
    return out, hit


def place_ref(src, s, oy, ox, out_hw):
    B, H, W, C = src.shape
    out = torch.zeros(B, out_hw[0], out_hw[1], C)
    out[:, oy:oy + (H - 1) * s + 1:s, ox:ox + (W - 1) * s + 1:s] = src
    return out


def unshuffle_ref(x):
    """[B, 2H, 2W, C] -> [B, H, W, 4C]: channel (py 2 + px) C + c of pixel (a, b) = x[2a + py, 2b + px, c]."""
    B, H2, W2, C = x.shape
    return x.view(B, H2 // 2, 2, W2 // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H2 // 2, W2 // 2, 4 * C)


def region_counts(reg, R):
    """int64 [B, R]: the pixels of every region; a label >= R belongs to no region."""
    return torch.stack([torch.bincount(r[r < R], minlength=R) for r in reg.reshape(reg.shape[0], -1)])


def region_ref(dcodes, reg, R, C, off, acc=None):
    """dfeat[b, p, c] = dcodes[b, r(p), off + c] / count[b, r(p)] (+ acc); a pixel whose label is >= R gets 0 (keeps acc)."""
    B = reg.shape[0]
    valid, idx = (reg < R)[..., None], reg.clamp(max=R - 1)
    counts = region_counts(reg, R)
    bi = torch.arange(B)[:, None, None]
    rows = dcodes.double()[bi, idx][..., off:off + C]
    q = torch.where(valid, rows / counts[bi, idx].double()[..., None], torch.zeros_like(rows))
    dfeat, bound = q, 3 * U * q.abs()
    if acc is not None:
        dfeat = q + acc.double()
        bound = torch.where(valid, bound + U * dfeat.abs(), torch.zeros_like(q))          # untouched pixels keep their bits
    return dict(dfeat=dfeat, bound=bound, counts=counts, valid=valid[..., 0])


# ---- case lists --------------------------------------------------------------------------------------------------------------------------
# InstanceNorm backward and PReLU backward: C = one, two and three 64-channel slabs.  (5, 7): H W < 64, one split, a pixel-group tail;
# (4, 8), (8, 8), (16, 32): H W a power of two (the grids on which dyadic dx is exact: one split, one split of exactly 64, 8 even splits);
# (16, 24): 6 even splits; (13, 37): 7 splits of 69, the last one ragged; (65, 65) with B = 1, C = 64: 66 splits of 65, the last one empty.
_IN_KEYS = ("C", "grid", "B", "gate", "acc")
IN_CASES = [dict(zip(_IN_KEYS, row)) for row in [
    (64, (5, 7), 1, False, False),
    (128, (5, 7), 3, True, True),
    (64, (4, 8), 3, True, False),
    (128, (8, 8), 1, False, True),
    (64, (16, 32), 3, True, True),
    (192, (16, 32), 1, False, False),
    (64, (16, 24), 3, True, False),
    (192, (16, 24), 1, False, True),
    (128, (13, 37), 1, True, True),
    (192, (13, 37), 3, False, False),
    (64, (13, 37), 3, False, True),
    (64, (65, 65), 1, True, True),
    (64, (65, 65), 1, False, False),
]]

# slope "rand": a PReLU's; "zero": the ReLU backward of the LPIPS trunk.  bwd False: a channel count only the forward takes.
_PRELU_KEYS = ("C", "grid", "B", "slope", "bwd")
PRELU_CASES = [dict(zip(_PRELU_KEYS, row)) for row in [
    (64, (5, 7), 1, "rand", True),
    (128, (5, 7), 3, "zero", True),
    (64, (16, 24), 3, "rand", True),
    (192, (16, 24), 1, "zero", True),
    (128, (13, 37), 1, "rand", True),
    (192, (13, 37), 3, "rand", True),
    (64, (13, 37), 3, "zero", True),
    (64, (65, 65), 1, "rand", True),
    (64, (65, 65), 1, "zero", True),
    (4, (5, 7), 3, "rand", False),
    (68, (13, 37), 1, "rand", False),
]]

SCATTER_CASES = [dict(s=s, C=C, grid=g, B=1 if (s + i + j) % 2 else 3)
                 for s in (1, 2, 3) for i, C in enumerate((4, 64, 68)) for j, g in enumerate(((1, 1), (5, 7), (16, 24)))]

# out_hw = the minimum ((H - 1) s + oy + 1, (W - 1) s + ox + 1) + extra
_PLACE_KEYS = ("C", "grid", "B", "s", "oy", "ox", "extra")
PLACE_CASES = [dict(zip(_PLACE_KEYS, row)) for row in [
    (64, (5, 7), 1, 2, 1, 1, (0, 0)),          # (10, 14): the minimum
    (4, (5, 7), 3, 2, 1, 1, (1, 1)),           # (11, 15): odd
    (64, (16, 24), 1, 2, 1, 1, (2, 3)),        # (34, 51): larger
    (4, (16, 24), 3, 2, 0, 0, (0, 0)),         # (31, 47): the minimum, odd
    (68, (5, 7), 1, 2, 0, 0, (1, 2)),          # (10, 15)
    (64, (1, 1), 3, 2, 0, 0, (0, 0)),          # (1, 1)
    (8, (5, 7), 3, 3, 2, 1, (0, 0)),           # (15, 20)
    (8, (5, 7), 1, 3, 0, 2, (2, 1)),           # (15, 22)
]]

UNSHUFFLE_CASES = [dict(C=C, grid=g, B=B) for C in (4, 36, 64) for g in ((1, 1), (3, 5), (16, 24)) for B in (1, 3)]

# region_mean_bwd: stride = off + C + 64 (the rows of dcodes are wider than the window).  Every row with every pattern of
# gen_bwd_cases.make_labels; "pow2": hand-built maps of 16 x 16 pixel cells on a 64 x 32 grid whose region counts are powers of two and
# differ between the samples; "out_of_range": a "blocks" map with a row of label R, rows of label 255 and a column of 200.
_REGION_KEYS = ("C", "grid", "rel", "R", "B", "off", "acc")
_REGION_ROWS = [
    (64, (5, 7), "larger", 3, 1, 0, False),
    (64, (13, 37), "smaller", 12, 3, 64, True),
    (64, (16, 24), "equal", 16, 3, 0, True),
    (256, (13, 37), "equal", 16, 1, 64, False),
    (256, (16, 24), "larger", 12, 3, 0, False),
    (256, (5, 7), "smaller", 3, 3, 64, True),
    (64, (33, 50), "larger", 16, 1, 64, True),
    (256, (33, 50), "smaller", 3, 1, 0, False),
]
POW2_GRID = (64, 32)
POW2_MAPS = {"larger": (128, 64), "equal": (64, 32), "smaller": (4, 2)}            # integer ratios: cells of 32, 16 and 1 label(s)
POW2_CELLS = [[0, 1, 1, 2, 2, 2, 2, 3], [5, 5, 5, 5, 5, 5, 5, 5], [0, 0, 1, 1, 2, 2, 3, 3]]          # per sample, 4 x 2 cells, row-major
REGION_CASES = [dict(zip(_REGION_KEYS, row), pattern=p) for p in ("blocks", "noise", "absent", "one") for row in _REGION_ROWS] + [
    dict(C=64, grid=POW2_GRID, rel="equal", R=12, B=3, off=0, acc=False, pattern="pow2"),
    dict(C=64, grid=POW2_GRID, rel="larger", R=16, B=3, off=64, acc=True, pattern="pow2"),
    dict(C=256, grid=POW2_GRID, rel="smaller", R=12, B=1, off=64, acc=True, pattern="pow2"),
    dict(C=64, grid=(13, 37), rel="larger", R=12, B=3, off=64, acc=False, pattern="out_of_range"),
    dict(C=64, grid=(13, 37), rel="larger", R=12, B=3, off=0, acc=True, pattern="out_of_range"),
]

TORGBW_CASES = [dict(C=C, grid=g, B=B) for C in (32, 64, 192) for g in ((5, 7), (13, 37), (33, 50)) for B in (1, 3)]

CASES = {"in": IN_CASES, "prelu": PRELU_CASES, "scatter": SCATTER_CASES, "place": PLACE_CASES, "unshuffle": UNSHUFFLE_CASES,
         "region": REGION_CASES, "torgbw": TORGBW_CASES}


def case_id(c):
    return gc.case_id({k: f"{v[0]}x{v[1]}" if isinstance(v, tuple) and k != "grid" else v for k, v in c.items()})


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def place_min_hw(c):
    (h, w), s = c["grid"], c["s"]
    return (h - 1) * s + c["oy"] + 1, (w - 1) * s + c["ox"] + 1


def region_labels(c, seed):
    """uint8 [B, Hm, Wm] of a region case."""
    B, R, p = c["B"], c["R"], c["pattern"]
    if p == "pow2":
        hm, wm = POW2_MAPS[c["rel"]]
        cells = torch.tensor(POW2_CELLS[:B], dtype=torch.uint8).reshape(B, 4, 2)
        return cells.repeat_interleave(hm // 4, 1).repeat_interleave(wm // 2, 2)
    hm, wm = MAPS[c["grid"]][c["rel"]]
    if p == "out_of_range":
        lab = make_labels("blocks", B, hm, wm, R, seed)
        lab[:, 0], lab[:, -3:] = R, 255          # three rows: the resize to a smaller grid skips single ones
        lab[-1, :, 0] = 200
        return lab
    return make_labels(p, B, hm, wm, R, seed)


def _gen(name, c, kind):
    seed = zlib.crc32(f"enc-{name}-{case_id(c)}-{kind}".encode())
    return torch.Generator().manual_seed(seed), seed & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def build(name, index, kind):
    """The fp32 operands of case `index` of CASES[name] with `kind` data and their references, built once per session and shared: treat as
    read-only.  `exact`: the dyadic outputs EQUAL the reference (see the module docstring for the two that cannot)."""
    c = CASES[name][index]
    g, seed = _gen(name, c, kind)
    B, (H, W), C = c["B"], c["grid"], c["C"]
    out = dict(case=c, exact=kind == "dyadic")
    if name == "in":
        dy, x = operand((B, H, W, C), kind, g), operand((B, H, W, C), kind, g)
        acc = operand((B, H, W, C), kind, g) if c["acc"] else None
        if kind == "dyadic":
            mean = torch.randint(-2, 3, (B, C), generator=g).float() * 0.25
            rstd = 2.0 ** torch.randint(-1, 3, (B, C), generator=g).float()
            gate = 2.0 ** torch.randint(-1, 2, (B, C), generator=g).float() if c["gate"] else None
            stats = torch.stack([mean, rstd], -1)
            out.update(stats=stats, ref=in_ref(dy, x, stats, gate, acc), exact_dx=is_pow2(H * W))
        else:                                      # a different mean and rstd per (b, c); stats and the reference are the caller's
            x = x * (0.25 + 2 * torch.rand((B, 1, 1, C), generator=g)) + torch.randn((B, 1, 1, C), generator=g)
            gate = 2 * torch.rand((B, C), generator=g) - 0.5 if c["gate"] else None
            out.update(stats=None, ref=None, exact_dx=False)
        out.update(dy=dy, x=x, gate=gate, acc=acc)
    elif name == "prelu":
        dy, u = operand((B, H, W, C), kind, g), operand((B, H, W, C), kind, g)
        flat = u.view(-1, C)
        if C > 2:                                  # exact +0.0 and -0.0 in the channels from 2 on (the first pixel and 1 in 16 of the rest)
            z = torch.rand(flat[:, 2:].shape, generator=g)
            flat[:, 2:][z < 1 / 16] = 0.0
            flat[:, 2:][z > 15 / 16] = -0.0
            flat[0, 2], flat[0, 3] = 0.0, -0.0
        flat[:, 0] = flat[:, 0].abs() + 0.25       # all positive: dslope[0] is exactly 0
        flat[:, 1] = -flat[:, 1].abs()             # all non-positive
        flat[0, 1] = -0.0
        if c["slope"] == "zero":
            slope = torch.zeros(C)
        else:
            slope = operand((C,), kind, g) if kind == "dyadic" else 0.25 + 0.25 * torch.randn(C, generator=g)
        out.update(dy=dy, u=u, slope=slope, ref=prelu_ref(dy, u, slope))
    elif name == "scatter":
        s = c["s"]
        src, prior = operand((B, H, W, C), kind, g), operand((B, H * s, W * s, C), kind, g)
        prior.view(-1)[::7] = -0.0                 # 0 + (-0.0) is +0.0: a position that is re-added instead of skipped changes its bits
        out.update(src=src, prior=prior, zero=scatter_ref(src, s)[0], accum=scatter_ref(src, s, prior)[0], hit=scatter_ref(src, s)[1])
    elif name == "place":
        src = operand((B, H, W, C), kind, g)
        hw = tuple(m + e for m, e in zip(place_min_hw(c), c["extra"]))
        out.update(src=src, out_hw=hw, ref=place_ref(src, c["s"], c["oy"], c["ox"], hw))
    elif name == "unshuffle":
        x = operand((B, 2 * H, 2 * W, C), kind, g)
        out.update(x=x, ref=unshuffle_ref(x))
    elif name == "region":
        R, off = c["R"], c["off"]
        labels = region_labels(c, seed)
        reg = region_map(labels, H, W)
        dcodes = operand((B, R, off + C + 64), kind, g)
        acc = operand((B, H, W, C), kind, g) if c["acc"] else None
        if acc is not None:
            acc.view(-1)[::7] = -0.0               # as in the scatter cases: 0 + (-0.0) would change the bits of a pixel of no region
        counts = region_counts(reg, R)
        # what the kernel has no business reading is NaN: the rows of regions without a pixel and the columns outside [off, off + C)
        dcodes[counts == 0] = float("nan")
        dcodes[:, :, :off] = float("nan")
        dcodes[:, :, off + C:] = float("nan")
        ref = region_ref(dcodes, reg, R, C, off, acc)
        out.update(labels=labels, reg=reg, dcodes=dcodes, acc=acc, ref=ref,
                   exact=kind == "dyadic" and all(is_pow2(int(n)) for n in counts.flatten() if n > 0))
    elif name == "torgbw":
        drgb, x = operand((B, 3, H, W), kind, g), operand((B, H, W, C), kind, g)
        out.update(drgb=drgb, x=x, ref=torgb_ref(drgb, x, torch.zeros(B, 3, C), None, 1))
    else:
        raise KeyError(name)
    return out
