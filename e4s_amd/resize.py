"""Pillow's `Image.resize` of 8-bit RGB images on the device, bit for bit (e4s_amd/csrc/resize.hip): what scripts/face_swap.py:184,
190-191 does to an un-cropped frame (`.resize((1024, 1024))`, BICUBIC) and what crop_image's shrink branch does to a large one
(src/utils/alignmengt.py:107-112, LANCZOS under its old name ANTIALIAS).

Pillow resamples in two passes, horizontal into a uint8 intermediate and then vertical, each a sum of 8-bit pixels times integer
coefficients with 22 fractional bits; the coefficients come from a float64 computation per output index.  `coefficients` restates
that computation (libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc) in numpy in Pillow's operation order; the
kernels do the integer part.  The tables are uploaded once per geometry and cached, so a repeated call is launches only: no
host-to-device copy, no synchronisation, capturable in a graph (the captured graph reads the cached tables: keep fewer than
CACHE_SIZE other geometries in flight while it lives, or the oldest is evicted).

Out of scope: NEAREST (another code path in Pillow), `reducing_gap`, every mode but 8-bit RGB."""
import collections

import numpy as np
import torch

from .lib import call, ptr, stream

NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 0, 1, 2, 3, 4, 5           # PIL.Image.Resampling
PRECISION_BITS = 32 - 8 - 2
CACHE_SIZE = 64
_TILES = ((128, 8), (64, 8), (32, 8), (16, 8), (8, 8), (4, 8), (4, 1))          # (output pixels, rows) of a block of the horizontal pass
_LDS_LIMIT = 64 * 1024


# ---- the filters (Resample.c), on float64 arrays -------------------------------------------------------------------------
def _sinc(x):
    px = x * np.pi
    with np.errstate(all="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(px) / px)


def _box(x):
    return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _hamming(x):
    x = np.abs(x)
    px = x * np.pi
    with np.errstate(all="ignore"):
        v = np.sin(px) / px * (0.54 + 0.46 * np.cos(px))
    return np.where(x == 0.0, 1.0, np.where(x >= 1.0, 0.0, v))


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _lanczos(x):
    return np.where((-3.0 <= x) & (x < 3.0), _sinc(x) * _sinc(x / 3), 0.0)


FILTERS = {BOX: (_box, 0.5), BILINEAR: (_bilinear, 1.0), HAMMING: (_hamming, 1.0), BICUBIC: (_bicubic, 2.0), LANCZOS: (_lanczos, 3.0)}


def coefficients(in_size, out_size, resample, in0, in1):
    """precompute_coeffs + normalize_coeffs_8bpc for one axis: input length in_size, box [in0, in1), output length out_size ->
    (bounds int32 [out_size,2] = (first input index, number of taps), kk int32 [out_size,ksize] with 22 fractional bits)."""
    if resample not in FILTERS:
        raise ValueError(f"resample must be BOX, BILINEAR, HAMMING, BICUBIC or LANCZOS, got {resample!r}")
    f, s = FILTERS[resample]
    in_size, out_size, in0, in1 = int(in_size), int(out_size), float(in0), float(in1)
    scale = (in1 - in0) / out_size
    filterscale = max(scale, 1.0)
    support = s * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = in0 + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                      # (int): truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    used = x < xmax[:, None]
    k = np.where(used, f(((x + xmin[:, None]) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(k, axis=1)[:, -1:]                                                    # left to right; the unused tail adds 0.0
    with np.errstate(all="ignore"):
        k = np.where(ww != 0.0, k / ww, k)
    scaled = k * float(1 << PRECISION_BITS)
    kk = np.where(k < 0, scaled - 0.5, scaled + 0.5).astype(np.int64)                    # (int): truncation
    return np.stack([xmin, xmax], axis=1).astype(np.int32), np.where(used, kk, 0).astype(np.int32)


def _identity(n):
    """The tables of a pass Pillow skips: one tap of weight 1, which reproduces every level."""
    return (np.stack([np.arange(n), np.ones(n, dtype=np.int64)], axis=1).astype(np.int32),
            np.full((n, 1), 1 << PRECISION_BITS, dtype=np.int32))


def passes(in_wh, size, box=None):
    """(horizontal, vertical): which of its two passes ImagingResample runs for a W x H image resized to `size` = (w, h)."""
    (W, H), (w, h) = in_wh, size
    x0, y0, x1, y1 = (0, 0, W, H) if box is None else box
    return bool(w != W or x0 != 0 or x1 != W), bool(h != H or y0 != 0 or y1 != H)


# ---- device tables, cached per geometry ----------------------------------------------------------------------------------
class _Axis(object):
    """One axis of one geometry on one device: the two tables and, per tile width of the horizontal pass, the largest number of
    input pixels that many consecutive outputs read."""

    def __init__(self, bounds, kk, device):
        self.bounds_host, self.ksize = bounds, int(kk.shape[1])
        self.bounds = torch.from_numpy(np.ascontiguousarray(bounds)).to(device)
        self.kk = torch.from_numpy(np.ascontiguousarray(kk)).to(device)
        first, end = bounds[:, 0].astype(np.int64), bounds[:, 0].astype(np.int64) + bounds[:, 1]
        n = len(first)
        self.span = {tx: int((end[np.minimum(np.arange(n) + tx - 1, n - 1)] - first).max()) for tx in sorted({t for t, _ in _TILES})}


_cache = collections.OrderedDict()


def _axis(device, in_size, out_size, resample, in0, in1, needed):
    key = (str(device), int(in_size), int(out_size), int(resample), float(in0), float(in1), bool(needed))
    hit = _cache.get(key)
    if hit is None:
        tables = coefficients(in_size, out_size, resample, in0, in1) if needed else _identity(out_size)
        hit = _cache[key] = _Axis(*tables, device)
        while len(_cache) > CACHE_SIZE:
            _cache.popitem(last=False)                                                   # the oldest entry
    return hit


def _tile(axis, width):
    """The widest tile of the horizontal pass whose staged rows fit in LDS -> (tx, rh, span)."""
    for tx, rh in _TILES:
        if tx > 4 and tx >= 2 * width:
            continue                                                                     # a narrow output: no block mostly idle
        span = axis.span[tx]
        if ((span * 3 + 15) // 16 + 1) * 16 * rh <= _LDS_LIMIT:
            return tx, rh, span
    raise ValueError(f"pil_resize: a tile of 4 output pixels reads {axis.span[4]} input pixels, more than the kernel stages")


def pil_resize(images_u8, size, resample=BICUBIC, box=None, window=None, out=None):
    """np.asarray(Image.fromarray(img).resize(size, resample, box=box)) for every image of a uint8 [B,H,W,3] (or [H,W,3]) device
    tensor.  size = (width, height); box = (x0, y0, x1, y1) floats in input pixels (default: the whole image); window = (x0, y0, x1,
    y1) ints in OUTPUT pixels: only that rectangle of the result is computed -> uint8 [B,y1 - y0,x1 - x0,3].  out: write there."""
    t = images_u8
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3 or t.numel() == 0:
        got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"pil_resize: images are a uint8 RGB tensor [B,H,W,3] or [H,W,3], got {got}")
    if not t.is_cuda:
        raise RuntimeError("pil_resize: images must be on the ROCm device (no CPU path)")
    if not t.is_contiguous():
        raise RuntimeError("pil_resize: images must be contiguous")
    if resample not in FILTERS:
        raise ValueError(f"pil_resize: resample is BOX, BILINEAR, HAMMING, BICUBIC or LANCZOS (NEAREST is another code path in Pillow), "
                         f"got {resample!r}")
    single = t.dim() == 3
    if single:
        t = t[None]
    b, H, W, _ = t.shape
    w, h = int(size[0]), int(size[1])
    if w <= 0 or h <= 0:
        raise ValueError(f"pil_resize: size must be positive, got {size}")
    bx = (0.0, 0.0, float(W), float(H)) if box is None else tuple(float(v) for v in box)
    if len(bx) != 4 or bx[0] < 0 or bx[1] < 0 or bx[2] > W or bx[3] > H or bx[2] <= bx[0] or bx[3] <= bx[1]:
        raise ValueError(f"pil_resize: box {box} is empty or leaves the {W} x {H} image")
    x0, y0, x1, y1 = (0, 0, w, h) if window is None else (int(v) for v in window)
    if not (0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h):
        raise ValueError(f"pil_resize: window {window} is empty or leaves the {w} x {h} output")
    ww, wh = x1 - x0, y1 - y0
    if out is None:
        out = torch.empty(b, wh, ww, 3, device=t.device, dtype=torch.uint8)
        res = out[0] if single else out
    else:
        want = (wh, ww, 3) if single else (b, wh, ww, 3)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != want:
            got = f"{tuple(out.shape)} {out.dtype}" if isinstance(out, torch.Tensor) else type(out).__name__
            raise ValueError(f"pil_resize: out must be uint8 {want}, got {got}")
        if out.device != t.device or not out.is_contiguous():
            raise RuntimeError("pil_resize: out must be a contiguous tensor on the images' device")
        res = out

    hor, ver = passes((W, H), (w, h), bx)
    ax = _axis(t.device, W, w, resample, bx[0], bx[2], hor)
    ay = _axis(t.device, H, h, resample, bx[1], bx[3], ver)
    tx, rh, span = _tile(ax, ww)
    st = stream()
    if not ver:                                      # rows pass through: the horizontal pass (or its identity) writes the result
        call("e4s_pil_resample_h_u8", ptr(t), b, H, W, ptr(ax.bounds), ptr(ax.kk), ax.ksize, w, x0, x1, y0, wh, ptr(out), ww * 3,
             wh * ww * 3, tx, rh, span, st)
        return res
    # the input rows the window's vertical pass reads, resampled horizontally (or copied) into a workspace of 16-byte row pitch
    ry0 = int(ay.bounds_host[y0, 0])
    ry1 = int(ay.bounds_host[y1 - 1, 0] + ay.bounds_host[y1 - 1, 1])
    rows, pitch = ry1 - ry0, (ww * 3 + 15) // 16 * 16
    ws = torch.empty(b, rows, pitch, device=t.device, dtype=torch.uint8)
    call("e4s_pil_resample_h_u8", ptr(t), b, H, W, ptr(ax.bounds), ptr(ax.kk), ax.ksize, w, x0, x1, ry0, rows, ptr(ws), pitch,
         rows * pitch, tx, rh, span, st)
    call("e4s_pil_resample_v_u8", ptr(ws), pitch, b, rows, ry0, ptr(ay.bounds), ptr(ay.kk), ay.ksize, h, y0, y1, ww * 3, ptr(out), st)
    return res
