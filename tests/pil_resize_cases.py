"""Shared by tests/test_pil_resize_host.py, tests/test_gpu_pil_resize.py and tests/test_gpu_any_size.py (not a test module): a plain
restatement of Pillow's 8-bit resample (libImaging/Resample.c), written with scalar Python arithmetic and independent of
e4s_amd/resize.py, the list of cases, live Pillow's answer, and crop_image with its shrink branch on live Pillow.

Per axis (input length inSize, box [in0, in1), output length outSize, filter f of support s):
  scale = (in1 - in0) / outSize, filterscale = max(scale, 1), support = s * filterscale, ksize = int(ceil(support)) * 2 + 1;
  for the output index xx: center = in0 + (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0),
  xmax = min(int(center + support + 0.5), inSize) - xmin, k[x] = f((x + xmin - center + 0.5) * (1 / filterscale)) for x < xmax,
  divided by their left-to-right sum if it is not 0; kk[x] = int(k[x] * 2^22 -+ 0.5), truncating (- for negative k).
Passes: horizontal (iff w != W or box[0] != 0 or box[2] != W) into a uint8 image, then vertical (same rule);
  value = clamp((2^21 + sum_x pixel[xmin + x] * kk[x]) >> 22, 0, 255), the shift arithmetic."""
import math

import numpy as np
from PIL import Image

import align_cases as ac

NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = (Image.Resampling.NEAREST, Image.Resampling.LANCZOS, Image.Resampling.BILINEAR,
                                                     Image.Resampling.BICUBIC, Image.Resampling.BOX, Image.Resampling.HAMMING)
FILTERS = (BOX, BILINEAR, HAMMING, BICUBIC, LANCZOS)

# (name, (W, H) of the input, (w, h) of the output)
CASES = (("up", (37, 53), (64, 64)), ("down", (64, 64), (23, 17)), ("y_only", (100, 75), (100, 40)), ("x_only", (75, 100), (40, 100)),
         ("binary", (16, 16), (64, 64)), ("down4", (130, 97), (32, 32)), ("tiny", (5, 7), (3, 11)), ("identity", (64, 48), (64, 48)))
RAGGED = (((300, 500), (257, 129)), ((129, 257), (500, 300)))                # several tiles, no multiple of any of them


def fractional_box(W, H):
    return (1.25, 2.5, W - 0.75, H - 1.5)


def image(name, W, H, seed=0):
    """uint8 [H,W,3]; 'binary' is made of 0 and 255 only, where the negative lobes of BICUBIC and LANCZOS overshoot."""
    rng = np.random.default_rng([seed, W, H])
    if name == "binary":
        return (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    return ac.frames(1, H, W, seed=seed + 7 * W + H)[0]


def pillow(img, size, resample, box=None):
    return np.asarray(Image.fromarray(img).resize(size, resample, box=box))


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


SUPPORT = {BOX: (_box, 0.5), BILINEAR: (_bilinear, 1.0), HAMMING: (_hamming, 1.0), BICUBIC: (_bicubic, 2.0), LANCZOS: (_lanczos, 3.0)}


def coefficients(in_size, out_size, resample, in0, in1):
    """-> (bounds int64 [out,2], kk int64 [out,ksize])."""
    f, s = SUPPORT[resample]
    scale = (in1 - in0) / out_size
    filterscale = max(scale, 1.0)
    support = s * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds, kk = np.zeros((out_size, 2), dtype=np.int64), np.zeros((out_size, ksize), dtype=np.int64)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k, ww = [], 0.0
        for x in range(xmax):
            w = f((x + xmin - center + 0.5) * ss)
            k.append(w)
            ww += w
        for x in range(xmax):
            v = k[x] / ww if ww != 0.0 else k[x]
            kk[xx, x] = int(v * (1 << 22) - 0.5) if v < 0 else int(v * (1 << 22) + 0.5)
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pass(img, bounds, kk):
    """Resample axis 0 of a uint8 array."""
    src = img.astype(np.int64)
    out = np.empty((len(bounds),) + img.shape[1:], dtype=np.uint8)
    for i, (lo, n) in enumerate(bounds):
        acc = (1 << 21) + np.tensordot(kk[i, :n], src[lo:lo + n], axes=(0, 0))
        out[i] = np.clip(acc >> 22, 0, 255)
    return out


def passes(in_wh, size, box=None):
    (W, H), (w, h) = in_wh, size
    x0, y0, x1, y1 = (0, 0, W, H) if box is None else box
    return (w != W or x0 != 0 or x1 != W), (h != H or y0 != 0 or y1 != H)


def resize(img, size, resample, box=None):
    """The restatement of Image.fromarray(img).resize(size, resample, box=box) for a uint8 [H,W,3] array."""
    H, W = img.shape[:2]
    x0, y0, x1, y1 = (0.0, 0.0, float(W), float(H)) if box is None else box
    hor, ver = passes((W, H), size, box)
    out = img
    if hor:
        out = _pass(out.transpose(1, 0, 2), *coefficients(W, size[0], resample, x0, x1)).transpose(1, 0, 2)
    if ver:
        out = _pass(out, *coefficients(H, size[1], resample, y0, y1))
    return np.ascontiguousarray(out)


# ---- crop_image with its shrink branch (src/utils/alignmengt.py:97-140), on live Pillow ---------------------------------
def crop_plan(quad, frame_hw, size):
    """-> (shrink, rsize, window in the shrunk frame, the shrunk quad relative to the window's origin)."""
    quad = np.array(quad, dtype=np.float64)
    H, W = frame_hw
    qsize = np.hypot(*((quad[3] - quad[1]) / 2)) * 2
    shrink = int(np.floor(qsize / size * 0.5))
    rsize = (W, H)
    if shrink > 1:
        rsize = (int(np.rint(float(W) / shrink)), int(np.rint(float(H) / shrink)))
        quad /= shrink
    win = ac.reference_window(quad, (rsize[1], rsize[0]))
    return shrink, rsize, tuple(int(v) for v in win), quad - np.array(win[:2], dtype=np.float64)


def pil_shrink_crop(frame, quad, size):
    """crop_image on a uint8 [H,W,3] frame -> (the face uint8 [size,size,3], the cropped window of the (shrunk) frame)."""
    shrink, rsize, win, q = crop_plan(quad, frame.shape[:2], size)
    img = Image.fromarray(frame)
    if shrink > 1:
        img = img.resize(rsize, LANCZOS)                      # Image.ANTIALIAS was LANCZOS' old name
    sub = img.crop(win)
    return np.array(sub.transform((size, size), Image.QUAD, (q + 0.5).flatten(), Image.BILINEAR)), np.array(sub)


SHRINK_HW, SHRINK_S = (400, 600), 64
R2 = np.sqrt(2.0) * SHRINK_S                  # the half-side at which the diagonal is 4 x size: shrink goes from 1 to 2
# shrink = floor(half-side * sqrt(2) / size): 1 (just below the threshold), 2 (just above it), 3 (half-side 2.2 x size) and 4
# (half-side 3 x size, which reaches beyond the frame), each turned a little
SHRINK_QUADS = np.stack([ac.square((300.3, 200.6), R2 - 0.5, 10.0), ac.square((310.7, 190.2), R2 + 0.5, -20.0),
                         ac.square((295.1, 205.3), 2.2 * SHRINK_S, 33.0), ac.square((290.4, 210.9), 3.0 * SHRINK_S, 5.0)])
SHRINKS = (1, 2, 3, 4)
