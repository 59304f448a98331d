"""numpy restatements of the OpenCV steps of face_enhancement.py:44-49,68-108 (cv2 itself is not available): the yardsticks of
tests/test_face_paste_host.py and tests/test_gpu_face_paste.py.  warp_affine follows imgwarp.cpp's fixed-point algorithm literally."""
import numpy as np


def invert(M):
    m = np.asarray(M, dtype=np.float64).reshape(6).copy()
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = a11, m[1] * -D, m[3] * -D, a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    return np.array([m[0], m[1], b1, m[3], m[4], b2])


def warp_affine(src, M, dsize, inverse=False):
    """cv2.warpAffine(src, M, dsize=(w, h), flags=INTER_LINEAR [| WARP_INVERSE_MAP]), constant border 0; uint8 [H,W,C] or fp32 [H,W]."""
    a = np.asarray(M, dtype=np.float64).reshape(6) if inverse else invert(M)
    wd, hd = dsize
    hs, ws = src.shape[:2]
    x, y = np.arange(wd, dtype=np.float64), np.arange(hd, dtype=np.float64)
    adelta, bdelta = np.rint(a[0] * x * 1024.0).astype(np.int64), np.rint(a[3] * x * 1024.0).astype(np.int64)
    X0, Y0 = np.rint((a[1] * y + a[2]) * 1024.0).astype(np.int64) + 16, np.rint((a[4] * y + a[5]) * 1024.0).astype(np.int64) + 16
    X, Y = (X0[:, None] + adelta[None, :]) >> 5, (Y0[:, None] + bdelta[None, :]) >> 5
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < hs) & (xx >= 0) & (xx < ws)
        v = src[np.clip(yy, 0, hs - 1), np.clip(xx, 0, ws - 1)]
        return np.where(ok[..., None] if src.ndim == 3 else ok, v, 0)

    p = [tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)]
    if src.dtype == np.uint8:
        w = [(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32]
        acc = sum(wi[..., None] * pi.astype(np.int64) for wi, pi in zip(w, p))
        return ((acc + 16384) >> 15).astype(np.uint8)
    one = np.float32(1)
    cx1, cy1 = fx.astype(np.float32) * np.float32(1 / 32), fy.astype(np.float32) * np.float32(1 / 32)
    cx0, cy0 = one - cx1, one - cy1
    w = [cy0 * cx0, cy0 * cx1, cy1 * cx0, cy1 * cx1]
    out = p[0].astype(np.float32) * w[0]
    for k in (1, 2, 3):
        out = out + p[k].astype(np.float32) * w[k]
    return out.astype(np.float32)


def reflect101(i, n):
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    while ((i < 0) | (i >= n)).any():
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)
    return i


def blur64(x, taps):
    """One GaussianBlur in fp64 with the given (float) taps: rows, then columns, BORDER_REFLECT_101."""
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(taps, dtype=np.float64)
    r = len(t) // 2
    h, w = x.shape
    rows = sum(t[k] * x[:, reflect101(np.arange(w) + k - r, w)] for k in range(len(t)))
    return sum(t[k] * rows[reflect101(np.arange(h) + k - r, h), :] for k in range(len(t)))


def mask_postprocess64(mask_u8, taps, thres=20):
    m = mask_u8.astype(np.float32) / np.float32(255)
    m[:thres, :] = 0
    m[-thres:, :] = 0
    m[:, :thres] = 0
    m[:, -thres:] = 0
    return blur64(blur64(m, taps), taps)


def binomial3(img):
    """cv2.filter2D(img, -1, [1 2 1] x [1 2 1] / 16) on uint8 [H,W,C]: exact sum, round half to even."""
    h, w = img.shape[:2]
    k = [1, 2, 1]
    s = np.zeros(img.shape, dtype=np.int64)
    for dy in (-1, 0, 1):
        yy = reflect101(np.arange(h) + dy, h)
        for dx in (-1, 0, 1):
            xx = reflect101(np.arange(w) + dx, w)
            s += k[dy + 1] * k[dx + 1] * img[yy][:, xx].astype(np.int64)
    return np.rint(s / 16.0).astype(np.uint8)


def merge_blend64(masks, faces, bg):
    """face_enhancement.py:100-108 in fp64: masks [n,H,W] (fp64), faces uint8 [n,H,W,3], bg uint8 [H,W,3] -> fp64 levels before rounding
    and the index of the face that owns each pixel (-1: none)."""
    h, w = bg.shape[:2]
    full_mask, full_img, who = np.zeros((h, w)), np.zeros((h, w, 3)), -np.ones((h, w), dtype=np.int64)
    for f in range(len(masks)):
        take = masks[f] - full_mask > 0
        full_mask[take], full_img[take], who[take] = masks[f][take], faces[f][take], f
    m = full_mask[..., None]
    return np.abs(bg.astype(np.float64) * (1 - m) + full_img * m), who
