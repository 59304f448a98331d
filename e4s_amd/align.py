"""Frame I/O of the face swap on the device: the aligned crop of a face out of a frame (step (1) of scripts/face_swap.py,
`crop_and_align_face` -> src/utils/alignmengt.py: crop_image) and the paste of the swapped face back into the frame (the last block
of step (6), scripts/face_swap.py:313-327) as HIP kernels (e4s_amd/csrc/align.hip) on uint8 HWC device tensors.  With them a frame
goes up once and the swapped frame comes down once; `paste_back` continues `postproc.stitch`.

Pillow's QUAD / PERSPECTIVE transforms with the BILINEAR filter are restated in fp64 in Pillow's operation order, so the kernels
reproduce `Image.transform` level for level (tests/test_gpu_align.py holds a numpy statement of the same arithmetic that is
bit-identical to live Pillow).  The small host-side geometry (`compute_quad`, `calc_alignment_coefficients`, `crop_window`,
`quad_coefficients`) is float64 numpy with the reference's formulas; function names and argument meaning follow the reference's.

Out of scope:
  * landmark detection (dlib / face_alignment): the feature starts from 68 landmarks or from a quad, as crop_faces_by_quads does;
  * crop_image's `enable_padding` branch (the pipeline never passes it): NotImplementedError.  Its `shrink` branch (a quad diagonal
    of 4 x size or more) is opt-in, `crop_faces_by_quads(shrink=True)`: the frame is resized with LANCZOS (Image.ANTIALIAS under its
    old name, which current Pillow no longer has) by `resize.pil_resize`; `crop_window` itself keeps refusing it;
  * paste_image_mask with a soft alpha (face_swap.py:52-72): Pillow warps RGBA premultiplied there, a different arithmetic, and the
    pipeline never calls it;
  * the `src/` overlay: `src.utils.alignmengt` keeps executing the reference module in place."""
import numpy as np
import torch

from . import resize
from .lib import call, fptr, ptr, stream


# ---- host geometry (float64) ---------------------------------------------------------------------------------------------
def compute_quad(lm68, scale=1.0):
    """src/utils/alignmengt.py:146-176 compute_transform on given landmarks plus the quad stacking of crop_faces (:209):
    lm68 [68,2] or [B,68,2] -> quad [4,2] or [B,4,2] (float64; corners nw, sw, se, ne as (x, y))."""
    lm = np.asarray(lm68, dtype=np.float64)
    if lm.ndim == 3:
        return np.stack([compute_quad(one, scale) for one in lm])
    if lm.shape != (68, 2):
        raise ValueError(f"compute_quad expects [68,2] or [B,68,2] landmarks, got {lm.shape}")
    c, x, y = _transform(lm, scale)
    return np.stack([c - x - y, c - x + y, c + x + y, c + x - y])


def _transform(lm, scale):
    """compute_transform's (c, x, y) of one [68,2] float64 landmark set."""
    eye_left = np.mean(lm[36:42], axis=0)
    eye_right = np.mean(lm[42:48], axis=0)
    eye_avg = (eye_left + eye_right) * 0.5
    eye_to_eye = eye_right - eye_left
    mouth_avg = (lm[48] + lm[54]) * 0.5
    eye_to_mouth = mouth_avg - eye_avg
    x = eye_to_eye - np.flipud(eye_to_mouth) * [-1, 1]
    x /= np.hypot(*x)
    x *= max(np.hypot(*eye_to_eye) * 2.0, np.hypot(*eye_to_mouth) * 1.8)
    x *= scale
    y = np.flipud(x) * [-1, 1]
    c = eye_avg + eye_to_mouth * 0.1
    return c, x, y


def gaussian_filter1d(a, sigma):
    """scipy.ndimage.gaussian_filter1d(a, sigma, axis=0) with its defaults, in numpy: radius int(4 sigma + 0.5), taps
    exp(-0.5 i^2 / sigma^2) normalised, boundary 'reflect' (d c b a | a b c d | d c b a, repeated as often as the radius needs);
    summed as scipy's symmetric correlation does, the centre first and then the pairs from the outside in."""
    a = np.asarray(a, dtype=np.float64)
    sigma = float(sigma)
    r = int(4.0 * sigma + 0.5)
    i = np.arange(-r, r + 1)
    taps = np.exp(-0.5 / (sigma * sigma) * i ** 2)
    taps = taps / taps.sum()
    n = a.shape[0]
    p = np.pad(a, [(r, r)] + [(0, 0)] * (a.ndim - 1), mode="symmetric")
    out = p[r:r + n] * taps[r]
    for j in range(-r, 0):
        out = out + (p[r + j:r + j + n] + p[r - j:r - j + n]) * taps[j + r]
    return out


def compute_quads(lm68, scale=1.0, center_sigma=0.0, xy_sigma=0.0):
    """src/utils/alignmengt.py:191-210, crop_faces on given landmarks: lm68 [N,68,2] of N consecutive frames -> quads [N,4,2]
    (float64), the centres smoothed over the frame axis with center_sigma and the half-axes with xy_sigma where that sigma is not
    0.  With both 0 it is `compute_quad` of every frame."""
    lm = np.asarray(lm68, dtype=np.float64)
    if lm.ndim != 3 or lm.shape[1:] != (68, 2) or len(lm) == 0:
        raise ValueError(f"compute_quads expects [N,68,2] landmarks, got {lm.shape}")
    cs, xs, ys = (np.stack(v) for v in zip(*(_transform(one, scale) for one in lm)))
    if center_sigma != 0:
        cs = gaussian_filter1d(cs, center_sigma)
    if xy_sigma != 0:
        xs = gaussian_filter1d(xs, xy_sigma)
        ys = gaussian_filter1d(ys, xy_sigma)
    return np.stack([cs - xs - ys, cs - xs + ys, cs + xs + ys, cs + xs - ys], axis=1)


def calc_alignment_coefficients(pa, pb):
    """src/utils/alignmengt.py:228-238: the 8 PERSPECTIVE coefficients that map the points pa onto pb, by the reference's normal
    equations inv(A^T A) A^T b (in this order: the system is ill-conditioned and the order is part of the result)."""
    matrix = []
    for p1, p2 in zip(pa, pb):
        matrix.append([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]])
        matrix.append([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]])
    a = np.array(matrix, dtype=np.float64)
    b = np.array(pb, dtype=np.float64).reshape(8)
    return np.dot(np.linalg.inv(a.T @ a) @ a.T, b).reshape(8)


def quad_coefficients(quad, size):
    """The 8 numbers Pillow's QUAD transform derives from the quad it is handed (corners nw, sw, se, ne; Image.py __transformer):
    source = (a0 + a1 x + a2 y + a3 x y, a4 + a5 x + a6 y + a7 x y) for the output point (x, y) of a size x size image."""
    q = np.asarray(quad, dtype=np.float64).reshape(4, 2)
    nw, sw, se, ne = q
    As = At = 1.0 / size
    return np.array([nw[0], (ne[0] - nw[0]) * As, (sw[0] - nw[0]) * At, (se[0] - sw[0] - ne[0] + nw[0]) * As * At,
                     nw[1], (ne[1] - nw[1]) * As, (sw[1] - nw[1]) * At, (se[1] - sw[1] - ne[1] + nw[1]) * As * At])


def crop_window(quad, frame_hw, size=1024, enable_padding=False):
    """src/utils/alignmengt.py:97-121: the integer window (x0, y0, x1, y1) crop_image cuts out of an H x W frame before it
    transforms (the quad's bounding box plus a border of a tenth of its diagonal, clipped to the frame), or the whole frame
    (0, 0, W, H) where the reference does not crop."""
    if enable_padding:
        raise NotImplementedError("crop_image(enable_padding=True) is not implemented (the pipeline never passes it)")
    quad = np.asarray(quad, dtype=np.float64).reshape(4, 2)
    h, w = int(frame_hw[0]), int(frame_hw[1])
    x = (quad[3] - quad[1]) / 2
    qsize = np.hypot(*x) * 2
    shrink = int(np.floor(qsize / size * 0.5))
    if shrink > 1:
        raise NotImplementedError(f"quad diagonal {qsize:.1f} >= 4 x size {size}: crop_image's shrink branch (Image.ANTIALIAS) is not "
                                  "implemented")
    border = max(int(np.rint(qsize * 0.1)), 3)
    crop = (int(np.floor(min(quad[:, 0]))), int(np.floor(min(quad[:, 1]))), int(np.ceil(max(quad[:, 0]))),
            int(np.ceil(max(quad[:, 1]))))
    crop = (max(crop[0] - border, 0), max(crop[1] - border, 0), min(crop[2] + border, w), min(crop[3] + border, h))
    if crop[2] <= crop[0] or crop[3] <= crop[1]:
        raise ValueError(f"the quad lies outside the {w} x {h} frame")
    if crop[2] - crop[0] < w or crop[3] - crop[1] < h:
        return crop
    return (0, 0, w, h)


def crop_plan(quad, frame_hw, size=1024):
    """crop_image up to its transform, shrink branch included (src/utils/alignmengt.py:97-121), for one quad in an H x W frame ->
    (shrink, rsize, window, quad_in_window): shrink = floor(qsize / size * 0.5); above 1 the frame is resized to rsize = (width,
    height) = rint(W / shrink), rint(H / shrink) with LANCZOS and the quad divided by shrink; window = (x0, y0, x1, y1) is what is
    cut out of that (shrunk) frame, as `crop_window` finds it; quad_in_window is the (shrunk) quad relative to the window's origin
    (Pillow gets it + 0.5).  With shrink <= 1, rsize is (W, H) and nothing is resized."""
    quad = np.array(quad, dtype=np.float64).reshape(4, 2)
    h, w = int(frame_hw[0]), int(frame_hw[1])
    qsize = np.hypot(*((quad[3] - quad[1]) / 2)) * 2
    shrink = int(np.floor(qsize / size * 0.5))
    rsize = (w, h)
    if shrink > 1:
        rsize = (int(np.rint(float(w) / shrink)), int(np.rint(float(h) / shrink)))
        quad /= shrink
    window = crop_window(quad, (rsize[1], rsize[0]), size)          # (q / floor(q) < 2: the shrunk quad is below the threshold)
    return shrink, rsize, window, quad - np.array(window[:2], dtype=np.float64)


def crop_parameters(quads, frame_hw, size=1024):
    """What `crop_faces_by_coeffs` takes, for quads as the reference passes them: (QUAD coefficients float64 [B,8] of
    quad - window origin + 0.5, windows int32 [B,4]) as numpy arrays."""
    quads = _quads(quads)
    coeffs, windows = np.empty((len(quads), 8)), np.empty((len(quads), 4), dtype=np.int32)
    for i, quad in enumerate(quads):
        win = crop_window(quad, frame_hw, size)
        windows[i] = win
        coeffs[i] = quad_coefficients(quad - np.array(win[:2], dtype=np.float64) + 0.5, size)
    return coeffs, windows


def paste_parameters(quads, size=1024):
    """scripts/face_swap.py:110-113 `inv_transforms`: PERSPECTIVE coefficients float64 [B,8] that take a frame point to its place in
    the size x size face, for `paste_back_by_coeffs`."""
    dst = [[0, 0], [0, size], [size, size], [size, 0]]
    return np.stack([calc_alignment_coefficients(quad + 0.5, dst) for quad in _quads(quads)])


def _quads(quads):
    q = np.asarray(quads.detach().cpu().numpy() if isinstance(quads, torch.Tensor) else quads, dtype=np.float64)
    if q.ndim == 2:
        q = q[None]
    if q.ndim != 3 or q.shape[1:] != (4, 2):
        raise RuntimeError(f"quads must be [B,4,2] (or one [4,2]), got {q.shape}")
    return q


# ---- device side ---------------------------------------------------------------------------------------------------------
def _images(t, what):
    if t.dtype != torch.uint8:
        raise RuntimeError(f"{what} must be uint8, got {t.dtype}")
    if t.dim() != 4 or t.shape[-1] != 3:
        raise RuntimeError(f"{what} must be HWC images [B,H,W,3], got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{what} must be contiguous")
    return t


def _table(t, b, cols, dtype, what):
    if t.dtype != dtype or tuple(t.shape) != (b, cols) or not t.is_contiguous():
        raise RuntimeError(f"{what} must be a contiguous {dtype} [{b},{cols}] tensor, got {t.dtype} {tuple(t.shape)}")
    return t


def _to_device(a, dtype, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def crop_faces_by_coeffs(frames_u8, coeffs, windows, size=1024, normalized=False, out=None, out_normalized=None):
    """The crop with ready device tensors (see `crop_parameters`): coeffs float64 [B,8], windows int32 [B,4].  Nothing is read on
    the host, so a captured graph replays with whatever the two tensors hold then.  `out` / `out_normalized`: write there."""
    frames = _images(frames_u8, "frames")
    b, h, w, _ = frames.shape
    _table(coeffs, b, 8, torch.float64, "coeffs")
    _table(windows, b, 4, torch.int32, "windows")
    if out is None:
        out = torch.empty(b, size, size, 3, device=frames.device, dtype=torch.uint8)
    elif _images(out, "out").shape != (b, size, size, 3):
        raise RuntimeError(f"out must be [{b},{size},{size},3], got {tuple(out.shape)}")
    norm = None
    if normalized or out_normalized is not None:
        norm = out_normalized if out_normalized is not None else torch.empty(b, 3, size, size, device=frames.device)
        if tuple(norm.shape) != (b, 3, size, size):
            raise RuntimeError(f"out_normalized must be [{b},3,{size},{size}], got {tuple(norm.shape)}")
    call("e4s_quad_crop_u8", ptr(frames), ptr(coeffs), ptr(windows), ptr(out), fptr(norm), b, h, w, size, stream())
    return (out, norm) if norm is not None else out


def crop_faces_by_quads(frames_u8, quads, size=1024, normalized=False, shrink=False, taps=None):
    """src/utils/alignmengt.py:217-225 for frames on the device: frames uint8 [B,H,W,3], quads [B,4,2] as the reference passes them
    (the + 0.5 is applied inside) -> aligned faces uint8 [B,size,size,3]; normalized=True: also the encoder's input, fp32
    [B,3,size,size] = (face / 255 - 0.5) / 0.5 (the reference's ToTensor + Normalize), written in the same pass.
    shrink=True: a quad whose diagonal is 4 x size or more takes crop_image's shrink branch (`crop_plan`) where the default
    refuses it: only the crop window of the LANCZOS-shrunk frame is made (`resize.pil_resize(window=...)`) and the crop kernel reads
    that buffer.  taps: a dict that receives taps['shrunk'] = [(index, shrink, window, the uint8 [h,w,3] window), ...]."""
    frames = _images(frames_u8, "frames")
    quads = _quads(quads)
    if len(quads) != frames.shape[0]:
        raise RuntimeError(f"{len(quads)} quads for {frames.shape[0]} frames")
    dev = frames.device
    plans = [crop_plan(q, frames.shape[1:3], size) for q in quads] if shrink else []
    if not any(p[0] > 1 for p in plans):
        coeffs, windows = crop_parameters(quads, frames.shape[1:3], size)
        return crop_faces_by_coeffs(frames, _to_device(coeffs, torch.float64, dev), _to_device(windows, torch.int32, dev), size, normalized)
    # faces of one call may shrink differently: one crop launch per face (a handful at most), each on its own frame or window
    b = len(quads)
    out = torch.empty(b, size, size, 3, device=dev, dtype=torch.uint8)
    norm = torch.empty(b, 3, size, size, device=dev) if normalized else None
    for i, (factor, rsize, win, quad) in enumerate(plans):
        image, origin = frames[i:i + 1], win
        if factor > 1:
            image = resize.pil_resize(frames[i:i + 1], rsize, resize.LANCZOS, window=win)
            origin = (0, 0, win[2] - win[0], win[3] - win[1])
            if taps is not None:
                taps.setdefault("shrunk", []).append((i, factor, win, image[0]))
        coeffs = quad_coefficients(quad + 0.5, size)[None]
        crop_faces_by_coeffs(image, _to_device(coeffs, torch.float64, dev), _to_device(np.array([origin]), torch.int32, dev), size,
                             out=out[i:i + 1], out_normalized=None if norm is None else norm[i:i + 1])
    return (out, norm) if norm is not None else out


def paste_back_by_coeffs(faces_u8, frames_u8, coeffs, out=None):
    """The paste with a ready device tensor (see `paste_parameters`): coeffs float64 [B,8]; graph-capturable as the crop is."""
    faces, frames = _images(faces_u8, "faces"), _images(frames_u8, "frames")
    b, h, w, _ = frames.shape
    s = faces.shape[1]
    if faces.shape[0] != b or faces.shape[2] != s:
        raise RuntimeError(f"faces must be [{b},S,S,3] for {b} frames, got {tuple(faces.shape)}")
    _table(coeffs, b, 8, torch.float64, "coeffs")
    if out is None:
        out = torch.empty_like(frames)
    elif _images(out, "out").shape != frames.shape:
        raise RuntimeError(f"out must be {tuple(frames.shape)}, got {tuple(out.shape)}")
    elif out.data_ptr() != frames.data_ptr() and out.untyped_storage().data_ptr() == frames.untyped_storage().data_ptr():
        raise RuntimeError("out must be the frames tensor itself or a tensor of its own, not another view of its storage")
    call("e4s_perspective_paste_u8", ptr(faces), ptr(frames), ptr(coeffs), ptr(out), b, h, w, s, stream())
    return out


def paste_back(faces_u8, frames_u8, quads, size=None, out=None):
    """scripts/face_swap.py:313-327 for a batch on the device: faces uint8 [B,S,S,3] are projected into frames uint8 [B,H,W,3] by
    the inverse transforms of their quads (face_swap.py:110-113); pixels the face does not cover keep the frame's value.
    `size`: the side the quads were cropped at (default: the faces' own).  out=frames_u8 pastes in place."""
    faces = _images(faces_u8, "faces")
    quads = _quads(quads)
    if len(quads) != faces.shape[0]:
        raise RuntimeError(f"{len(quads)} quads for {faces.shape[0]} faces")
    if size is not None and size != faces.shape[1]:
        raise RuntimeError(f"faces are {faces.shape[1]} pixels wide, the quads were cropped at {size}")
    coeffs = paste_parameters(quads, faces.shape[1])
    return paste_back_by_coeffs(faces, frames_u8, _to_device(coeffs, torch.float64, faces.device), out)


def swap_into_frames(stitched_u8, frames_u8, quads, out=None):
    """The continuation of `postproc.stitch`: its stitched uint8 [B,1024,1024,3] faces go back into the frames their targets were
    cropped from with `crop_faces_by_quads(frames_u8, quads)`."""
    return paste_back(stitched_u8, frames_u8, quads, out=out)
