"""Restored faces back into the frame, on the device: FaceEnhancement.process(aligned=False), face_enhancement.py:68-110.

Once a detector has produced boxes and five landmarks per face, the frame stays on the device until the blended frame is done.  The
detector is e4s_amd.retinaface.RetinaFaceDetection (FaceRestorer(detector=...) calls it when process gets no boxes):

    reference (per face)                                             here
    ---------------------------------------------------------------  ---------------------------------------------------------
    get_reference_facial_points((s, s), 0.25, (0, 0), True)          reference_5pts(s)                      (host, float64)
    _umeyama(src, ref), _umeyama(ref, src, False, 1 / scale)         similarity_transform(pts5, ref)        (host, float64)
    cv2.warpAffine(img, tfm, (s, s), flags=3)                        warp_affine (e4s_warp_affine)
    self.facegan.process(of)                                         restore(faces_u8)   (any callable; gpen_restore(generator))
    self.faceparser.process(ef)[0] / 255.                            parser.masks(ef)    (e4s_amd.parsenet.FaceParse)
    mask_postprocess: 20-pixel frame, two GaussianBlur(101, 11)      mask_postprocess (e4s_mask_prep_f32, e4s_blur_pass_f32 x 4)
    cv2.filter2D(ef, -1, kernel) for small faces                     smooth_small_face (e4s_binomial3_u8)
    cv2.warpAffine(tmp_mask / ef, tfm_inv, (width, height), flags=3) warp_affine
    mask > full_mask merge, convertScaleAbs(bg (1 - m) + face m)     merge_and_blend (e4s_merge_blend_u8, one launch per frame)

cv2 is not a dependency.  warp_affine, the Gaussian blur and the 3x3 filter restate OpenCV's published algorithms (imgwarp.cpp's
fixed-point coordinate grid and weights, getGaussianKernel's formula, BORDER_REFLECT_101); they are cross-checked against
scipy.ndimage and fp64 restatements in the tests, not against cv2 itself.  Two deliberate differences from the reference's call:
the mask is blurred in fp32 (the reference hands GaussianBlur a float64 array), and the landmark arithmetic is float64 (the
reference rounds the points to float32 first).  The resize of the frame to the SR size, align types other than similarity and
in_size != out_size stay outside."""
import numpy as np
import torch

from . import kernels as K

REFERENCE_FACIAL_POINTS = [[30.29459953, 51.69630051], [65.53179932, 51.50139999], [48.02519989, 71.73660278],
                           [33.54930115, 92.3655014], [62.72990036, 92.20410156]]                  # align_faces.py:14-20
DEFAULT_CROP_SIZE = (96, 112)


def reference_5pts(in_size):
    """get_reference_facial_points((in_size, in_size), 0.25, (0, 0), True) (align_faces.py:102-184): float64 [5,2] (x, y)."""
    pts = np.array(REFERENCE_FACIAL_POINTS, dtype=np.float64)
    crop = np.array(DEFAULT_CROP_SIZE, dtype=np.int64)
    size_diff = crop.max() - crop                                           # default_square
    pts = pts + size_diff / 2
    crop = crop + size_diff
    inner = 0.25
    size_diff = crop * inner * 2
    pts = pts + size_diff / 2
    crop = crop + np.round(size_diff).astype(np.int32)
    if in_size * crop[1] != in_size * crop[0]:
        raise ValueError("reference_5pts: a square crop")
    return pts * (float(in_size) / crop[0])


def _umeyama(src, dst, estimate_scale=True, scale=1.0):
    """align_faces.py:25-95 (skimage's similarity estimate) for 2-D points in float64."""
    num, dim = src.shape
    src_mean, dst_mean = src.mean(axis=0), dst.mean(axis=0)
    src_demean, dst_demean = src - src_mean, dst - dst_mean
    A = dst_demean.T @ src_demean / num
    d = np.ones((dim,), dtype=np.double)
    if np.linalg.det(A) < 0:
        d[dim - 1] = -1
    T = np.eye(dim + 1, dtype=np.double)
    U, S, V = np.linalg.svd(A)
    rank = np.linalg.matrix_rank(A)
    if rank == 0:
        raise ValueError("similarity_transform: degenerate landmarks")
    if rank == dim - 1:
        if np.linalg.det(U) * np.linalg.det(V) > 0:
            T[:dim, :dim] = U @ V
        else:
            s = d[dim - 1]
            d[dim - 1] = -1
            T[:dim, :dim] = U @ np.diag(d) @ V
            d[dim - 1] = s
    else:
        T[:dim, :dim] = U @ np.diag(d) @ V
    if estimate_scale:
        scale = 1.0 / src_demean.var(axis=0).sum() * (S @ d)
    T[:dim, dim] = dst_mean - scale * (T[:dim, :dim] @ src_mean.T)
    T[:dim, :dim] *= scale
    return T, scale


def similarity_transform(pts5, ref):
    """(tfm, tfm_inv), float64 [2,3] each: warp_and_crop_face's similarity branch (align_faces.py:258-262).  pts5, ref: [5,2] or
    [2,5] landmark arrays (x, y)."""
    src, dst = np.asarray(pts5, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    src = src.T if src.shape[0] == 2 else src
    dst = dst.T if dst.shape[0] == 2 else dst
    if src.shape != dst.shape or src.ndim != 2 or src.shape[1] != 2 or src.shape[0] < 3:
        raise ValueError("similarity_transform: two [K,2] point sets, K > 2")
    params, scale = _umeyama(src, dst)
    inv, _ = _umeyama(dst, src, False, scale=1.0 / scale)
    return params[:2, :].copy(), inv[:2, :].copy()


def invert_affine(M):
    """The destination -> source map cv2.warpAffine derives from M (imgwarp.cpp: in double, in this order of operations)."""
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = a11, m[1] * -D, m[3] * -D, a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    return [m[0], m[1], b1, m[3], m[4], b2]


def warp_affine(src, M, dsize, inverse=False):
    """cv2.warpAffine(src, M, dsize=(width, height), flags=3 [| WARP_INVERSE_MAP with inverse]) with the constant border 0: src a
    device uint8 [H,W,3] or fp32 [H,W] image."""
    if not src.is_cuda:
        raise RuntimeError("warp_affine runs on the ROCm device only (no CPU path)")
    coef = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)] if inverse else invert_affine(M)
    return K.warp_affine(src, coef, (int(dsize[1]), int(dsize[0])))


def gaussian_taps(ksize=101, sigma=11.0):
    """cv2.getGaussianKernel(ksize, sigma, CV_32F) by its formula: exp(-x^2 / (2 sigma^2)) in double, normalised, cast to float."""
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    t = np.exp((-0.5 / (sigma * sigma)) * x * x)
    return (t * (1.0 / t.sum())).astype(np.float32)


_TAPS = {}


def _taps_on(device, ksize=101, sigma=11.0):
    key = (str(device), ksize, sigma)
    if key not in _TAPS:
        _TAPS[key] = torch.from_numpy(gaussian_taps(ksize, sigma)).to(device)
    return _TAPS[key]


def mask_postprocess(mask_u8, thres=20):
    """face_enhancement.py:44-49 on device uint8 masks [B,H,W] (0 / 255): / 255, a frame of thres pixels zeroed, two
    GaussianBlur((101, 101), 11) -- each rows then columns, fp32 -> fp32 [B,H,W]."""
    if not mask_u8.is_cuda:
        raise RuntimeError("mask_postprocess runs on the ROCm device only (no CPU path)")
    taps = _taps_on(mask_u8.device)
    a = K.mask_prep(mask_u8, thres)
    b = torch.empty_like(a)
    for _ in range(2):
        K.blur_pass(a, taps, 1, out=b)
        K.blur_pass(b, taps, 0, out=a)
    return a


def smooth_small_face(faces_u8):
    """cv2.filter2D(ef, -1, [[1,2,1],[2,4,2],[1,2,1]] / 16) (face_enhancement.py:32-36,93-94) on device uint8 [B,H,W,3] or [H,W,3]."""
    if not faces_u8.is_cuda:
        raise RuntimeError("smooth_small_face runs on the ROCm device only (no CPU path)")
    return K.binomial3_u8(faces_u8[None])[0] if faces_u8.dim() == 3 else K.binomial3_u8(faces_u8)


def merge_and_blend(masks, faces, background, out=None):
    """face_enhancement.py:100-108: masks fp32 [n,H,W] and faces uint8 [n,H,W,3], already warped into the frame, over the uint8
    frame `background`; out may be the background itself."""
    if not background.is_cuda:
        raise RuntimeError("merge_and_blend runs on the ROCm device only (no CPU path)")
    return K.merge_blend(masks, faces, background, out=out)


def gpen_restore(generator):
    """FaceGAN.process (face_gan.py:38-62) around a GPEN generator, for uint8 BGR batches [B,S,S,3] on the device."""
    @torch.no_grad()
    def restore(faces_u8):
        x = ((faces_u8.float() / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2).flip(1).contiguous()
        out = generator(x)[0]
        out = (out * 0.5 + 0.5).permute(0, 2, 3, 1).flip(3)
        return (out.float().clamp(0, 1) * 255.0).to(torch.uint8).contiguous()
    return restore


class FaceRestorer(object):
    """face_enhancement.py:68-110 with the detector's output as an argument.  restore: a callable on device uint8 BGR batches
    [n,S,S,3] -> the same (gpen_restore(e4s_amd.gpen.FullGenerator(..)) is the reference's FaceGAN); parser: an
    e4s_amd.parsenet.FaceParse (anything with .masks(faces_u8, bgr=True)); detector: an e4s_amd.retinaface.RetinaFaceDetection
    (anything with .detect_device(frame_u8)), asked when process is given neither boxes nor landmarks."""

    def __init__(self, restore, parser, in_size=512, out_size=None, threshold=0.9, detector=None):
        out_size = in_size if out_size is None else out_size
        if in_size != out_size:
            raise NotImplementedError("FaceRestorer: in_size != out_size (the reference's cv2.resize of the face) is not provided")
        if not callable(restore):
            raise TypeError("FaceRestorer: restore is a callable on uint8 face batches (see gpen_restore)")
        self.restore, self.parser, self.detector = restore, parser, detector
        self.in_size, self.threshold = in_size, threshold
        self.reference_5pts = reference_5pts(in_size)

    @torch.no_grad()
    def process(self, frame_u8, boxes=None, landms=None, background=None):
        """frame_u8: device uint8 [H,W,3] (BGR); boxes [n,5] (x0, y0, x1, y1, score) and landms [n,10] (five x, then five y) on
        the host, as RetinaFace returns them -- both None: the detector given at construction finds them on the device (one
        device-to-host copy of its at most 750 x 15 floats); background: the frame the faces are blended over (the SR frame), same size; default
        the frame itself.  Returns (blended frame, aligned faces [n',S,S,3], restored faces [n',S,S,3]) on the device."""
        if not frame_u8.is_cuda:
            raise RuntimeError("FaceRestorer runs on the ROCm device only (no CPU path)")
        if frame_u8.dtype != torch.uint8 or frame_u8.dim() != 3 or frame_u8.shape[2] != 3:
            raise ValueError("FaceRestorer.process: a uint8 [H,W,3] frame")
        frame_u8 = frame_u8.contiguous()
        if (boxes is None) != (landms is None):
            raise ValueError("FaceRestorer.process: boxes and landms come together (or neither, with a detector)")
        if boxes is None:
            if self.detector is None:
                raise ValueError("FaceRestorer.process: no boxes / landms and no detector (FaceRestorer(detector=RetinaFaceDetection(..)))")
            dets, lms, counts = self.detector.detect_device(frame_u8)
            n = int(counts[0])
            both = torch.cat((dets[0, :n], lms[0, :n]), 1).cpu().numpy()
            boxes, landms = both[:, :5], both[:, 5:]
        bg = frame_u8 if background is None else background.contiguous()
        if tuple(bg.shape) != tuple(frame_u8.shape) or bg.dtype != torch.uint8:
            raise ValueError("FaceRestorer.process: background is a uint8 frame of the frame's size (resize the frame to the SR size first)")
        h, w = frame_u8.shape[:2]
        s = self.in_size
        boxes, landms = np.asarray(boxes, dtype=np.float64).reshape(-1, 5), np.asarray(landms, dtype=np.float64).reshape(-1, 10)
        keep = [i for i in range(len(boxes)) if not boxes[i, 4] < self.threshold]
        empty = torch.empty(0, s, s, 3, device=frame_u8.device, dtype=torch.uint8)
        if not keep:
            return K.merge_blend(None, None, bg), empty, empty
        tfms = [similarity_transform(landms[i].reshape(2, 5), self.reference_5pts) for i in keep]
        orig = torch.stack([warp_affine(frame_u8, tfm, (s, s)) for tfm, _ in tfms])
        enhanced = self.restore(orig)
        if tuple(enhanced.shape) != tuple(orig.shape) or enhanced.dtype != torch.uint8:
            raise RuntimeError("FaceRestorer: restore must return uint8 faces of the shape it was given")
        enhanced = enhanced.contiguous()
        soft = mask_postprocess(self.parser.masks(enhanced, bgr=True))
        small = [k for k, i in enumerate(keep) if min(boxes[i, 3] - boxes[i, 1], boxes[i, 2] - boxes[i, 0]) < 100]
        pasted = enhanced
        if small:
            pasted = enhanced.clone()
            pasted[small] = smooth_small_face(enhanced[small].contiguous())
        masks = torch.stack([warp_affine(soft[k], inv, (w, h)) for k, (_, inv) in enumerate(tfms)])
        faces = torch.stack([warp_affine(pasted[k], inv, (w, h)) for k, (_, inv) in enumerate(tfms)])
        return K.merge_blend(masks, faces, bg), orig, enhanced
