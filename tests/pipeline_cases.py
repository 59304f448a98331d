"""The yardsticks of tests/test_pipeline_cases_host.py and tests/test_gpu_pipeline.py: numpy / torch-CPU statements of the four joins
of e4s_amd/pipeline.py (csrc/pipeline.hip), stub stages, and `compose`, the 13 steps of scripts/face_swap.py:150-331 written out by
hand.  skimage and cv2 are not available: the resize is stated through the two scipy calls scikit-image 0.20 makes, the enlargement
through the integer arithmetic of OpenCV's resize.cpp."""
import numpy as np
import torch


# ---- join 1: skimage.transform.resize(x / 255.0, (H/4, W/4)) -------------------------------------------------------------
def resize_aa4_scipy(img_u8):
    """scikit-image 0.20 `resize` for an exact factor of 4 (anti_aliasing, order 1, mode 'reflect' = ndimage 'mirror'), fp64."""
    from scipy import ndimage as ndi
    x = np.asarray(img_u8).astype(np.float64) / 255.0
    g = ndi.gaussian_filter(x, (1.5, 1.5, 0), mode="mirror", cval=0)
    return ndi.zoom(g, (0.25, 0.25, 1), order=1, mode="mirror", grid_mode=True)


def aa4_taps():
    """The 14 taps per axis at inputs 4 i - 5 .. 4 i + 8: t[k] = (g[k] + g[k-1]) / 2, g the normalised Gaussian (sigma 1.5, radius 6)."""
    k = np.arange(-6, 7, dtype=np.float64)
    g = np.exp(-0.5 / (1.5 * 1.5) * k * k)
    g /= g.sum()
    return 0.5 * (np.concatenate([g, [0.0]]) + np.concatenate([[0.0], g]))


def mirror(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def resize_aa4_closed(img_u8):
    """The closed form the kernel implements, fp64: rows first (scipy filters axis 0 first), then columns."""
    x = np.asarray(img_u8).astype(np.float64) / 255.0
    t = aa4_taps()
    idx = lambda n: mirror(4 * np.arange(n // 4)[:, None] - 5 + np.arange(14)[None, :], n)    # [n/4, 14]
    x = np.einsum("ikwc,k->iwc", x[idx(x.shape[0])], t)
    return np.einsum("hjkc,k->hjc", x[:, idx(x.shape[1])], t)


# ---- join 2: (pred * 255).astype(np.uint8) and cv2.resize(img, (4w, 4h)) ---------------------------------------------------
def truncate_u8(pred):
    """numpy's own statement: the fp32 product, truncated."""
    return (np.asarray(pred, dtype=np.float32) * np.float32(255)).astype(np.uint8)


def cv_linear_coeffs(n_src, n_dst):
    """resize.cpp, INTER_LINEAR: (first sample index, coefficient of the first, of the second sample) per destination index."""
    scale = n_src / n_dst
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= n_src - 1
    f = np.where(lo | hi, np.float32(0), f)
    s = np.where(lo, 0, np.where(hi, n_src - 1, s))
    c1 = np.rint(f.astype(np.float64) * 2048).astype(np.int64)
    return s, 2048 - c1, c1


def cv_resize_x4(img_u8):
    """cv2.resize(img, (4w, 4h)) (INTER_LINEAR, 8-bit, the non-exact path): HResizeLinear then VResizeLinear in int32."""
    src = np.asarray(img_u8).astype(np.int64)
    h, w = src.shape[:2]
    sx, a0, a1 = cv_linear_coeffs(w, 4 * w)
    sy, b0, b1 = cv_linear_coeffs(h, 4 * h)
    sx1, sy1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    S = src[:, sx] * a0[None, :, None] + src[:, sx1] * a1[None, :, None]                      # [h, 4w, C]
    S0, S1 = S[sy] >> 4, S[sy1] >> 4
    out = (((b0[:, None, None] * S0) >> 16) + ((b1[:, None, None] * S1) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def bilinear_x4_rounded(img_u8):
    """floor(exact + 0.5) of the same bilinear sample (half-pixel centres, replicated border), for comparison only."""
    src = np.asarray(img_u8).astype(np.float64)
    h, w = src.shape[:2]
    sx, a0, a1 = cv_linear_coeffs(w, 4 * w)
    sy, b0, b1 = cv_linear_coeffs(h, 4 * h)
    sx1, sy1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    S = src[:, sx] * (a0 / 2048.0)[None, :, None] + src[:, sx1] * (a1 / 2048.0)[None, :, None]
    out = S[sy] * (b0 / 2048.0)[:, None, None] + S[sy1] * (b1 / 2048.0)[:, None, None]
    return np.floor(out + 0.5).astype(np.uint8)


# ---- join 3: ToTensor + Normalize(0.5, 0.5) ------------------------------------------------------------------------------
def to_net_torch(rgb_u8):
    """torchvision's ToTensor (permute, float32, div 255) and Normalize (sub_ 0.5, div_ 0.5) on CPU: uint8 [B,H,W,3] -> [B,3,H,W]."""
    t = torch.from_numpy(np.ascontiguousarray(rgb_u8)).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    mean = torch.tensor([0.5, 0.5, 0.5], dtype=torch.float32).view(1, 3, 1, 1)
    return t.sub_(mean).div_(mean.clone())


# ---- stub stages (elementwise torch ops on the device; deterministic, so two runs agree bit for bit) -----------------------
class StubReenactor(object):
    def run(self, source, driving):
        return (0.5 * source[None] + 0.5 * driving).roll(1, dims=-1).contiguous()


class StubSR(object):
    def upscale(self, images_u8, bgr=False):
        return images_u8.repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()


class StubParser(object):
    def parse(self, images_u8):
        return ((images_u8[:, ::2, ::2, 0] >> 3) % 12).contiguous()


class StubMaskParser(object):
    """FaceRestorer's parser: a fixed blob."""

    def masks(self, faces_u8, bgr=True):
        n, s = faces_u8.shape[0], faces_u8.shape[1]
        y, x = torch.meshgrid(torch.arange(s, device=faces_u8.device), torch.arange(s, device=faces_u8.device), indexing="ij")
        blob = ((y - s // 2) ** 2 * 2 + (x - s // 2) ** 2 * 3 < (s * s) // 3).to(torch.uint8) * 255
        return blob[None].expand(n, s, s).contiguous()


class StubDetector(object):
    """One fixed box and the five landmarks of a face slightly turned in a 1024^2 frame."""

    def detect_device(self, frame_u8):
        dev = frame_u8.device
        dets = torch.tensor([[[230.0, 180.0, 800.0, 860.0, 0.99]]], device=dev)
        lms = torch.tensor([[[400.0, 640.0, 530.0, 430.0, 630.0, 450.0, 430.0, 570.0, 660.0, 645.0]]], device=dev)
        return dets, lms, torch.tensor([1], dtype=torch.int32)


class StubSwap(object):
    """face_swap_core's arguments behind the net: driven where the swapped mask holds a face class, else the target."""
    num_seg_cls = 12

    def __call__(self, driven, driven_mask, target, target_mask, swapped_mask, noise=None):
        w = swapped_mask[:, [1, 2, 3, 5, 6, 9]].sum(1, keepdim=True).repeat_interleave(2, 2).repeat_interleave(2, 3)
        return (w * driven + (1.0 - w) * target).contiguous()


def stub_stages(swap=None):
    """(net, reenactor, sr, restorer, parser) for FaceSwapPipeline and compose."""
    from e4s_amd.face_paste import FaceRestorer
    restorer = FaceRestorer(lambda x: 255 - x, StubMaskParser(), in_size=512, detector=StubDetector())
    return (StubSwap() if swap is None else swap), StubReenactor(), StubSR(), restorer, StubParser()


# ---- the pipeline by hand ------------------------------------------------------------------------------------------------
@torch.no_grad()
def compose(stages, source_u8, targets_u8, source_quad=None, target_quads=None, target_labels=None, lap_bld=False, outer_dilation=5,
            noise=None):
    """scripts/face_swap.py:150-331 from the stages, the existing native stage functions and the HOST statements above for the joins
    -> (result, taps).  One exception: the anti-aliased resize is defined to a tolerance, not to the bit (28 fp32 multiply-adds), and
    everything behind it truncates, so compose takes the kernel's fp32 values and returns the fp64 statement beside them
    (taps['S_256_f64'], taps['T_256_f64']) for the caller to bound."""
    from e4s_amd import align, postproc
    from e4s_amd import kernels as K
    swap, reenactor, sr, restorer, parser = stages
    dev = targets_u8.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    b = targets_u8.shape[0]
    # 1
    S = align.crop_faces_by_quads(source_u8[None], source_quad) if source_quad is not None else source_u8[None]
    T = align.crop_faces_by_quads(targets_u8, target_quads) if target_quads is not None else targets_u8
    # 2
    S_256, T_256 = K.resize_aa4(S), K.resize_aa4(T)
    S_f64 = resize_aa4_closed(S[0].cpu().numpy())[None]
    T_f64 = np.stack([resize_aa4_closed(t) for t in T.cpu().numpy()])
    # 3
    T_lab = parser.parse(T) if target_labels is None else target_labels
    # 4
    pred = reenactor.run(S_256[0], T_256).cpu().numpy()                                       # [B,256,256,3] RGB in [0,1]
    # 5
    pred_bgr = np.ascontiguousarray(truncate_u8(pred)[..., ::-1])
    enlarged = np.stack([cv_resize_x4(f) for f in pred_bgr])
    # 6
    sr_frames = sr.upscale(up(pred_bgr), bgr=True)
    # 7
    D_bgr = torch.stack([restorer.process(up(enlarged[i]), background=sr_frames[i])[0] for i in range(b)])
    # 8
    D_rgb = np.ascontiguousarray(D_bgr.cpu().numpy()[..., ::-1])
    driven = to_net_torch(D_rgb).to(dev)
    D_lab = parser.parse(up(D_rgb))
    # 9
    target = to_net_torch(T.cpu().numpy()).to(dev)
    # 10
    s_lab, hole = postproc.swap_head_mask_revisit_considerGlass(D_lab.contiguous(), T_lab.contiguous())
    # 11
    r = swap.num_seg_cls if hasattr(swap, "num_seg_cls") else 12
    d_oh, t_oh, s_oh = (postproc.labelMap2OneHot(l[:, None].contiguous(), r) for l in (D_lab, T_lab, s_lab))
    face = swap(driven, d_oh, target, t_oh, s_oh, noise=noise)
    # 12
    stitched = postproc.stitch(face, T, s_lab, hole, lap_bld, outer_dilation)
    # 13
    out = align.swap_into_frames(stitched, targets_u8, target_quads) if target_quads is not None else stitched
    taps = dict(S_256=S_256, T_256=T_256, S_256_f64=S_f64, T_256_f64=T_f64, pred=pred, pred_bgr=up(pred_bgr), enlarged=up(enlarged),
                sr=sr_frames, D_bgr=D_bgr, D_labels=D_lab, T_labels=T_lab, swapped_labels=s_lab, hole=hole, swapped_face=face,
                stitched=stitched)
    return out, taps
