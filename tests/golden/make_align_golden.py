"""Generate tests/golden/align.pt by running the REAL reference's alignment code on CPU (build container only):
    python tests/golden/make_align_golden.py

What runs is the reference's own src/utils/alignmengt.py, executed in place with its absent third-party imports (cv2, skimage)
stubbed: compute_transform (get_landmark replaced by the given landmarks), the quad stacking of crop_faces, crop_image and
calc_alignment_coefficients; then the paste-back of scripts/face_swap.py:313-327 (putalpha(255) -> transform(PERSPECTIVE,
BILINEAR) -> alpha_composite) with the inverse transform of scripts/face_swap.py:110-113.

Stored (data only; uint8 images zlib-packed as make_golden.py:_z does):
  frame     uint8 [300,400,3]  rows 380..679, columns 312..711 of example/input/faceswap/target.jpg
  lm68      float64 [68,2]     one seeded landmark set placed on it (eyes ~57 px apart, tilted; a quad of side ~240 px that
                               leaves the frame at the top)
  size      128
  c, x, y   float64 [2]        compute_transform's centre and axes
  quad      float64 [4,2]
  window    (x0, y0, x1, y1)   what crop_image cut out before the transform (read off the image it handed to transform)
  quad_coeffs   float64 [8]    the QUAD coefficients Pillow derived (Image.py restated) from the quad crop_image passed it
  inv_coeffs    float64 [8]    calc_alignment_coefficients(quad + 0.5, [[0,0],[0,S],[S,S],[S,0]])
  crop      uint8 [128,128,3]  crop_image's result
  pasted    uint8 [300,400,3]  the frame with the INVERTED crop (255 - crop: a face that differs from the frame) pasted back"""
import importlib.util
import os
import sys
import types
import zlib

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("E4S_REFERENCE_ROOT", "/root/reference")
SIZE = 128
SEED = 20


def _z(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return zlib.compress(a.tobytes(), 9), tuple(a.shape)


def reference_alignment():
    for name in ("cv2", "skimage", "skimage.io", "tqdm"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except ImportError:
                mod = types.ModuleType(name)
                mod.tqdm = lambda it, *a, **k: it
                sys.modules[name] = mod
    if not hasattr(sys.modules["skimage"], "io"):
        sys.modules["skimage"].io = sys.modules["skimage.io"]
    spec = importlib.util.spec_from_file_location("ref_alignmengt", os.path.join(REF_ROOT, "src", "utils", "alignmengt.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def landmarks():
    """A seeded 68-point set: only the eyes (36..47) and the mouth corners (48, 54) enter compute_transform; the rest is filled
    with plausible positions so the array looks like a detector's."""
    rng = np.random.default_rng(SEED)
    lm = np.array([190.0, 150.0]) + rng.normal(0.0, 40.0, (68, 2))
    ring = np.stack([np.cos(np.arange(6) * np.pi / 3), 0.5 * np.sin(np.arange(6) * np.pi / 3)], 1) * 9.0
    lm[36:42] = np.array([160.3, 112.6]) + ring + rng.normal(0.0, 0.7, (6, 2))
    lm[42:48] = np.array([216.1, 124.9]) + ring + rng.normal(0.0, 0.7, (6, 2))
    lm[48:60] = np.array([176.0, 186.0]) + rng.normal(0.0, 6.0, (12, 2))
    lm[48] = np.array([153.7, 176.2]) + rng.normal(0.0, 0.7, 2)
    lm[54] = np.array([198.4, 187.9]) + rng.normal(0.0, 0.7, 2)
    return lm


def main():
    ref = reference_alignment()
    target = np.array(Image.open(os.path.join(REF_ROOT, "example", "input", "faceswap", "target.jpg")).convert("RGB"))
    frame = np.ascontiguousarray(target[380:680, 312:712])
    lm = landmarks()
    ref.get_landmark = lambda *a, **k: lm.copy()
    c, x, y = ref.compute_transform(None, None, scale=1.0)
    quad = np.stack([c - x - y, c - x + y, c + x + y, c + x - y])                      # crop_faces, alignmengt.py:209

    seen = {}
    orig_transform = Image.Image.transform

    def spy(self, size, method, data=None, *a, **k):
        seen.setdefault("calls", []).append((self.size, np.array(data, dtype=np.float64)))
        return orig_transform(self, size, method, data, *a, **k)

    img = Image.fromarray(frame)
    Image.Image.transform = spy
    try:
        crop = ref.crop_image(img, SIZE, quad.copy())
    finally:
        Image.Image.transform = orig_transform
    (win_size, passed), = seen["calls"]
    passed = passed.reshape(4, 2)                                                       # quad - window origin + 0.5
    origin = np.rint(quad[0] + 0.5 - passed[0]).astype(int)
    window = (int(origin[0]), int(origin[1]), int(origin[0]) + win_size[0], int(origin[1]) + win_size[1])
    nw, sw, se, ne = passed
    As = At = 1.0 / SIZE                                                                # Image.py: __transformer, QUAD
    quad_coeffs = np.array([nw[0], (ne[0] - nw[0]) * As, (sw[0] - nw[0]) * At, (se[0] - sw[0] - ne[0] + nw[0]) * As * At,
                            nw[1], (ne[1] - nw[1]) * As, (sw[1] - nw[1]) * At, (se[1] - sw[1] - ne[1] + nw[1]) * As * At])
    inv = ref.calc_alignment_coefficients(quad + 0.5, [[0, 0], [0, SIZE], [SIZE, SIZE], [SIZE, 0]])   # face_swap.py:110-113

    crop = np.array(crop)
    face = Image.fromarray(255 - crop)
    swapped_and_pasted = face.convert("RGBA")                                           # face_swap.py:313-327
    pasted_image = img.convert("RGBA")
    swapped_and_pasted.putalpha(255)
    projected = swapped_and_pasted.transform(img.size, Image.PERSPECTIVE, inv, Image.BILINEAR)
    pasted_image.alpha_composite(projected)
    pasted = np.array(pasted_image)
    assert int(pasted[..., 3].min()) == 255 and set(np.unique(np.array(projected)[..., 3])) <= {0, 255}

    out = dict(frame=_z(frame), lm68=torch.from_numpy(lm), size=SIZE, c=torch.from_numpy(c), x=torch.from_numpy(x),
               y=torch.from_numpy(y), quad=torch.from_numpy(quad), window=window, quad_coeffs=torch.from_numpy(quad_coeffs),
               inv_coeffs=torch.from_numpy(np.asarray(inv, dtype=np.float64)), crop=_z(crop), pasted=_z(pasted[..., :3]))
    path = os.path.join(HERE, "align.pt")
    torch.save(out, path)
    side = float(np.hypot(*(quad[3] - quad[0])))
    print(f"wrote {path}: {os.path.getsize(path)} bytes; window {window}, quad side {side:.1f}, covered "
          f"{float((np.array(projected)[..., 3] == 255).mean()):.3f} of the frame, crop zeros {float((crop.sum(-1) == 0).mean()):.3f}")
    print(quad)


if __name__ == "__main__":
    main()
