"""GPU tests of the face paste path (e4s_amd/face_paste.py, csrc/face_paste.hip) against the numpy restatements of the OpenCV
steps in tests/paste_cases.py (themselves checked against scipy in tests/test_face_paste_host.py) and fp64 restatements."""
import numpy as np
import pytest
import torch

import paste_cases as pc
from e4s_amd import face_paste as fp

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROT = [[0.9, -0.35, 12.5], [0.35, 0.9, -7.25]]                            # leaves part of a 64 x 48 target uncovered
MAPS = [ROT, [[1.7, 0.2, -20.0], [-0.1, 1.4, 3.0]], [[1, 0, 5], [0, 1, -3]], [[0.31, 0.02, 3.3], [-0.02, 0.31, 1.9]]]


def _img(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("shape,dsize", [((37, 53), (64, 48)), ((48, 64), (53, 37))])
def test_uint8_warp_is_bit_equal_and_fp32_warp_within_1e_6_of_the_restatement(shape, dsize):
    src = _img(*shape, seed=1)
    f32 = np.random.RandomState(2).rand(*shape).astype(np.float32)
    for M in MAPS:
        for inverse in (False, True):
            want = pc.warp_affine(src, M, dsize, inverse=inverse)
            got = fp.warp_affine(_dev(src), M, dsize, inverse=inverse).cpu().numpy()
            assert got.shape == (dsize[1], dsize[0], 3) and np.array_equal(got, want), (M, inverse)
            wf = pc.warp_affine(f32, M, dsize, inverse=inverse)
            gf = fp.warp_affine(_dev(f32), M, dsize, inverse=inverse).cpu().numpy()
            assert gf.dtype == np.float32 and float(np.abs(gf - wf).max()) <= 1e-6, (M, inverse)
    cover = pc.warp_affine(np.full(shape + (3,), 255, np.uint8), ROT, dsize)
    assert (cover == 0).any() and (cover == 255).any()                    # the rotation leaves part of the target uncovered


@pytest.mark.parametrize("shape", [(140, 150), (60, 70)])                  # larger than the 50-pixel reflection / the reflection wraps
def test_mask_postprocess_against_fp64(shape):
    """Worst-case fp32 rounding: 4 passes x 101 taps x 2^-24 ~ 2.4e-5 on values in [0, 1]; bound 1e-4 (a factor 4 of margin)."""
    rng = np.random.RandomState(3)
    mask = (np.kron(rng.rand(shape[0] // 10, shape[1] // 10) > 0.4, np.ones((10, 10))) * 255).astype(np.uint8)
    masks = np.stack([mask, 255 - mask])
    got = fp.mask_postprocess(_dev(masks)).cpu().numpy()
    taps = fp.gaussian_taps()
    for b in range(2):
        ref = pc.mask_postprocess64(masks[b], taps)
        err = float(np.abs(got[b] - ref).max())
        print(f"blur {shape} sample {b}: err {err:.2e}, max {ref.max():.3f}")
        assert ref.max() > 0.05 and err <= 1e-4
    one = fp.mask_postprocess(_dev(masks[1:]))
    assert torch.equal(one[0].cpu(), torch.from_numpy(got[1]))            # the batch does not change a sample's bits


def test_small_face_filter_is_exact():
    img = _img(23, 31, seed=4)
    assert np.array_equal(fp.smooth_small_face(_dev(img)).cpu().numpy(), pc.binomial3(img))
    batch = np.stack([img, _img(23, 31, seed=5)])
    got = fp.smooth_small_face(_dev(batch)).cpu().numpy()
    assert np.array_equal(got[0], pc.binomial3(batch[0])) and np.array_equal(got[1], pc.binomial3(batch[1]))


def test_merge_and_blend_two_overlapping_faces_in_both_orders_and_in_place():
    h, w = 40, 56
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    blob = lambda cy, cx, r: np.clip(1.2 - np.hypot(ys - cy, xs - cx) / r, 0, 1)
    m64 = np.stack([blob(18, 20, 14), blob(22, 34, 15)])
    m64[:, :, 50:] = 0                                                    # columns outside every face
    faces, bg = np.stack([_img(h, w, 6), _img(h, w, 7)]), _img(h, w, 8)
    for order in ([0, 1], [1, 0]):
        mm, ff = m64[order], faces[order]
        levels, who = pc.merge_blend64(mm, ff, bg)
        got = fp.merge_and_blend(_dev(mm.astype(np.float32)), _dev(ff), _dev(bg)).cpu().numpy()
        assert float(np.abs(got.astype(np.float64) - levels).max()) <= 1.0
        assert (who == 0).any() and (who == 1).any() and (who == -1).any()
        assert np.array_equal(got[who == -1], bg[who == -1])              # outside every face: bit-equal to the background
        frame = _dev(bg)
        out = fp.merge_and_blend(_dev(mm.astype(np.float32)), _dev(ff), frame, out=frame)
        assert out.data_ptr() == frame.data_ptr() and np.array_equal(frame.cpu().numpy(), got)
    a = fp.merge_and_blend(_dev(m64.astype(np.float32)), _dev(faces), _dev(bg)).cpu().numpy()
    b = fp.merge_and_blend(_dev(m64[::-1].astype(np.float32)), _dev(faces[::-1]), _dev(bg)).cpu().numpy()
    assert np.array_equal(a, b)                                           # distinct masks: the larger one wins in either order


class _Parser:
    """Stand-in for FaceParse: an ellipse mask that depends on nothing but the batch size."""

    def masks(self, faces_u8, bgr=True):
        ys, xs = np.mgrid[0:512, 0:512]
        m = ((((ys - 256) / 200.0) ** 2 + ((xs - 256) / 160.0) ** 2) <= 1).astype(np.uint8) * 255
        return _dev(np.stack([m] * faces_u8.shape[0]))


def test_face_restorer_on_a_small_frame_against_the_numpy_pipeline(golden):
    g = golden("parsenet.pt")
    h, w = 256, 320
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    frame = np.rint(np.stack([128 + 70 * np.sin(xs / 23.0 + c) + 40 * np.cos(ys / 17.0 - c) for c in range(3)], -1)).astype(np.uint8)
    names = ["frontal", "small", "outside"]
    pts = [g[f"lm.{n}"]["pts"].numpy() for n in names]
    landms = np.stack([p.T.reshape(10) for p in pts])                     # five x, then five y
    boxes = np.array([[80, 40, 230, 200, 0.99], [40, 180, 80, 225, 0.95], [250, 0, 320, 90, 0.5]])   # the third is below 0.9
    restorer = fp.FaceRestorer(lambda faces: 255 - faces, _Parser(), in_size=512)
    out, orig, enh = restorer.process(_dev(frame), boxes, landms)
    assert tuple(orig.shape) == (2, 512, 512, 3) and torch.equal(enh, 255 - orig)
    # the numpy pipeline, face_enhancement.py:68-108
    taps = fp.gaussian_taps()
    ref5 = g["ref5"].numpy()
    masks, faces = [], []
    for k in range(2):
        tfm, inv = g[f"lm.{names[k]}"]["tfm"].numpy(), g[f"lm.{names[k]}"]["tfm_inv"].numpy()
        of = pc.warp_affine(frame, tfm, (512, 512))
        assert np.array_equal(orig[k].cpu().numpy(), of)
        ef = 255 - of
        soft = pc.mask_postprocess64(_Parser().masks(torch.zeros(1))[0].cpu().numpy(), taps)
        if k == 1:                                                        # min(fh, fw) = 40 < 100
            ef = pc.binomial3(ef)
        masks.append(pc.warp_affine(soft.astype(np.float32), inv, (w, h)).astype(np.float64))
        faces.append(pc.warp_affine(ef, inv, (w, h)))
    levels, who = pc.merge_blend64(np.stack(masks), np.stack(faces), frame)
    got = out.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - levels).max())
    print(f"FaceRestorer: err {err:.3f} levels; faces own {float((who >= 0).mean()):.3f} of the frame")
    assert err <= 1.0 and (who == 0).any() and (who == 1).any() and not np.array_equal(got, frame)
    # a background of its own (the SR frame), and a face below the threshold alone leaves the frame untouched
    bgd = 255 - frame
    out2, _, _ = restorer.process(_dev(frame), boxes, landms, background=_dev(bgd))
    assert np.array_equal(out2.cpu().numpy()[who == -1], bgd[who == -1])
    out3, o3, e3 = restorer.process(_dev(frame), boxes[2:], landms[2:])
    assert np.array_equal(out3.cpu().numpy(), frame) and o3.shape[0] == 0 and e3.shape[0] == 0
    with pytest.raises(ValueError):
        restorer.process(_dev(frame), boxes, landms, background=_dev(bgd[:100]))
