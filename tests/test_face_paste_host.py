"""Host-side tests of e4s_amd/face_paste.py: the landmark arithmetic against the reference's recorded results
(tests/golden/parsenet.pt), the Gaussian taps against their formula, and the numpy restatement of cv2.warpAffine
(tests/paste_cases.py), which the GPU tests use as their yardstick, against scipy.ndimage.  No GPU, no cv2."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

import paste_cases as pc
from e4s_amd import face_paste as fp


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def test_reference_points_and_similarity_transform_equal_the_reference(golden):
    g = golden("parsenet.pt")
    ref5 = g["ref5"].numpy()
    assert _rel(fp.reference_5pts(512), ref5) <= 1e-12
    assert _rel(fp.reference_5pts(256), ref5 / 2) <= 1e-12
    for name in ("frontal", "rotated30", "small", "outside"):
        rec = g[f"lm.{name}"]
        tfm, inv = fp.similarity_transform(rec["pts"].numpy(), ref5)
        assert tfm.dtype == np.float64 and tfm.shape == (2, 3) and inv.shape == (2, 3)
        assert _rel(tfm, rec["tfm"].numpy()) <= 1e-12, name
        assert _rel(inv, rec["tfm_inv"].numpy()) <= 1e-12, name
        tfm2, _ = fp.similarity_transform(rec["pts"].numpy().T.reshape(10).reshape(2, 5), ref5)      # RetinaFace's (2, 5) layout
        assert np.array_equal(tfm2, tfm)
        full = np.vstack([tfm, [0, 0, 1]]) @ np.vstack([inv, [0, 0, 1]])
        assert np.abs(full - np.eye(3)).max() < 1e-9                      # the pair are inverses of each other
    with pytest.raises(ValueError):
        fp.similarity_transform(np.zeros((5, 2)), ref5)


def test_gaussian_taps_follow_getGaussianKernel_formula():
    t = fp.gaussian_taps(101, 11.0)
    assert t.dtype == np.float32 and t.shape == (101,)
    raw = [math.exp(-((i - 50.0) ** 2) / (2 * 11.0 * 11.0)) for i in range(101)]
    want = np.array([v / sum(raw) for v in raw])
    assert np.abs(t.astype(np.float64) - want).max() <= 2.0 ** -24 * want.max()
    assert np.array_equal(t, t[::-1]) and abs(float(t.astype(np.float64).sum()) - 1) < 1e-6


def test_invert_affine_is_opencvs_and_shared_with_the_yardstick():
    M = np.array([[0.9, -0.35, 12.5], [0.35, 0.9, -7.25]])
    a = np.array(fp.invert_affine(M))
    assert np.array_equal(a, pc.invert(M))
    fwd = np.vstack([M, [0, 0, 1]])
    assert np.abs(np.vstack([a.reshape(2, 3), [0, 0, 1]]) @ fwd - np.eye(3)).max() < 1e-12


def _smooth_u8(h, w, seed):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.RandomState(seed)
    ph = rng.uniform(0, 6.28, 3)
    img = np.stack([128 + 60 * np.sin(xs / 9.0 + ph[c]) + 50 * np.cos(ys / 7.0 + ph[c] * 2) for c in range(3)], -1)
    return np.rint(img).astype(np.uint8)


@pytest.mark.parametrize("M", [[[0.9, -0.35, 12.5], [0.35, 0.9, -7.25]], [[1.7, 0.2, -20.0], [-0.1, 1.4, 3.0]],
                               [[0.5, 0.0, 5.3], [0.0, 0.5, 2.7]]])
def test_numpy_warp_affine_against_scipy_bilinear_within_the_coordinate_grid_bound(M):
    """OpenCV's warpAffine rounds the source coordinates to a 1/32-pixel grid: each coordinate is off by at most 1/64 from that
    rounding plus 2^-9 from the two cvRound calls at 1/1024 (row term and column term, 2^-11 each, and the >> 5 floor).  On an image
    whose neighbouring pixels differ by at most G levels along either axis the bilinear interpolant moves by at most G per pixel
    per axis, so the value is off by at most 2 G (1/64 + 2^-9); rounding the result to a level adds at most 1/2, the integer
    weights' rounding less than 1/2: 2 G (1/64 + 2^-9) + 1 levels against an exact fp64 bilinear of the same pixels."""
    src = _smooth_u8(53, 64, 1)
    G = float(max(np.abs(np.diff(src.astype(np.int64), axis=0)).max(), np.abs(np.diff(src.astype(np.int64), axis=1)).max()))
    bound = 2 * G * (1 / 64 + 2.0 ** -9) + 1
    wd, hd = 48, 37
    a = pc.invert(M)
    got = pc.warp_affine(src, M, (wd, hd)).astype(np.float64)
    mat, off = np.array([[a[4], a[3]], [a[1], a[0]]]), np.array([a[5], a[2]])
    ys, xs = np.mgrid[0:hd, 0:wd]
    sx, sy = a[0] * xs + a[1] * ys + a[2], a[3] * xs + a[4] * ys + a[5]
    inside = (sx >= 1) & (sx <= src.shape[1] - 2) & (sy >= 1) & (sy <= src.shape[0] - 2)
    assert inside.mean() > 0.2
    for c in range(3):
        ref = ndimage.affine_transform(src[..., c].astype(np.float64), mat, offset=off, output_shape=(hd, wd), order=1, mode="constant")
        err = np.abs(got[..., c] - ref)[inside].max()
        assert err <= bound, (err, bound, G)
    f32 = pc.warp_affine(src[..., 0].astype(np.float32), M, (wd, hd))
    ref = ndimage.affine_transform(src[..., 0].astype(np.float64), mat, offset=off, output_shape=(hd, wd), order=1, mode="constant")
    assert f32.dtype == np.float32 and np.abs(f32 - ref)[inside].max() <= bound - 1 + 1e-3
    # far outside the source everything is the border value
    assert not pc.warp_affine(src, [[1, 0, 500], [0, 1, 0]], (wd, hd)).any()


def test_numpy_warp_affine_is_exact_for_integer_translations_and_inverse_flag():
    src = _smooth_u8(37, 53, 2)
    for tx, ty in ((0, 0), (5, 3), (-7, 11)):
        out = pc.warp_affine(src, [[1, 0, tx], [0, 1, ty]], (64, 48))
        want = np.zeros((48, 64, 3), dtype=np.uint8)
        for y in range(48):
            for x in range(64):
                if 0 <= y - ty < 37 and 0 <= x - tx < 53:
                    want[y, x] = src[y - ty, x - tx]
        assert np.array_equal(out, want)
        f = pc.warp_affine(src[..., 1].astype(np.float32), [[1, 0, tx], [0, 1, ty]], (64, 48))
        assert np.array_equal(f, want[..., 1].astype(np.float32))
    M = [[0.9, -0.35, 12.5], [0.35, 0.9, -7.25]]
    assert np.array_equal(pc.warp_affine(src, pc.invert(M).reshape(2, 3), (64, 48), inverse=True), pc.warp_affine(src, M, (64, 48)))


def test_yardstick_filters_on_known_answers():
    img = np.full((6, 7, 3), 77, dtype=np.uint8)
    assert np.array_equal(pc.binomial3(img), img)
    img[2, 3] = 255                                                       # 77 + 178 k / 16 for k in 1, 2, 4: .125, .25, .5 -> half to even
    out = pc.binomial3(img)[..., 0]
    assert out[2, 3] == 122 and out[2, 2] == 99 and out[1, 2] == 88 and out[0, 0] == 77
    taps = fp.gaussian_taps()
    flat = pc.blur64(np.full((60, 70), 0.5), taps)
    assert np.abs(flat - 0.5).max() < 1e-6                                # reflection keeps a constant, even where it wraps


def test_face_restorer_refuses_what_is_out_of_scope():
    with pytest.raises(NotImplementedError):
        fp.FaceRestorer(lambda x: x, None, in_size=512, out_size=1024)
    with pytest.raises(TypeError):
        fp.FaceRestorer(None, None)
    r = fp.FaceRestorer(lambda x: x, None)
    assert r.threshold == 0.9 and r.reference_5pts.shape == (5, 2)
    with pytest.raises(RuntimeError):
        r.process(torch.zeros(8, 8, 3, dtype=torch.uint8), np.zeros((0, 5)), np.zeros((0, 10)))     # no CPU path
    with pytest.raises(RuntimeError):
        fp.warp_affine(torch.zeros(8, 8, 3, dtype=torch.uint8), np.eye(3)[:2], (4, 4))
