"""CPU tests of e4s_amd.align's host geometry against the fixture the reference's own functions produced
(tests/golden/make_align_golden.py), and of the yardstick of tests/test_gpu_align.py: the float64 numpy statement of Pillow's QUAD /
PERSPECTIVE + BILINEAR arithmetic (tests/align_cases.py) must equal live Pillow exactly."""
import numpy as np
import pytest
from PIL import Image

import align_cases as ac
from conftest import unz
from e4s_amd import align

RTOL = 1e-12


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert float(np.abs(got - want).max()) <= RTOL * float(np.abs(want).max()), (got, want)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("align.pt")


def test_compute_quad_matches_reference(fx):
    lm = fx["lm68"].numpy()
    quad = align.compute_quad(lm)
    _close(quad, fx["quad"].numpy())
    c, x, y = fx["c"].numpy(), fx["x"].numpy(), fx["y"].numpy()
    _close(quad, np.stack([c - x - y, c - x + y, c + x + y, c + x - y]))
    batch = align.compute_quad(np.stack([lm, lm + 3.0]), scale=1.25)
    assert batch.shape == (2, 4, 2)
    centre = quad.mean(0)
    _close(batch[0], centre + 1.25 * (quad - centre))                   # scale stretches the axes about the centre
    _close(batch[1], batch[0] + 3.0)


def test_calc_alignment_coefficients_matches_reference(fx):
    s = fx["size"]
    got = align.calc_alignment_coefficients(fx["quad"].numpy() + 0.5, [[0, 0], [0, s], [s, s], [s, 0]])
    _close(got, fx["inv_coeffs"].numpy())
    _close(align.paste_parameters(fx["quad"].numpy(), s)[0], fx["inv_coeffs"].numpy())
    # it is the frame -> face map: the quad's corners (+ 0.5) land on the face's corners
    for (px, py), (fx_, fy_) in zip(fx["quad"].numpy() + 0.5, [[0, 0], [0, s], [s, s], [s, 0]]):
        d = got[6] * px + got[7] * py + 1
        assert abs((got[0] * px + got[1] * py + got[2]) / d - fx_) < 1e-6 and abs((got[3] * px + got[4] * py + got[5]) / d - fy_) < 1e-6


def test_crop_window_and_quad_coefficients_match_reference(fx):
    quad, s = fx["quad"].numpy(), fx["size"]
    frame = unz(fx["frame"]).numpy()
    win = align.crop_window(quad, frame.shape[:2], s)
    assert tuple(int(v) for v in win) == tuple(fx["window"])
    assert tuple(win) == tuple(ac.reference_window(quad, frame.shape[:2]))
    coeffs, windows = align.crop_parameters(quad, frame.shape[:2], s)
    assert windows.dtype == np.int32 and tuple(windows[0]) == tuple(fx["window"])
    _close(coeffs[0], fx["quad_coeffs"].numpy())
    # a quad whose bounding box + border covers the frame: the reference does not crop
    h, w = frame.shape[:2]
    assert align.crop_window(ac.square((w / 2, h / 2), 200.0, 45.0), (h, w), 1024) == (0, 0, w, h)


def test_crop_window_refuses_the_branches_it_does_not_implement():
    size = 64
    # crop_image's qsize is the quad's diagonal: half-side sqrt(2) * size makes it 4 x size, where shrink becomes 2
    with pytest.raises(NotImplementedError):
        align.crop_window(ac.square((500.0, 500.0), np.sqrt(2.0) * size + 1e-9, 0.0), (1000, 1000), size)
    with pytest.raises(NotImplementedError):
        align.crop_window(ac.square((500.0, 500.0), 3.0 * size, 20.0), (1000, 1000), size)
    align.crop_window(ac.square((500.0, 500.0), np.sqrt(2.0) * size - 0.01, 0.0), (1000, 1000), size)      # just below: shrink == 1
    with pytest.raises(NotImplementedError):
        align.crop_window(ac.SMALL_QUADS[0], ac.SMALL_HW, ac.SMALL_S, enable_padding=True)


def test_restatement_equals_pillow_quad():
    """The yardstick itself: float64 numpy == live Pillow, every pixel, inside and outside the image."""
    frames = ac.frames(3, *ac.SMALL_HW)
    for frame, quad in zip(frames, ac.SMALL_QUADS):
        want, sub, passed = ac.pil_crop(frame, quad, ac.SMALL_S)
        got, valid = ac.quad_warp(sub, passed, ac.SMALL_S)
        assert np.array_equal(got, want)
        assert 0.0 < valid.mean() <= 1.0
    assert ac.quad_warp(*ac.pil_crop(frames[2], ac.SMALL_QUADS[2], ac.SMALL_S)[1:], ac.SMALL_S)[1].mean() < 0.7   # the corner quad leaves the frame
    # without the crop, on the whole frame
    passed = ac.SMALL_QUADS[0] + 0.5
    want = np.array(Image.fromarray(frames[0]).transform((96, 96), Image.QUAD, passed.flatten(), Image.BILINEAR))
    assert np.array_equal(ac.quad_warp(frames[0], passed, 96)[0], want)


def test_restatement_equals_pillow_perspective():
    frames = ac.frames(3, *ac.SMALL_HW)
    faces = ac.frames(3, ac.SMALL_S, ac.SMALL_S, seed=1)
    h, w = ac.SMALL_HW
    for face, frame, quad in zip(faces, frames, ac.SMALL_QUADS):
        coeffs = ac.inverse_coefficients(quad, ac.SMALL_S)
        want, alpha = ac.pil_paste(face, frame, coeffs)
        assert set(np.unique(alpha)) <= {0, 255}                        # the composite is a select
        got, valid = ac.perspective_warp(face, coeffs, w, h)
        assert np.array_equal(valid, alpha == 255)
        assert np.array_equal(np.where(valid[..., None], got, frame), want)


def test_float32_coordinates_would_not_pass():
    """Why the kernels compute in fp64: the same statement in float32 breaks the bound the GPU tests set."""
    frames = ac.frames(3, *ac.SMALL_HW)
    shares = []
    for frame, quad in zip(frames, ac.SMALL_QUADS):
        want, sub, passed = ac.pil_crop(frame, quad, ac.SMALL_S)
        shares.append(ac.score(ac.quad_warp(sub, passed, ac.SMALL_S, np.float32)[0], want)[1])
    assert max(shares) > ac.MAX_SHARE, shares


def test_fixture_is_what_pillow_gives_for_the_stored_coefficients(fx):
    """The stored crop / pasted frame follow from the stored inputs and coefficients by the restated arithmetic."""
    frame, crop, pasted = (unz(fx[k]).numpy() for k in ("frame", "crop", "pasted"))
    x0, y0, x1, y1 = fx["window"]
    s = fx["size"]
    passed = fx["quad"].numpy() - np.array([x0, y0], dtype=np.float64) + 0.5
    assert np.array_equal(ac.quad_warp(frame[y0:y1, x0:x1], passed, s)[0], crop)
    got, valid = ac.perspective_warp(255 - crop, fx["inv_coeffs"].numpy(), frame.shape[1], frame.shape[0])
    assert np.array_equal(np.where(valid[..., None], got, frame), pasted)
