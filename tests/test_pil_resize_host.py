"""Host side of the device resize (no GPU): the yardstick of tests/test_gpu_pil_resize.py against live Pillow, the product's
coefficient tables against the yardstick, which passes run, crop_image's shrink arithmetic and the temporal smoothing of quads."""
import numpy as np
import pytest

import pil_resize_cases as pc


def _boxes(W, H):
    return (None, pc.fractional_box(W, H))


@pytest.mark.parametrize("name,in_wh,size", pc.CASES, ids=[c[0] for c in pc.CASES])
def test_restatement_equals_pillow(name, in_wh, size):
    """The yardstick testing itself: every pixel, all five filters, with and without a fractional box."""
    img = pc.image(name, *in_wh)
    for resample in pc.FILTERS:
        for box in _boxes(*in_wh):
            got, want = pc.resize(img, size, resample, box), pc.pillow(img, size, resample, box)
            assert got.shape == want.shape and np.array_equal(got, want), (name, int(resample), box, int((got != want).sum()))


@pytest.mark.parametrize("name,in_wh,size", pc.CASES, ids=[c[0] for c in pc.CASES])
def test_product_tables_equal_the_restatement(name, in_wh, size):
    from e4s_amd import resize
    for resample in pc.FILTERS:
        for box in _boxes(*in_wh):
            x0, y0, x1, y1 = (0.0, 0.0) + tuple(float(v) for v in in_wh) if box is None else box
            for n_in, n_out, lo, hi in ((in_wh[0], size[0], x0, x1), (in_wh[1], size[1], y0, y1)):
                bounds, kk = resize.coefficients(n_in, n_out, int(resample), lo, hi)
                wb, wk = pc.coefficients(n_in, n_out, resample, lo, hi)
                assert bounds.dtype == np.int32 and kk.dtype == np.int32
                assert np.array_equal(bounds, wb) and np.array_equal(kk, wk), (name, int(resample), box)


def test_filter_constants_are_pillows():
    from e4s_amd import resize
    assert (resize.NEAREST, resize.LANCZOS, resize.BILINEAR, resize.BICUBIC, resize.BOX, resize.HAMMING) == tuple(
        int(v) for v in (pc.NEAREST, pc.LANCZOS, pc.BILINEAR, pc.BICUBIC, pc.BOX, pc.HAMMING))
    with pytest.raises(ValueError):
        resize.coefficients(8, 4, resize.NEAREST, 0.0, 8.0)


def test_skipped_passes():
    from e4s_amd import resize
    cases = {c[0]: c[1:] for c in pc.CASES}
    assert resize.passes(*cases["identity"]) == (False, False)
    assert resize.passes(*cases["identity"], box=(0, 0, 64, 48)) == (False, False)
    assert resize.passes(*cases["identity"], box=pc.fractional_box(64, 48)) == (True, True)
    assert resize.passes(*cases["y_only"]) == (False, True)
    assert resize.passes(*cases["x_only"]) == (True, False)
    assert resize.passes(*cases["up"]) == (True, True)
    for name, in_wh, size in pc.CASES:
        for box in _boxes(*in_wh):
            assert resize.passes(in_wh, size, box) == pc.passes(in_wh, size, box)


def test_crop_plan_follows_crop_image():
    from e4s_amd import align
    for quad, want_shrink in zip(pc.SHRINK_QUADS, pc.SHRINKS):
        before = quad.copy()
        shrink, rsize, window, q = align.crop_plan(quad, pc.SHRINK_HW, pc.SHRINK_S)
        w_shrink, w_rsize, w_window, w_q = pc.crop_plan(quad, pc.SHRINK_HW, pc.SHRINK_S)
        assert shrink == w_shrink == want_shrink
        assert tuple(rsize) == w_rsize and tuple(int(v) for v in window) == w_window
        assert all(isinstance(v, int) for v in tuple(rsize) + tuple(window))
        assert np.abs(q - w_q).max() <= 1e-12
        assert np.array_equal(quad, before), "crop_plan changed the caller's quad"
        if want_shrink > 1:
            with pytest.raises(NotImplementedError):
                align.crop_window(quad, pc.SHRINK_HW, pc.SHRINK_S)
        else:
            assert tuple(window) == tuple(align.crop_window(quad, pc.SHRINK_HW, pc.SHRINK_S)) and tuple(rsize) == (600, 400)


def _landmarks(n, seed=3):
    """n frames of 68 landmarks: a plausible face that drifts and jitters."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-60, 60, (68, 2))
    base[36:42] = [-40, -30] + rng.uniform(-6, 6, (6, 2))
    base[42:48] = [40, -28] + rng.uniform(-6, 6, (6, 2))
    base[48], base[54] = [-25, 45], [27, 47]
    t = np.arange(n)[:, None, None]
    return base[None] + np.array([500.0, 400.0]) + 3.0 * t + rng.normal(0, 2.5, (n, 68, 2))


def test_compute_quads_without_smoothing_is_compute_quad():
    from e4s_amd import align
    for n in (1, 2, 12):
        lm = _landmarks(n)
        for scale in (1.0, 1.3):
            assert np.array_equal(align.compute_quads(lm, scale), np.stack([align.compute_quad(one, scale) for one in lm]))
    with pytest.raises(ValueError):
        align.compute_quads(_landmarks(3)[0])


@pytest.mark.parametrize("n", (1, 2, 12))
def test_compute_quads_smoothing_follows_scipy(n):
    """crop_faces' lines 191-210 with scipy's own filter; one rounding per tap is all the restated filter may differ by."""
    from scipy.ndimage import gaussian_filter1d
    from e4s_amd import align
    lm, center_sigma, xy_sigma = _landmarks(n), 2.0, 1.5
    cs, xs, ys = (np.stack(v) for v in zip(*(align._transform(one, 1.0) for one in lm)))
    # c, x, y as compute_quad derives them: the unsmoothed stacking is compute_quad's
    assert np.array_equal(np.stack([cs - xs - ys, cs - xs + ys, cs + xs + ys, cs + xs - ys], axis=1), align.compute_quad(lm))
    cs = gaussian_filter1d(cs, sigma=center_sigma, axis=0)
    xs, ys = gaussian_filter1d(xs, sigma=xy_sigma, axis=0), gaussian_filter1d(ys, sigma=xy_sigma, axis=0)
    want = np.stack([cs - xs - ys, cs - xs + ys, cs + xs + ys, cs + xs - ys], axis=1)
    got = align.compute_quads(lm, 1.0, center_sigma=center_sigma, xy_sigma=xy_sigma)
    n_taps = 2 * int(4 * 2.0 + 0.5) + 1
    bound = n_taps * 2.0 ** -52 * np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"n={n}: max |difference| {err:.3e}, bound {bound:.3e}")
    assert got.shape == (n, 4, 2) and err <= bound
    if n > 2:
        assert np.abs(got - align.compute_quad(lm)).max() > 0.1, "the smoothing changed nothing"
