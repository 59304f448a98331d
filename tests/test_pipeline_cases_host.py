"""Host checks of the yardsticks in tests/pipeline_cases.py (no GPU): the closed form of the anti-aliased x4 reduction against the two
scipy calls scikit-image 0.20 makes, and the properties that pin the enlargement to OpenCV's non-exact 8-bit INTER_LINEAR path."""
import numpy as np
import pytest

import pipeline_cases as pc


def _img(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


@pytest.mark.parametrize("shape", [(8, 12), (24, 32), (28, 36)])
def test_closed_form_of_the_aa4_resize_equals_the_scipy_calls(shape):
    img = _img(*shape, seed=1)
    want, got = pc.resize_aa4_scipy(img), pc.resize_aa4_closed(img)
    assert got.shape == want.shape == (shape[0] // 4, shape[1] // 4, 3)
    err = float(np.abs(got - want).max())
    print(f"closed form vs scipy at {shape}: {err:.2e}")
    assert err <= 1e-15
    taps = pc.aa4_taps()
    assert taps.shape == (14,) and abs(taps.sum() - 1.0) < 1e-15 and np.array_equal(taps, taps[::-1])


def test_enlargement_is_the_non_exact_path_within_one_level_of_the_rounded_value():
    img = _img(16, 20, seed=2)
    got, exact = pc.cv_resize_x4(img).astype(np.int64), pc.bilinear_x4_rounded(img).astype(np.int64)
    assert got.shape == (64, 80, 3)
    d = np.abs(got - exact)
    print(f"OpenCV formula vs floor(exact + 0.5): {float((d != 0).mean()):.3f} of the pixels differ, max {int(d.max())}")
    assert int(d.max()) == 1                                   # within one level, and it does differ somewhere


def test_enlargement_coefficients_for_x4():
    for n in (5, 7, 64):
        s, c0, c1 = pc.cv_linear_coeffs(n, 4 * n)
        inner = slice(2, 4 * n - 2)                            # the first and last two destinations are clamped
        pairs = {(int(a), int(b)) for a, b in zip(c0[inner], c1[inner])}
        assert pairs == {(1792, 256), (1280, 768), (768, 1280), (256, 1792)}
        assert [(int(a), int(b)) for a, b in zip(c0[2:6], c1[2:6])] == [(1792, 256), (1280, 768), (768, 1280), (256, 1792)]
        assert list(s[:6]) == [0, 0, 0, 0, 0, 0] and list(c1[:2]) == [0, 0]
        assert list(s[-2:]) == [n - 1, n - 1] and list(c1[-2:]) == [0, 0] and list(s[-4:-2]) == [n - 2, n - 2]
        assert np.all(c0 + c1 == 2048)


def test_enlargement_replicates_the_border_rows_and_columns_of_a_5_by_7_image():
    img = _img(5, 7, seed=3)
    big = pc.cv_resize_x4(img)
    assert big.shape == (20, 28, 3)
    for r in (0, 1):                                           # s < 0: the first sample alone
        assert np.array_equal(big[r], big[0]) and np.array_equal(big[:, r], big[:, 0])
        assert np.array_equal(big[-1 - r], big[-1]) and np.array_equal(big[:, -1 - r], big[:, -1])
    assert np.array_equal(big[0, 0], img[0, 0]) and np.array_equal(big[-1, -1], img[-1, -1])
    assert np.array_equal(big[0, -1], img[0, -1]) and np.array_equal(big[-1, 0], img[-1, 0])
    assert not np.array_equal(big[2], big[1])                  # the third row already mixes two source rows


def test_truncation_of_every_level_and_of_one():
    k = np.arange(256)
    p = (k / 255.0).astype(np.float32)
    got = pc.truncate_u8(p)
    prod = p * np.float32(255)
    assert np.array_equal(got, np.floor(prod).astype(np.uint8))
    assert np.array_equal(got, k)                                          # the fp32 product of fp32(k / 255) and 255 is exactly k
    under = pc.truncate_u8(np.nextafter(p[1:], np.float32(0)) - np.float32(1e-6))
    assert np.array_equal(under, k[1:] - 1)                                # just below a level: truncated, where rounding gives k
    assert np.array_equal(np.rint((np.nextafter(p[1:], np.float32(0)) - np.float32(1e-6)) * np.float32(255)).astype(np.uint8), k[1:])
    assert pc.truncate_u8(np.float32(1.0)) == 255 and pc.truncate_u8(np.float32(0.0)) == 0
    assert pc.truncate_u8(np.float32(0.999)) == 254


def test_to_net_statement_is_the_plain_formula_in_fp32():
    img = _img(6, 6, seed=4)[None]
    got = pc.to_net_torch(img).numpy()
    want = ((img.astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)).transpose(0, 3, 1, 2)
    assert got.dtype == np.float32 and np.array_equal(got, want)
