"""The fp64 yardsticks of tests/style_cases.py, checked on the CPU: each bound holds for the same formula evaluated in fp32 by ATen, the
`exact` predicates hold bit for bit, the closed-form Gram gradient is fp64 autograd's, the prep adjoint is the transpose of the prep map,
and the restated launch geometry is consistent."""
import pytest
import torch

import style_cases as sc


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("index", range(len(sc.GRAM_SHAPES)), ids=[sc.shape_id(s) for s in sc.GRAM_SHAPES])
def test_gram_yardstick(index, kind):
    t = sc.gram_case(index, kind)
    shape = sc.GRAM_SHAPES[index]
    got = sc.gram_ref(t["f"]).double()                                  # the same formula in fp32
    if sc.gram_exact(shape, kind):
        assert torch.equal(got, t["ref"])
    else:
        assert bool(((got - t["ref"]).abs() <= t["bound"]).all())
    assert torch.equal(t["ref"], t["ref"].t())
    assert torch.equal(t["d"], t["d"].t())
    s = float(t["gloss"].double()) * t["coef"]
    auto = sc.gram_grad_autograd(t["f"], t["d"], s)
    assert float((auto - t["grad"]).abs().max()) <= 1e-12 * max(float(t["grad"].abs().max()), 1e-30)
    n, h, w, c = shape
    a = sc._rows(t["f"])
    g32 = (torch.mm(t["d"], a) * torch.tensor(s).float()).reshape(n, c, h, w).permute(0, 2, 3, 1).double()
    if kind == "dyadic":
        assert torch.equal(g32, t["grad"])
    else:
        assert bool(((g32 - t["grad"]).abs() <= t["grad_bound"] + sc.U * t["grad"].abs()).all())


@pytest.mark.parametrize("shape", sc.GRAM_SHAPES + [(2, 256, 256, 64), (2, 32, 32, 512), (2, 128, 128, 128), (2, 64, 64, 256)], ids=sc.shape_id)
def test_gram_slices_cover_the_pixels(shape):
    n, h, w, c = shape
    ntile, nsplit, chunk = sc.gram_slices(n, h * w, c)
    assert chunk % 2 == 0 and (nsplit - 1) * chunk < h * w <= nsplit * chunk
    assert ntile == (n * c // 64) * (n * c // 64 + 1) // 2
    if shape not in sc.GRAM_SHAPES:                                 # the four taps of a batch-2 step at 256^2
        assert 512 <= ntile * nsplit <= 2048                        # about one wave per SIMD of 256 CUs at both ends of the shape range


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("index", range(len(sc.MSE_SIZES)))
def test_gram_mse_yardstick(index, kind):
    t = sc.mse_case(index, kind)
    d32 = t["gx"] - t["gy"]
    assert bool(((d32.double() - t["d"]).abs() <= t["d_bound"]).all())
    term32 = float((d32 * d32).mean())
    if t["exact"]:
        assert torch.equal(d32.double(), t["d"]) and term32 == t["term"]
    else:
        assert abs(term32 - t["term"]) <= t["term_bound"] + 64 * sc.U * t["term"]      # ATen's fp32 mean is a pairwise sum, not the kernel's


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("index", range(len(sc.PREP_CASES)), ids=[sc.prep_id(c) for c in sc.PREP_CASES])
def test_prep_yardstick(index, kind):
    c = sc.PREP_CASES[index]
    t = sc.prep_case(index, kind)
    for (normalize, use_mask), m in t["modes"].items():
        what = f"{sc.prep_id(c)} normalize={normalize} mask={use_mask} {kind}"
        x = t["x"].clone().requires_grad_(True)
        got = sc.prep_ref(x, t["mask"] if use_mask else None, c["dst"], normalize)
        got.backward(t["dy"])
        if sc.prep_exact(c, kind, normalize, use_mask):
            assert torch.equal(got.detach().double(), m["fwd"]), what
            assert torch.equal(x.grad.double(), m["bwd"]), what
        else:
            assert bool(((got.detach().double() - m["fwd"]).abs() <= m["fwd_bound"]).all()), what
            assert bool(((x.grad.double() - m["bwd"]).abs() <= m["bwd_bound"]).all()), what
        # <prep(x), y> = <x, prep^T(y)> minus the affine part of the normalisation, in fp64
        zero = sc.prep_ref(torch.zeros_like(t["x"]).double(), t["mask"].double() if use_mask else None, c["dst"], normalize)
        lhs = float(((m["fwd"] - zero) * t["dy"].double()).sum())
        rhs = float((t["x"].double() * m["bwd"]).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), what
    if index == 0:
        mres = torch.nn.functional.interpolate(t["mask"].double(), size=c["dst"], mode="bilinear")
        assert bool((mres == 0).any()) and bool((mres == 1).any()) and bool(((mres > 0) & (mres < 1)).any())
