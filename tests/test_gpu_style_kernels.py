"""The StyleLoss kernels (csrc/gram.hip: style_prep and its adjoint, gram, gram_mse, gram_grad), each on its own against the fp64
yardsticks of tests/style_cases.py (checked on the CPU by tests/test_style_cases_host.py; the bounds are derived in that module's
docstring).

Per case, where the data are dyadic and the sums exact the output EQUALS the reference (no tolerance), otherwise |got - ref| <= the derived
bound elementwise.  A second call reproduces every output bit for bit; G equals its transpose bit for bit; the accumulate form of
gram_grad equals acc + plain within one rounding; no element of an output or of a workspace is left unwritten, and the elements on either
side of every tensor a wrapper allocates keep their sentinel.  C % 64 != 0 is refused by the return value before any launch."""
import pytest
import torch

import style_cases as sc
from guarded_alloc import DEV, _GuardedTorch, unwritten

pytestmark = pytest.mark.gpu
U = sc.U
_WORST = {}


@pytest.fixture
def guard(monkeypatch):
    from e4s_amd import kernels as K
    g = _GuardedTorch()
    monkeypatch.setattr(K, "torch", g)
    return g


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_WORST):
        print(f"\n[style] largest error / bound of {k}: {_WORST[k]:.3f}", end="")
    print()


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(key, exact, got, ref, bound, what):
    assert got.shape == ref.shape, what
    assert unwritten(got) == 0, f"{what}: {unwritten(got)} elements were never written"
    if exact:
        assert torch.equal(got.cpu(), ref.float()), f"{what}: not equal to the fp64 reference"
        return
    err = (got.cpu().double() - ref).abs()
    live = bound > 0
    if bool(live.any()):
        _WORST[key] = max(_WORST.get(key, 0.0), float((err[live] / bound[live]).max()))
    ok = err <= bound
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements outside the bound, worst error {float(err[~ok].max()):.3e}"


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("index", range(len(sc.GRAM_SHAPES)), ids=[sc.shape_id(s) for s in sc.GRAM_SHAPES])
def test_gram_and_its_gradient_vs_f64(index, kind, guard):
    from e4s_amd import kernels as K
    from e4s_amd import lib
    shape = sc.GRAM_SHAPES[index]
    n, h, w, c = shape
    t = sc.gram_case(index, kind)
    what = f"gram {sc.shape_id(shape)} {kind}"
    assert lib.load().e4s_gram_ws_floats(n, h * w, c) == sc.gram_ws_floats(n, h * w, c), what + ": the restated slice plan is not the library's"
    f = _dev(t["f"])
    G = K.gram(f)
    ws = guard.insides(torch.float32)[-1]
    assert unwritten(ws) == 0, what + ": part of the workspace was never written"
    guard.check()
    _check("gram", sc.gram_exact(shape, kind), G, t["ref"], t["bound"], what)
    assert _same_bits(G, G.t()), what + ": G is not bit-symmetric"
    assert _same_bits(G, K.gram(f)), what + ": second call differs"
    guard.check()

    what = what.replace("gram", "gram_grad")
    d, gloss = _dev(t["d"]), _dev(t["gloss"])
    df = K.gram_grad(f, d, gloss, t["coef"])
    guard.check()
    _check("gram_grad", kind == "dyadic", df, t["grad"], t["grad_bound"], what)
    assert _same_bits(df, K.gram_grad(f, d, gloss, t["coef"])), what + ": second call differs"
    dacc = K.gram_grad(f, d, gloss, t["coef"], addend=_dev(t["acc"]))
    guard.check()
    assert unwritten(dacc) == 0, what
    want = t["acc"].double() + df.cpu().double()
    if kind == "dyadic":
        assert torch.equal(dacc.cpu(), want.float()), what + ": acc + plain is not exact"
    else:
        err, bound = (dacc.cpu().double() - want).abs(), U * (want.abs() + df.cpu().double().abs())
        _WORST["gram_grad (accumulate)"] = max(_WORST.get("gram_grad (accumulate)", 0.0), float((err / bound.clamp(min=1e-300)).max()))
        assert bool((err <= bound).all()), what + ": the accumulate form is more than one rounding from acc + plain"


@pytest.mark.parametrize("shape", sc.GRAM_REFUSED, ids=sc.shape_id)
def test_gram_refuses_channel_counts_it_does_not_tile(shape):
    from e4s_amd import kernels as K
    from e4s_amd import lib
    from e4s_amd.lib import fptr, stream
    n, h, w, c = shape
    L = lib.load()
    assert L.e4s_gram_ws_floats(n, h * w, c) == 0
    f = torch.zeros(shape, device=DEV)
    out = torch.full((n * c, n * c), 7.0, device=DEV)
    ws = torch.full((4096,), 7.0, device=DEV)
    assert L.e4s_gram_f32(fptr(f), fptr(out), fptr(ws), n, h * w, c, stream()) != 0
    g1 = torch.zeros(1, device=DEV)
    assert L.e4s_gram_grad_f32(fptr(f), fptr(out), fptr(g1), 1.0, None, fptr(torch.full(shape, 7.0, device=DEV)), n, h * w, c, stream()) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all()), "a refused call launched something"
    with pytest.raises(ValueError):
        K.gram(f)


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("index", range(len(sc.MSE_SIZES)), ids=[str(s) for s in sc.MSE_SIZES])
def test_gram_mse_vs_f64(index, kind, guard):
    from e4s_amd import kernels as K
    from e4s_amd import lib
    t = sc.mse_case(index, kind)
    n = t["gx"].numel()
    what = f"gram_mse {sc.MSE_SIZES[index]} {kind}"
    assert lib.load().e4s_gram_mse_ws_doubles(n) == sc.mse_blocks(n), what
    gx, gy = _dev(t["gx"]), _dev(t["gy"])
    acc = guard.place(torch.tensor([123.0]))
    term, d = K.gram_mse(gx, gy, acc, t["weight"], init=True)
    ws = guard.insides(torch.float64)[-1]
    assert unwritten(ws) == 0, what + ": part of the workspace was never written"
    guard.check()
    _check("gram_mse D", kind == "dyadic", d, t["d"], t["d_bound"], what)
    tb = torch.tensor([t["term_bound"]], dtype=torch.float64)
    _check("gram_mse term", t["exact"], term, torch.tensor([t["term"]], dtype=torch.float64), tb, what)
    first = float(acc.cpu())
    wt = t["weight"] * float(term.cpu())
    assert first == float(torch.tensor(wt).float()), what + ": init does not overwrite the accumulator"       # weight is a power of two
    term2, d2 = K.gram_mse(gx, gy, acc, t["weight"])
    guard.check()
    assert _same_bits(term, term2) and _same_bits(d, d2), what + ": second call differs"
    second = float(acc.cpu())
    if t["exact"]:
        assert second == 2 * first, what + ": the second launch does not add exactly"
    else:
        assert abs(second - 2 * wt) <= 2 * U * 2 * abs(wt), what


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("index", range(len(sc.PREP_CASES)), ids=[sc.prep_id(c) for c in sc.PREP_CASES])
def test_style_prep_and_its_adjoint_vs_f64(index, kind, guard):
    from e4s_amd import kernels as K
    c = sc.PREP_CASES[index]
    t = sc.prep_case(index, kind)
    x, dy = _dev(t["x"]), _dev(t["dy"].permute(0, 2, 3, 1))
    for (normalize, use_mask), m in t["modes"].items():
        what = f"style_prep {sc.prep_id(c)} normalize={normalize} mask={use_mask} {kind}"
        mask = _dev(t["mask"]) if use_mask else None
        exact = sc.prep_exact(c, kind, normalize, use_mask)
        y = K.style_prep(x, mask, c["dst"], normalize)
        guard.check()
        _check("style_prep", exact, y, m["fwd"].permute(0, 2, 3, 1).contiguous(), m["fwd_bound"].permute(0, 2, 3, 1).contiguous(), what)
        assert _same_bits(y, K.style_prep(x, mask, c["dst"], normalize)), what + ": second call differs"
        what = what.replace("style_prep", "style_prep_bwd")
        dx = K.style_prep_bwd(dy, mask, tuple(x.shape), normalize)
        guard.check()
        _check("style_prep_bwd", exact, dx, m["bwd"], m["bwd_bound"], what)
        assert _same_bits(dx, K.style_prep_bwd(dy, mask, tuple(x.shape), normalize)), what + ": second call differs"
        guard.check()
        # <prep(x) - prep(0), dy> = <x, prep_bwd(dy)> on the kernel's outputs, to the sum of the two bounds
        y0 = K.style_prep(torch.zeros_like(x), mask, c["dst"], normalize)
        lhs = float(((y.cpu().double() - y0.cpu().double()) * dy.cpu().double()).sum())
        rhs = float((t["x"].double() * dx.cpu().double()).sum())
        fb = m["fwd_bound"].permute(0, 2, 3, 1)
        slack = float(((2 * fb + 8 * U * y0.cpu().double().abs()) * dy.cpu().double().abs()).sum() + (t["x"].double().abs() * m["bwd_bound"]).sum()) + 1e-30
        _WORST["style_prep adjoint"] = max(_WORST.get("style_prep adjoint", 0.0), abs(lhs - rhs) / slack)
        assert abs(lhs - rhs) <= slack, what + ": the gradient is not the adjoint of the prep"
        guard.check()
