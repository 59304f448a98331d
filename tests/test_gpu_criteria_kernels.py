"""The loss networks' glue (csrc/criteria.hip: adaptive_pool and its gradient, conv_smallcin, its gradient on both routes and col2im,
maxpool3s2 / maxpool2 and their gradients, relu_bwd, lpips_layer and its gradient, cosine and its gradient, norm_bwd_frozen), each on its
own against the fp64 yardsticks of tests/crit_cases.py (checked on the CPU by tests/test_crit_cases_host.py; the bounds are derived in
that module's docstring).

Per case, wherever the reference leaves no arithmetic to the kernel or the data are dyadic the output EQUALS the reference (no
tolerance), otherwise |got - ref| <= the derived bound elementwise.  A second call reproduces every output bit for bit; sample i of a
batch equals the batch-1 call on that sample (every kernel here reduces within one sample); the accumulate forms equal acc + plain
within one rounding; no element of an output or of a used fp64 workspace is left unwritten, and the elements on either side of every
tensor a wrapper allocates keep their sentinel.  Geometry the ABI does not take is refused by its return value before any launch."""
import itertools

import pytest
import torch

import crit_cases as cc
from guarded_alloc import DEV, _GuardedTorch, unwritten

pytestmark = pytest.mark.gpu
U = cc.U
_WORST = {}                 # kernel output -> largest observed error / bound


@pytest.fixture
def guard(monkeypatch):
    from e4s_amd import kernels as K
    g = _GuardedTorch()
    monkeypatch.setattr(K, "torch", g)
    monkeypatch.setattr(K, "PRECISION", "f32")
    return g


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_WORST):
        print(f"\n[criteria] largest error / bound of {k}: {_WORST[k]:.3f}", end="")
    print()


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _ratio(key, err, bound):
    live = bound > 0
    if bool(live.any()):
        _WORST[key] = max(_WORST.get(key, 0.0), float((err[live] / bound[live]).max()))


def _check(key, exact, got, ref, bound, what):
    """exact: got EQUALS the fp64 reference; else |got - ref| <= bound elementwise (0 where the bound is 0)."""
    assert got.shape == ref.shape, what
    assert unwritten(got) == 0, f"{what}: {unwritten(got)} elements were never written"
    if exact:
        assert torch.equal(got.cpu(), ref.float()), f"{what}: not equal to the fp64 reference"
        return
    err = (got.cpu().double() - ref).abs()
    _ratio(key, err, bound)
    ok = err <= bound
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements outside the bound, worst error {float(err[~ok].max()):.3e}"


def _check_acc(key, exact, got, acc, plain, what):
    """the accumulate form against acc + plain (the kernel's own plain result): one rounding, and the plain form's last one if the
    compiler contracts its last product into the addition; exact: the plain form EQUALS its reference, so this one has to as well."""
    assert unwritten(got) == 0, what
    want = acc.double() + plain.cpu().double()
    if exact:
        assert torch.equal(got.cpu(), want.float()), f"{what}: acc + plain is not exact"
        return
    err, bound = (got.cpu().double() - want).abs(), U * (want.abs() + plain.cpu().double().abs())
    _ratio(key + " (accumulate)", err, bound)
    assert bool((err <= bound).all()), f"{what}: the accumulate form is more than one rounding from acc + plain"


# ---- adaptive pooling ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cc.POOL_CASES)), ids=[cc.case_id(c) for c in cc.POOL_CASES])
def test_adaptive_pool_and_its_gradient_vs_f64(index, guard):
    from e4s_amd import kernels as K
    c = cc.POOL_CASES[index]
    crop, dst = c["crop"], c["dst"]
    for kind, C, nchw in itertools.product(cc.KINDS, cc.POOL_C, (True, False)):
        t = cc.pool_case(index, kind, C)
        lay = (lambda v: v.contiguous()) if nchw else _nhwc                                          # NCHW reference -> the image's layout
        x_cpu, acc_cpu = lay(t["x"]), lay(t["acc"])
        x, dy = _dev(x_cpu), _dev(t["dy"])
        shape = tuple(x_cpu.shape)
        for a in cc.AFFINES:
            what = f"adaptive_pool {cc.case_id(c)} C{C} {'nchw' if nchw else 'nhwc'} {a} {kind}"
            scale, shift = (_dev(v) for v in cc._affine(t, a))
            kw = dict(crop=crop, in_nchw=nchw, scale=scale)
            y = K.adaptive_pool(x, dst, shift=shift, **kw)
            guard.check()
            ref, bound = t["fwd"][a]
            _check("adaptive_pool", cc.pool_exact(c, kind, a), y, ref, bound, what)
            assert _same_bits(y, K.adaptive_pool(x, dst, shift=shift, **kw)), what + ": second call differs"
            for i in range(cc.POOL_B):
                assert _same_bits(K.adaptive_pool(x[i:i + 1], dst, shift=shift, **kw)[0], y[i]), what + f": sample {i} depends on the batch"
            guard.check()
            if a == "scale_shift":          # the gradient takes no shift
                continue
            what = what.replace("adaptive_pool", "adaptive_pool_bwd")
            dref, dbound, inside = t["bwd"][a]
            exact = cc.pool_exact(c, kind, a, bwd=True)
            dx = K.adaptive_pool_bwd(dy, shape, **kw)
            guard.check()
            _check("adaptive_pool_bwd", exact, dx, lay(dref), lay(dbound), what)
            assert _same_bits(dx, K.adaptive_pool_bwd(dy, shape, **kw)), what + ": second call differs"
            for i in range(cc.POOL_B):
                assert _same_bits(K.adaptive_pool_bwd(dy[i:i + 1], (1,) + shape[1:], **kw)[0], dx[i]), what + f": sample {i} depends on the batch"
            dacc = K.adaptive_pool_bwd(dy, shape, dx_acc=guard.place(acc_cpu), **kw)
            guard.check()
            _check_acc("adaptive_pool_bwd", exact and kind == "dyadic", dacc, acc_cpu, dx, what)
            out = ~lay(inside.expand(cc.POOL_B, C, *inside.shape))
            assert float(dx.cpu()[out].abs().max() if out.any() else 0) == 0, what + ": a pixel outside the crop has a gradient"
            assert _same_bits(dacc.cpu()[out], acc_cpu[out]), what + ": a pixel outside the crop lost its accumulated value"
            # <pool(x), dy> = <x, pool_bwd(dy)> on the kernel's outputs, to the sum of the two bounds
            lhs, rhs = float((y.cpu().double() * t["dy"].double()).sum()), float((x_cpu.double() * dx.cpu().double()).sum())
            slack = float((bound * t["dy"].double().abs()).sum() + (x_cpu.double().abs() * lay(dbound)).sum())
            _WORST["adaptive_pool adjoint"] = max(_WORST.get("adaptive_pool adjoint", 0.0), abs(lhs - rhs) / slack)
            assert abs(lhs - rhs) <= slack, what + ": the gradient is not the adjoint of the pool"
            guard.check()


# ---- stem convs ------------------------------------------------------------------------------------------------------------------------------
def _conv_bwd_direct(guard, name, src, wp, c, extra=()):
    from e4s_amd.lib import call, fptr, stream
    ho, wo = cc.conv_out(c)
    dx = guard.empty(c["B"], c["Hi"], c["Wi"], c["Cin"], device=DEV)
    ops = (fptr(src), fptr(wp), fptr(dx)) if wp is not None else (fptr(src), fptr(dx))
    call(name, *ops, c["B"], c["Hi"], c["Wi"], c["Cin"], ho, wo, *extra, c["k"], c["stride"], c["pad"], stream())
    guard.check()
    return dx


def _conv_gradients(guard, t, kind, what):
    """both routes of the image gradient and col2im on its own, against fp64 autograd of F.conv2d"""
    from e4s_amd import kernels as K
    c = t["case"]
    k, s, p = c["k"], c["stride"], c["pad"]
    shape = (c["B"], c["Hi"], c["Wi"], c["Cin"])
    wp, dy, z = K.pack_smallcin(_dev(t["w"])), _dev(t["dy"]), _dev(t["z"])
    ref, bound = t["bwd"]
    pixel = _conv_bwd_direct(guard, "e4s_conv_smallcin_bwd_f32", dy, wp, c, (c["Cout"],))
    _check("conv_smallcin_bwd (per pixel)", t["exact"], pixel, ref, bound, what + " per-pixel route")
    assert _same_bits(pixel, _conv_bwd_direct(guard, "e4s_conv_smallcin_bwd_f32", dy, wp, c, (c["Cout"],))), what + ": second call differs"
    routed = K.conv_smallcin_bwd(dy, wp, shape, k, s, p)
    guard.check()
    if cc.conv_gemm_route(c):
        _check("conv_smallcin_bwd (GEMM + col2im)", t["exact"], routed, ref, bound, what + " GEMM route")
        again = K.conv_smallcin_bwd(dy, wp, shape, k, s, p, cache={})
        guard.check()
        assert _same_bits(routed, again), what + ": second call differs"
    else:
        assert _same_bits(routed, pixel), what + ": K.conv_smallcin_bwd is not the per-pixel kernel here"
    cref, cbound = t["col2im"]
    folded = _conv_bwd_direct(guard, "e4s_conv_smallcin_col2im_f32", z, None, c, (z.shape[3],))
    _check("conv_smallcin_col2im", t["exact"], folded, cref, cbound, what + " col2im of a hand-made z")
    assert _same_bits(folded, _conv_bwd_direct(guard, "e4s_conv_smallcin_col2im_f32", z, None, c, (z.shape[3],))), what + ": second call differs"
    if c["B"] > 1:
        c1 = dict(c, B=1)
        for i in range(c["B"]):
            assert _same_bits(_conv_bwd_direct(guard, "e4s_conv_smallcin_bwd_f32", dy[i:i + 1].contiguous(), wp, c1, (c["Cout"],))[0], pixel[i]), what
            assert _same_bits(_conv_bwd_direct(guard, "e4s_conv_smallcin_col2im_f32", z[i:i + 1].contiguous(), None, c1, (z.shape[3],))[0], folded[i]), what


@pytest.mark.parametrize("index", range(len(cc.CONV_CASES)), ids=[cc.case_id(c) for c in cc.CONV_CASES])
def test_conv_smallcin_and_its_gradient_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in cc.KINDS:
        t = cc.conv_case(index, kind)
        c = t["case"]
        what = f"conv_smallcin {cc.case_id(c)} {kind}"
        x, wp, bias = _dev(t["x"]), K.pack_smallcin(_dev(t["w"])), _dev(t["bias"])
        for (has_bias, relu), (ref, bound, pad_only) in t["fwd"].items():
            w2 = f"{what} bias{int(has_bias)} relu{int(relu)}"
            args = (wp, bias if has_bias else None, c["Cout"], c["k"], c["stride"], c["pad"])
            y = K.conv_smallcin(x, *args, relu=relu)
            guard.check()
            _check("conv_smallcin", t["exact"], y, ref, bound, w2)
            if bool(pad_only.any()):
                assert torch.equal(y.cpu()[pad_only], ref.float()[pad_only]), w2 + ": an output wholly in the padding is not the bias"
            assert _same_bits(y, K.conv_smallcin(x, *args, relu=relu)), w2 + ": second call differs"
            for i in range(c["B"] if c["B"] > 1 else 0):
                assert _same_bits(K.conv_smallcin(x[i:i + 1], *args, relu=relu)[0], y[i]), w2 + f": sample {i} depends on the batch"
            guard.check()
        _conv_gradients(guard, t, kind, what.replace("conv_smallcin", "conv_smallcin_bwd"))


@pytest.mark.parametrize("index", range(len(cc.CONV_BWD_ONLY)), ids=[cc.case_id(c) for c in cc.CONV_BWD_ONLY])
def test_conv_smallcin_gradient_of_a_hand_made_dy(index, guard):
    for kind in cc.KINDS:
        t = cc.conv_case(index, kind, True)
        _conv_gradients(guard, t, kind, f"conv_smallcin_bwd {cc.case_id(t['case'])} {kind}")


# ---- max pools, relu -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, index", [(n, i) for n in ("maxpool3s2", "maxpool2") for i in range(len(cc.MP_CASES[n]))],
                         ids=[f"{n}-{cc.case_id(c)}" for n in ("maxpool3s2", "maxpool2") for c in cc.MP_CASES[n]])
def test_maxpool_values_indices_and_gradient(name, index, guard):
    from e4s_amd import kernels as K
    fwd, bwd = getattr(K, name), getattr(K, name + "_bwd")
    for kind in cc.MP_KINDS:
        t = cc.maxpool_case(name, index, kind)
        c = t["case"]
        what = f"{name} {cc.case_id(c)} {kind}"
        x, dy = _dev(t["x"]), _dev(t["dy"])
        shape = tuple(x.shape)
        y, idx = fwd(x)
        guard.check()
        _check(name, True, y, t["y"], None, what)
        assert idx.dtype == torch.uint8 and unwritten(idx) == 0, what + ": an index was never written"
        assert torch.equal(idx.cpu(), t["code"]), what + ": not ATen's first maximum"
        y2, idx2 = fwd(x)
        assert _same_bits(y, y2) and _same_bits(idx, idx2), what + ": second call differs"
        dx = bwd(dy, idx, shape)
        guard.check()
        _check(name + "_bwd", t["exact_bwd"], dx, t["dx"], t["bound"], what + " gradient")
        assert _same_bits(dx, bwd(dy, idx, shape)), what + ": second call differs"
        for i in range(c["B"] if c["B"] > 1 else 0):
            yi, ii = fwd(x[i:i + 1])
            assert _same_bits(yi[0], y[i]) and _same_bits(ii[0], idx[i]), what + f": sample {i} depends on the batch"
            assert _same_bits(bwd(dy[i:i + 1], ii, (1,) + shape[1:])[0], dx[i]), what + f": sample {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(cc.RELU_CASES)), ids=[f"n{n}" for n in cc.RELU_CASES])
def test_relu_bwd_is_exact(index, guard):
    from e4s_amd import kernels as K
    for kind in cc.KINDS:
        t = cc.relu_case(index, kind)
        y, dy = _dev(t["y"]), _dev(t["dy"])
        dx = K.relu_bwd(dy, y)
        guard.check()
        assert unwritten(dx) == 0 and torch.equal(dx.cpu(), t["ref"]), f"relu_bwd n{t['n']} {kind}"
        dacc = K.relu_bwd(dy, y, dx_acc=guard.place(t["acc"]))
        guard.check()
        assert torch.equal(dacc.cpu(), t["ref_acc"]), f"relu_bwd n{t['n']} {kind}: accumulate"
        assert _same_bits(dx, K.relu_bwd(dy, y)), "second call differs"
        guard.check()


# ---- LPIPS ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cc.LPIPS_CASES)), ids=[cc.case_id(c) for c in cc.LPIPS_CASES])
def test_lpips_layer_and_its_gradient_vs_f64(index, guard):
    from e4s_amd import kernels as K
    c = cc.LPIPS_CASES[index]
    B, HW = c["B"], c["h"] * c["w"]
    gout = torch.tensor([cc.LPIPS_GOUT], device=DEV)
    for kind in cc.KINDS:
        t = cc.lpips_case(index, kind)
        what = f"lpips_layer {cc.case_id(c)} {kind}"
        fx, fy, w = _dev(t["fx"]), _dev(t["fy"]), _dev(t["w"])
        out = K.lpips_layer(fx, fy, w)
        ws = guard.insides(torch.float64)[-1]
        assert ws.numel() == B * -(-HW // 16) and unwritten(ws) == 0, what + ": a slot of the fp64 workspace was never written"
        guard.check()
        _check("lpips_layer", False, out, *t["fwd"], what)
        assert _same_bits(out, K.lpips_layer(fx, fy, w)), what + ": second call differs"
        dfx = K.lpips_layer_bwd(fx, fy, w, gout, cc.LPIPS_GMUL)
        guard.check()
        _check("lpips_layer_bwd", False, dfx, *t["bwd"], what + " gradient")
        if t["special"] is not None:          # the deliberate deviation from torch autograd: dn / eps where fx is all zero, 0 where both are
            flat = dfx.cpu().view(B, HW, -1)
            assert bool(torch.isfinite(flat).all()) and float(flat[:, t["special"][0]].abs().max()) > 1e6, what
            assert float(flat[:, t["special"][2]].abs().max()) == 0, what
        assert _same_bits(dfx, K.lpips_layer_bwd(fx, fy, w, gout, cc.LPIPS_GMUL)), what + ": second call differs"
        dacc = K.lpips_layer_bwd(fx, fy, w, gout, cc.LPIPS_GMUL, dfx_acc=guard.place(t["acc"]))
        guard.check()
        _check_acc("lpips_layer_bwd", False, dacc, t["acc"], dfx, what)
        for i in range(B if B > 1 else 0):          # the pixel order within a sample does not depend on B
            assert _same_bits(K.lpips_layer(fx[i:i + 1], fy[i:i + 1], w), out[i:i + 1]), what + f": sample {i} depends on the batch"
            assert _same_bits(K.lpips_layer_bwd(fx[i:i + 1], fy[i:i + 1], w, gout, cc.LPIPS_GMUL)[0], dfx[i]), what + f": sample {i}"
        guard.check()


# ---- cosine, frozen norm -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cc.COS_CASES)), ids=[cc.case_id(c) for c in cc.COS_CASES])
def test_cosine_and_its_gradient_vs_f64(index, guard):
    from e4s_amd import kernels as K, lib
    c = cc.COS_CASES[index]
    B, D = c["B"], c["D"]
    gout = torch.tensor([cc.COS_GOUT], device=DEV)
    for kind in cc.KINDS:
        t = cc.cosine_case(index, kind)
        what = f"cosine {cc.case_id(c)} {kind}"
        a, b = _dev(t["a"]), _dev(t["b"])
        coef = K.cosine(a, b)
        ws = guard.insides(torch.float64)[-1]
        assert ws.numel() == lib.load().e4s_cosine_ws_doubles(B, D) == 3 * B * cc.cos_nchunk(D), what + ": workspace size"
        assert unwritten(ws) == 0, what + ": a slot of the fp64 workspace was never written"
        guard.check()
        _check("cosine", False, coef, t["vals"], t["bounds"], what)
        assert _same_bits(coef, K.cosine(a, b)), what + ": second call differs"
        da = K.cosine_bwd(a, b, coef, gout, cc.COS_GMUL)
        guard.check()
        _check("cosine_bwd", False, da, *cc.cosine_bwd_ref(t["a"], t["b"], coef.cpu(), cc.COS_GOUT, cc.COS_GMUL), what + " gradient")
        assert _same_bits(da, K.cosine_bwd(a, b, coef, gout, cc.COS_GMUL)), what + ": second call differs"
        dacc = K.cosine_bwd(a, b, coef, gout, cc.COS_GMUL, da_acc=guard.place(t["acc"]))
        guard.check()
        _check_acc("cosine_bwd", False, dacc, t["acc"], da, what)
        for i in range(B if B > 1 else 0):          # the chunk order within a row does not depend on B
            ci = K.cosine(a[i:i + 1], b[i:i + 1])
            assert _same_bits(ci[0], coef[i]), what + f": row {i} depends on the batch"
            assert _same_bits(K.cosine_bwd(a[i:i + 1], b[i:i + 1], ci, gout, cc.COS_GMUL)[0], da[i]), what + f": row {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(cc.NORM_CASES)), ids=[cc.case_id(c) for c in cc.NORM_CASES])
def test_norm_bwd_frozen_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in cc.KINDS:
        t = cc.norm_case(index, kind)
        c = t["case"]
        dy, stats = _dev(t["dy"]), _dev(t["stats"])
        for og, oe in cc.NORM_OPTIONS:
            what = f"norm_bwd_frozen {cc.case_id(c)} gate{int(og)} extra{int(oe)} {kind}"
            gate, extra = _dev(t["gate"]) if og else None, _dev(t["extra"]) if oe else None
            dx = K.norm_bwd_frozen(dy, stats, gate=gate, extra=extra)
            guard.check()
            _check("norm_bwd_frozen", t["exact"], dx, *t["ref"][(og, oe)], what)
            assert _same_bits(dx, K.norm_bwd_frozen(dy, stats, gate=gate, extra=extra)), what + ": second call differs"
            dacc = K.norm_bwd_frozen(dy, stats, gate=gate, extra=extra, dx_acc=guard.place(t["acc"]))
            guard.check()
            _check_acc("norm_bwd_frozen", t["exact"], dacc, t["acc"], dx, what)
            for i in range(c["B"] if c["B"] > 1 else 0):
                gi, ei = (None if v is None else v[i:i + 1] for v in (gate, extra))
                assert _same_bits(K.norm_bwd_frozen(dy[i:i + 1], stats[i:i + 1], gate=gi, extra=ei)[0], dx[i]), what + f": sample {i}"
            guard.check()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_geometry_outside_the_kernels_sets_is_refused_before_any_launch(guard):
    """Every call returns an error code and leaves its (guarded) outputs as they were: no such kernel ever runs."""
    from e4s_amd import lib
    from e4s_amd.lib import fptr, ptr, stream
    L = lib.load()
    f = lambda n: torch.zeros(n, device=DEV)                                                           # noqa: E731
    src, src8 = f(1 << 16), torch.zeros(1 << 12, device=DEV, dtype=torch.uint8)
    out = lambda: fptr(guard.empty(1 << 12, device=DEV))                                               # noqa: E731
    out8 = lambda: ptr(guard.empty(1 << 12, device=DEV, dtype=torch.uint8))                            # noqa: E731
    ws = lambda: ptr(guard.empty(64, device=DEV, dtype=torch.float64))                                 # noqa: E731
    x, st = fptr(src), stream()

    def pool(y0, x0, hc, wc, ho, wo):          # an 8 x 8 image of 3 channels, both entry points
        return [lambda: L.e4s_adaptive_pool_f32(x, out(), 1, 3, 8, 8, y0, x0, hc, wc, ho, wo, 1, None, None, st),
                lambda: L.e4s_adaptive_pool_bwd_f32(x, out(), 1, 3, 8, 8, y0, x0, hc, wc, ho, wo, 1, None, 0, st)]

    def stem(cin, cout_f, cout_b, k, s, p, ho, wo):          # an 8 x 8 image; cout_f / cout_b None: that direction is not asked
        calls = []
        if cout_f is not None:
            calls.append(lambda: L.e4s_conv_smallcin_f32(x, x, None, out(), 1, 8, 8, cin, ho, wo, cout_f, k, s, p, 0, st))
        if cout_b is not None:
            calls.append(lambda: L.e4s_conv_smallcin_bwd_f32(x, x, out(), 1, 8, 8, cin, ho, wo, cout_b, k, s, p, st))
        return calls

    refused = (
        pool(2, 0, 7, 8, 4, 4) + pool(0, 2, 8, 7, 4, 4)                # a crop past the image
        + pool(-1, 0, 4, 4, 4, 4) + pool(0, -1, 4, 4, 4, 4)            # a negative origin
        + pool(0, 0, 8, 8, 0, 4) + pool(0, 0, 8, 8, 4, 0)              # Ho = 0
        + stem(5, 16, 16, 3, 1, 1, 8, 8)                               # Cin = 5
        + stem(3, 24, None, 3, 1, 1, 8, 8)                             # forward Cout = 24
        + stem(3, None, 18, 3, 1, 1, 8, 8)                             # backward Cout = 18
        + stem(3, 16, 16, 0, 1, 1, 8, 8)                               # k = 0
        + stem(3, 16, 16, 3, 0, 1, 8, 8)                               # stride = 0
        + stem(3, 16, 16, 3, 1, 1, 7, 7) + stem(3, 16, 16, 3, 1, -1, 4, 4)          # an output grid that is not the geometry's; pad < 0
        + [lambda: L.e4s_conv_smallcin_f32(x, x, None, out(), 1, 16, 16, 4, 3, 3, 96, 11, 4, 2, 0, st),          # 185856 B of weights: over the LDS limit
           lambda: L.e4s_conv_smallcin_col2im_f32(x, out(), 1, 8, 8, 3, 8, 8, 26, 3, 1, 1, st),                # ZC < k k Cin
           lambda: L.e4s_conv_smallcin_col2im_f32(x, out(), 1, 8, 8, 3, 7, 7, 32, 3, 1, 1, st),
           lambda: L.e4s_maxpool3s2_f32(x, out(), out8(), 1, 8, 8, 6, st),                                      # C = 6
           lambda: L.e4s_maxpool3s2_bwd_f32(x, ptr(src8), out(), 1, 8, 8, 6, st),
           lambda: L.e4s_maxpool2_f32(x, out(), out8(), 1, 8, 8, 6, st),
           lambda: L.e4s_maxpool2_bwd_f32(x, ptr(src8), out(), 1, 8, 8, 6, st),
           lambda: L.e4s_maxpool3s2_f32(x, out(), out8(), 1, 2, 8, 4, st),                                      # H = 2 for the 3 x 3 pool
           lambda: L.e4s_maxpool3s2_bwd_f32(x, ptr(src8), out(), 1, 2, 8, 4, st),
           lambda: L.e4s_relu_bwd_f32(x, x, out(), 6, 0, st),                                                   # n = 6
           lambda: L.e4s_lpips_layer_f32(x, x, x, out(), ws(), 1, 4, 513, st),                                  # C = 513
           lambda: L.e4s_lpips_layer_bwd_f32(x, x, x, x, 1.0, out(), 1, 4, 513, 0, st),
           lambda: L.e4s_lpips_layer_f32(x, x, x, out(), ws(), 1, 4, 0, st),                                    # C = 0
           lambda: L.e4s_lpips_layer_bwd_f32(x, x, x, x, 1.0, out(), 1, 4, 0, 0, st),
           lambda: L.e4s_lpips_layer_f32(x, x, x, out(), ws(), 1, 0, 64, st),                                   # HW = 0
           lambda: L.e4s_lpips_layer_bwd_f32(x, x, x, x, 1.0, out(), 1, 0, 64, 0, st),
           lambda: L.e4s_cosine_f32(x, x, out(), ws(), 1, 0, st),                                               # D = 0
           lambda: L.e4s_cosine_bwd_f32(x, x, x, x, 1.0, out(), 1, 0, 0, st),
           lambda: L.e4s_norm_bwd_frozen_f32(x, x, None, None, out(), 1, 4, 6, 0, st)])                         # C = 6
    for n, call_ in enumerate(refused):
        assert call_() != 0, f"refusal {n}: the call was accepted"
        torch.cuda.synchronize()
        for dt in (torch.float32, torch.float64, torch.uint8):
            for buf in guard.insides(dt):
                assert unwritten(buf) == buf.numel(), f"refusal {n}: a refused call wrote to a tensor"
        guard.check()
    # the neighbours of the refused geometry are taken
    assert L.e4s_adaptive_pool_f32(x, out(), 1, 3, 8, 8, 1, 0, 7, 8, 4, 4, 1, None, None, st) == 0
    assert L.e4s_conv_smallcin_bwd_f32(x, x, out(), 1, 8, 8, 3, 8, 8, 20, 3, 1, 1, st) == 0
    assert L.e4s_conv_smallcin_col2im_f32(x, out(), 1, 8, 8, 3, 8, 8, 27, 3, 1, 1, st) == 0
    assert L.e4s_lpips_layer_f32(x, x, x, out(), ws(), 1, 4, 512, st) == 0
    guard.check()
