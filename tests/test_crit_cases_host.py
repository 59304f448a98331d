"""The yardsticks of tests/test_gpu_criteria_kernels.py checked on the CPU, before any kernel is involved (tests/crit_cases.py): every
reference against an independent fp64 statement, every bound against the same formula evaluated in fp32, every case declared exact
evaluated in fp32, the paths the case lists reach, and the bin range of the pool gradient against a search over every bin."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import crit_cases as cc

U = cc.U
KINDS = cc.KINDS


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _same(a32, ref64):
    assert a32.dtype == torch.float32 and ref64.dtype == torch.float64
    return torch.equal(a32.double(), ref64)


def _inside(got32, ref, bound, what):
    err = (got32.double() - ref).abs()
    assert bool((err <= bound).all()), f"{what}: fp32 evaluation outside the bound, worst ratio {float((err / bound.clamp(min=1e-300)).max()):.3f}"


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- adaptive pooling ----------------------------------------------------------------------------------------------------------------------
def _pool_loops(x, c, scale, shift, dy):
    """the pool and its gradient by explicit loops over the bins, fp64, NCHW in, (y NHWC, dx NCHW)"""
    y0, x0, hc, wc = cc.pool_crop(c)
    ho, wo = c["dst"]
    xd = x.double()
    B, C = xd.shape[:2]
    y, dx = torch.zeros(B, ho, wo, C, dtype=torch.float64), torch.zeros_like(xd)
    s = torch.ones(C, dtype=torch.float64) if scale is None else scale.double()
    sh = torch.zeros(C, dtype=torch.float64) if shift is None else shift.double()
    for oy, (ys, ye) in enumerate(cc.bins(hc, ho)):
        for ox, (xs, xe) in enumerate(cc.bins(wc, wo)):
            area = (ye - ys) * (xe - xs)
            y[:, oy, ox] = xd[:, :, y0 + ys:y0 + ye, x0 + xs:x0 + xe].sum((2, 3)) / area * s + sh
            dx[:, :, y0 + ys:y0 + ye, x0 + xs:x0 + xe] += (dy[:, oy, ox].double() * s / area)[:, :, None, None]
    return y, dx


@pytest.mark.parametrize("index", range(len(cc.POOL_CASES)), ids=[cc.case_id(c) for c in cc.POOL_CASES])
def test_pool_refs_are_loops_over_the_bins_and_fp32_stays_inside(index):
    c = cc.POOL_CASES[index]
    y0, x0, hc, wc = cc.pool_crop(c)
    for kind in KINDS:
        for C in cc.POOL_C:
            t = cc.pool_case(index, kind, C)
            for a in cc.AFFINES:
                scale, shift = cc._affine(t, a)
                (y, yb), (dx, db, inside) = t["fwd"][a], t["bwd"][a]
                wy, wdx = _pool_loops(t["x"], c, scale, shift, t["dy"])
                assert _rel(y, wy) < 1e-13 and float((dx - wdx).abs().max()) < 1e-13 and (yb >= 0).all()
                assert float(dx[:, :, ~inside].abs().max() if (~inside).any() else 0) == 0 and float(db[:, :, ~inside].sum() if (~inside).any() else 0) == 0
                # the same operations in fp32
                xc = t["x"][:, :, y0:y0 + hc, x0:x0 + wc].clone().requires_grad_(True)
                v = F.adaptive_avg_pool2d(xc, c["dst"])
                if scale is not None:
                    v = v * scale.view(1, -1, 1, 1)
                g32 = torch.autograd.grad((v * _nchw(t["dy"])).sum(), xc)[0]
                if shift is not None:
                    v = v + shift.view(1, -1, 1, 1)
                y32 = _nhwc(v.detach())
                what = f"{cc.case_id(c)} C{C} {a} {kind}"
                if cc.pool_exact(c, kind, a):
                    assert _same(y32, y), what
                else:
                    _inside(y32, y, yb, what)
                dxc, dbc = dx[:, :, y0:y0 + hc, x0:x0 + wc], db[:, :, y0:y0 + hc, x0:x0 + wc]
                if cc.pool_exact(c, kind, a, bwd=True):
                    assert _same(g32.contiguous(), dxc.contiguous()), what + " bwd"
                else:
                    _inside(g32, dxc, dbc, what + " bwd")
    # what is held to equality: the identity and the integer up-samplings in both kinds, the integer ratio with dyadic data
    exact = {cc.case_id(k): (cc.pool_exact(k, "random", "none"), cc.pool_exact(k, "dyadic", "scale_shift")) for k in cc.POOL_CASES}
    assert exact["8x12-nocrop-8x12"] == (True, True) and exact["16x24-nocrop-4x6"] == (False, True)
    assert exact["6x6-nocrop-12x12"] == (True, True) and exact["1x1-nocrop-3x5"] == (True, True)
    assert exact["5x7-nocrop-8x11"] == (False, True) and exact["13x10-nocrop-5x7"] == (False, False)          # bins of 1 and 2; bins of 3
    assert cc.pool_exact(cc.POOL_CASES[1], "random", "none", bwd=True) and not cc.pool_exact(cc.POOL_CASES[6], "random", "none", bwd=True)


def _bin_tables(hc, ho):
    """contains[yc, oy]; the closed-form range; the walk over floor(yc ho / hc) - 1 .. + 1 that the gradient kernel used to take"""
    o, y = np.arange(ho), np.arange(hc)
    starts, ends = (o * hc) // ho, -((-(o + 1) * hc) // ho)
    contains = (starts[None, :] <= y[:, None]) & (y[:, None] < ends[None, :])
    lo, hi = (y * ho) // hc, -((-(y + 1) * ho) // hc)
    closed = (lo[:, None] <= o[None, :]) & (o[None, :] < hi[:, None])
    walk = contains & (np.abs(o[None, :] - lo[:, None]) <= 1)
    return contains, closed, walk


def test_the_bin_range_of_the_pool_gradient_is_the_brute_force_search():
    bad = []
    for hc in range(1, 65):
        for ho in range(1, 130):
            contains, closed, walk = _bin_tables(hc, ho)
            assert np.array_equal(contains, closed), (hc, ho)
            assert contains.any(1).all() and contains.any(0).all()
            if not np.array_equal(contains, walk):
                bad.append((hc, ho))
    # the walk over +-1 misses bins only where the pool up-samples; the sizes the loss networks use today are not among them
    assert len(bad) == 5896 and all(ho > hc for hc, ho in bad) and min(bad) == (1, 3) and (5, 8) in bad
    assert min(ho / hc for hc, ho in bad) <= 1.6
    for hc, ho in ((1024, 256), (1024, 512), (512, 512), (188, 112), (256, 512)):
        contains, closed, walk = _bin_tables(hc, ho)
        assert np.array_equal(contains, closed) and np.array_equal(contains, walk)
    for hc, ho in ((128, 512), (64, 256)):          # FaceParsingLoss on a 128^2 image, IDLoss on a 64^2 image
        contains, closed, walk = _bin_tables(hc, ho)
        assert np.array_equal(contains, closed) and not np.array_equal(contains, walk)
    # the up-sampling cases of the list are among the pairs the walk got wrong (x2 is not)
    ups = [(cc.pool_crop(c)[2 + ax], c["dst"][ax]) for c in cc.POOL_CASES for ax in (0, 1) if c["dst"][ax] > cc.pool_crop(c)[2 + ax]]
    assert {(5, 8), (7, 11), (3, 9), (4, 16), (1, 3), (1, 5)} <= set(ups) & set(bad) and (6, 12) in ups and (6, 12) not in bad


# ---- stem convs ------------------------------------------------------------------------------------------------------------------------------
def _conv_cases():
    return [(i, False) for i in range(len(cc.CONV_CASES))] + [(i, True) for i in range(len(cc.CONV_BWD_ONLY))]


@pytest.mark.parametrize("index, bwd_only", _conv_cases(), ids=[cc.case_id(c) for c in cc.CONV_CASES + cc.CONV_BWD_ONLY])
def test_conv_refs_are_the_sum_over_the_taps_and_the_transposed_conv(index, bwd_only):
    for kind in KINDS:
        t = cc.conv_case(index, kind, bwd_only)
        c = t["case"]
        k, s, p = c["k"], c["stride"], c["pad"]
        ho, wo = cc.conv_out(c)
        xd, wd = _nchw(t["x"].double()), t["w"].double()
        what = f"{cc.case_id(c)} {kind}"
        if not bwd_only:
            xp = F.pad(xd, (p, p, p, p))
            want = sum(torch.einsum("bchw,oc->bhwo", xp[:, :, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s], wd[:, :, ky, kx])
                       for ky in range(k) for kx in range(k))
            for (has_bias, relu), (y, bound, pad_only) in t["fwd"].items():
                w2 = want + t["bias"].double() if has_bias else want
                w2 = torch.relu(w2) if relu else w2
                assert _rel(y, w2) < 1e-13 and (bound >= 0).all(), what
                y32 = F.conv2d(_nchw(t["x"]), t["w"], t["bias"] if has_bias else None, stride=s, padding=p)
                y32 = _nhwc(torch.relu(y32) if relu else y32)
                if t["exact"]:
                    assert _same(y32, y), what
                else:
                    _inside(y32, y, bound, what)
                if pad_only.any():
                    b0 = t["bias"].double() if has_bias else torch.zeros(c["Cout"], dtype=torch.float64)
                    assert torch.equal(y[pad_only], (torch.relu(b0) if relu else b0).expand_as(y)[pad_only]), what
        dx, db = t["bwd"]
        want = _nhwc(F.conv_transpose2d(_nchw(t["dy"].double()), wd, stride=s, padding=p,
                                        output_padding=(c["Hi"] + 2 * p - k - s * (ho - 1), c["Wi"] + 2 * p - k - s * (wo - 1))))
        assert dx.shape == t["x"].shape and float((dx - want).abs().max()) < 1e-12, what
        # the GEMM image folded back is the same gradient; the fold of the fp32 z stays inside the gradient's bound
        ncol = k * k * c["Cin"]
        z64 = t["dy"].double() @ wd.permute(2, 3, 1, 0).reshape(ncol, c["Cout"]).t()
        assert float((cc.col2im_ref(z64, c)[0] - dx).abs().max()) < 1e-12, what
        cdx, cb = t["col2im"]
        assert bool(((cdx - dx).abs() <= db).all()) and bool(torch.isnan(t["z"][..., ncol:]).all()) and not bool(torch.isnan(t["z"][..., :ncol]).any())
        assert bool((cb <= db + 1e-300).all()), what
        xg = _nchw(t["x"]).clone().requires_grad_(True)
        g32 = _nhwc(torch.autograd.grad((F.conv2d(xg, t["w"], stride=s, padding=p) * _nchw(t["dy"])).sum(), xg)[0])
        if t["exact"]:
            assert _same(g32, dx) and _same(cdx.float(), dx), what
        else:
            _inside(g32, dx, db, what)


def test_conv_cases_reach_every_path():
    C = cc.CONV_CASES
    assert [cc.conv_gemm_route(c) for c in C] == [False, False, True, False, False, False, False] and not cc.conv_gemm_route(cc.CONV_BWD_ONLY[0])
    lds = [cc.conv_lds_bytes(c) for c in C]
    assert sum(b > cc.LDS_OPT_IN for b in lds) == 1 and lds[2] == 92928 and all(b <= cc.LDS_LIMIT for b in lds)
    assert cc.conv_lds_bytes(dict(k=11, Cin=4, Cout=96)) > cc.LDS_LIMIT                         # the refused weight image
    groups = [c["Cout"] // 16 for c in C]
    assert any(g > cc.CONV_WAVES for g in groups) and any(g == 1 for g in groups) and C[3]["Cout"] // 16 == 5
    npix = [c["B"] * cc.conv_out(c)[0] * cc.conv_out(c)[1] for c in C]
    assert npix[4] == 272 and npix[4] % 64 == 16 and any(n < 64 for n in npix) and any(n > 64 for n in npix)
    assert cc.CONV_BWD_ONLY[0]["Cout"] % 16 != 0 and cc.CONV_BWD_ONLY[0]["Cout"] % 4 == 0
    # stride > k: pixels with a zero gradient and a zero bound; pad = k: outputs that see no pixel
    t = cc.conv_case(5, "random")
    unseen = t["bwd"][1] == 0
    assert unseen.any() and not unseen.all() and float(t["bwd"][0][unseen].abs().max()) == 0
    assert cc.conv_case(6, "random")["fwd"][(True, False)][2].any()
    assert not any(cc.conv_case(i, "random")["fwd"][(True, False)][2].any() for i in range(6))


# ---- max pools, relu -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["maxpool3s2", "maxpool2"])
def test_maxpool_refs_are_the_first_maximum_of_every_window(name):
    k, s = cc.MP_GEOM[name]
    for index, c in enumerate(cc.MP_CASES[name]):
        for kind in cc.MP_KINDS:
            t = cc.maxpool_case(name, index, kind)
            x = t["x"].double()
            ho, wo = (c["H"] - k) // s + 1, (c["W"] - k) // s + 1
            assert t["y"].shape == (c["B"], ho, wo, c["C"]) and int(t["code"].max()) < k * k
            win = torch.stack([x[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s] for ky in range(k) for kx in range(k)])
            assert torch.equal(win.max(0).values, t["y"])
            first = (win == win.max(0).values).to(torch.uint8).argmax(0)                           # the first of the maxima in scan order
            assert torch.equal(first.to(torch.uint8), t["code"]), (name, index, kind)
            want = torch.zeros_like(x)
            for j in range(k * k):
                want[:, j // k:j // k + s * (ho - 1) + 1:s, j % k:j % k + s * (wo - 1) + 1:s] += torch.where(first == j, t["dy"].double(), 0.0)
            assert float((want - t["dx"]).abs().max()) < 1e-14
            if kind == "equal":
                assert int(t["code"].max()) == 0
            if kind == "relu" and c["C"] * c["H"] > 40:
                assert int(((win == 0).sum(0) > 1).sum()) > 0 or name == "maxpool2"               # windows with ties at 0
            xg = _nchw(t["x"]).clone().requires_grad_(True)
            g32 = _nhwc(torch.autograd.grad((F.max_pool2d(xg, k, s) * _nchw(t["dy"])).sum(), xg)[0])
            if t["exact_bwd"]:
                assert _same(g32, t["dx"])
            else:
                _inside(g32, t["dx"], t["bound"], f"{name} {index} {kind}")
    # rows and columns that are in no window: their gradient is 0
    i = 1
    c = cc.MP_CASES[name][i]
    t = cc.maxpool_case(name, i, "negative")
    assert (c["H"], c["W"]) == ((8, 9) if name == "maxpool3s2" else (5, 7))
    assert float(t["dx"][:, -1].abs().max()) == 0 and float(t["dx"][:, :-1].abs().max()) > 0
    if name == "maxpool2":
        assert float(t["dx"][:, :, -1].abs().max()) == 0


def test_relu_cases_hold_both_zeros():
    for index, n in enumerate(cc.RELU_CASES):
        for kind in KINDS:
            t = cc.relu_case(index, kind)
            y = t["y"]
            assert n % 4 == 0 and float(y[1]) == 0 and float(y[2]) == 0 and not np.signbit(y[1].item()) and np.signbit(y[2].item())
            assert torch.equal(t["ref"] != 0, (y > 0) & (t["dy"] != 0)) and (y > 0).any()
    assert cc.RELU_CASES == [4, 1028]


# ---- LPIPS ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cc.LPIPS_CASES)), ids=[cc.case_id(c) for c in cc.LPIPS_CASES])
def test_lpips_refs_are_the_written_formula_and_its_autograd(index):
    c = cc.LPIPS_CASES[index]
    B, HW, C = c["B"], c["h"] * c["w"], c["C"]
    for kind in KINDS:
        t = cc.lpips_case(index, kind)
        fx, fy, w = t["fx"], t["fy"], t["w"]
        nrm = lambda v: v / (torch.sqrt(torch.sum(v ** 2, dim=-1, keepdim=True)) + cc.LP_EPS)          # noqa: E731
        want = (((nrm(fx.double()) - nrm(fy.double())) ** 2) * w.double()).sum(-1).mean((1, 2))
        out, ob = t["fwd"]
        assert _rel(out, want) < 1e-13 and (ob > 0).all() and (w == 0).any() and (w > 0).any()
        _inside((((nrm(fx) - nrm(fy)) ** 2) * w).sum(-1).mean((1, 2)), out, ob, f"lpips {index} {kind}")
        dfx, db = t["bwd"]
        auto = cc.lpips_autograd(fx, fy, w, cc.LPIPS_GOUT, cc.LPIPS_GMUL).reshape(B, HW, C)
        closed, dbf = dfx.reshape(B, HW, C), db.reshape(B, HW, C)
        nan = torch.isnan(auto).any(-1)
        sp = t["special"]
        if sp is None:
            assert not nan.any()
        else:          # autograd differentiates the root at 0: NaN wherever fx is all zero, and only there
            want_nan = torch.zeros(B, HW, dtype=torch.bool)
            want_nan[:, [sp[0], sp[2]]] = True
            assert torch.equal(nan, want_nan)
            fyn = fy.double().reshape(B, HW, C)
            g = cc.f32(cc.LPIPS_GOUT) * cc.f32(cc.LPIPS_GMUL) / HW
            lim = -2 * w.double() * g * (fyn[:, sp[0]] / (fyn[:, sp[0]].pow(2).sum(-1, keepdim=True).sqrt() + cc.LP_EPS)) / cc.LP_EPS
            assert _rel(closed[:, sp[0]], lim) < 1e-13 and float(closed[:, sp[0]].abs().max()) > 1e6          # dn / eps
            assert float(closed[:, sp[2]].abs().max()) == 0 and float(dbf[:, sp[2]].max()) == 0              # both zero: no gradient
            assert float(closed[:, sp[1]].abs().max()) > 0
        assert float((closed[~nan] - auto[~nan]).abs().max()) <= 1e-12 * float(closed[~nan].abs().max())
        # the closed form in fp32
        x32, y32 = fx.reshape(B, HW, C), fy.reshape(B, HW, C)
        rx = x32.pow(2).sum(-1, keepdim=True).sqrt()
        ix, iy = 1 / (rx + cc.LP_EPS), 1 / (y32.pow(2).sum(-1, keepdim=True).sqrt() + cc.LP_EPS)
        g32 = torch.tensor(cc.LPIPS_GOUT) * (torch.tensor(cc.LPIPS_GMUL) / HW)
        dn = 2 * w * (x32 * ix - y32 * iy) * g32
        k2 = torch.where(rx > 0, (dn * x32).sum(-1, keepdim=True) * ix * ix / rx, torch.zeros_like(rx))
        _inside(dn * ix - x32 * k2, closed, dbf, f"lpips_bwd {index} {kind}")
    assert {k["C"] % 64 for k in cc.LPIPS_CASES} >= {0, 4} and any(k["h"] * k["w"] % 16 for k in cc.LPIPS_CASES)
    assert max(k["C"] for k in cc.LPIPS_CASES) == cc.LP_MAX_C and {k["h"] * k["w"] for k in cc.LPIPS_CASES} == {1, 15, 17, 16, 33, 25}


# ---- cosine, frozen norm -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cc.COS_CASES)), ids=[cc.case_id(c) for c in cc.COS_CASES])
def test_cosine_refs_are_F_cosine_similarity_and_its_autograd(index):
    c = cc.COS_CASES[index]
    for kind in KINDS:
        t = cc.cosine_case(index, kind)
        a, b, vals, bounds = t["a"], t["b"], t["vals"], t["bounds"]
        assert float((vals[:, 0] - F.cosine_similarity(a.double(), b.double(), dim=1, eps=0.0)).abs().max()) < 1e-12 and (bounds > 0).all()
        auto = cc.cosine_autograd(a, b)
        da, db = cc.cosine_bwd_ref(a, b, vals, cc.COS_GOUT, cc.COS_GMUL)
        scale = abs(cc.COS_GOUT * cc.COS_GMUL) * float((vals[:, 1:2] * b.double()).abs().max() + (vals[:, 2:3] * a.double()).abs().max())
        assert float((da - auto).abs().max()) <= 1e-10 * scale          # relative to the two terms: they cancel where a is parallel to b
        if c["special"] == "orthogonal":
            assert float(vals[:, 0].abs().max()) < 1e-12 and float(bounds[:, 0].min()) > 0
        if c["special"] == "opposite":
            assert float((vals[:, 0] + 1).abs().max()) < 1e-12
        # fp32 sums stay far outside these bounds (the kernel has to accumulate in double), fp64 sums cast once stay inside
        _inside(vals.float(), vals, bounds, f"cosine {index} {kind}")
        v32 = cc.cosine_ref(a, b)[0].float()
        _inside((cc.f32(cc.COS_GOUT) * cc.f32(cc.COS_GMUL)) * (v32[:, 1:2] * b + v32[:, 2:3] * a), *cc.cosine_bwd_ref(a, b, v32, cc.COS_GOUT, cc.COS_GMUL),
                f"cosine_bwd {index} {kind}")
    assert [cc.cos_nchunk(k["D"]) for k in cc.COS_CASES] == [1, 1, 1, 2, 3, 242]
    assert [cc.cos_chunk(k["D"]) for k in cc.COS_CASES] == [4096] * 5 + [4352] and 4096 * 256 < cc.COS_CASES[-1]["D"]
    assert 4097 - cc.cos_chunk(4097) == 1


def test_norm_ref_is_the_gradient_of_a_frozen_normalisation():
    for index, c in enumerate(cc.NORM_CASES):
        for kind in KINDS:
            t = cc.norm_case(index, kind)
            dy, st, gate, extra = t["dy"], t["stats"], t["gate"], t["extra"]
            xg = torch.zeros(dy.shape, dtype=torch.float64, requires_grad=True)
            y = (xg - st[..., 0].double()[:, None, None]) * st[..., 1].double()[:, None, None]          # BatchNorm2d in eval mode
            loss = (y * gate.double()[:, None, None] * dy.double()).sum() + (y * extra.double()[:, None, None]).sum()
            assert _rel(t["ref"][(True, True)][0], torch.autograd.grad(loss, xg)[0]) < 1e-13
            for (og, oe), (ref, bound) in t["ref"].items():
                v = dy if not og else gate[:, None, None] * dy
                v = v if not oe else v + extra[:, None, None]
                got = st[..., 1][:, None, None] * v
                if t["exact"]:
                    assert _same(got, ref)
                else:
                    _inside(got, ref, bound, f"norm {index} {og} {oe}")
    assert len(cc.NORM_OPTIONS) == 4 and {c["C"] % 64 for c in cc.NORM_CASES} == {4, 12, 0}
