"""The yardsticks, the bounds and the restated launch rule of tests/test_gpu_conv_bwd_kernel.py checked on the CPU, before any kernel is
involved (tests/conv_bwd_cases.py)."""
import numpy as np
import pytest
import torch

import conv_bwd_cases as cc

_IDS = [cc.case_id(c) for c in cc.CASES]
_ALL = range(len(cc.CASES))


def _loop_form(gz, wt, x, s, d, reg, R, ncls):
    """dx and ds as the header of csrc/conv_bwd.hip states them, tap by tap in fp64 numpy, on the kernel's own weight layout wt
    [ncls, 9, Cx, Cy] (taps flipped):
        T[q, tap', ci] = sum_co wt[tap', ci, co] d[r(p), co] gz[p, co],   p = q + tap' - 1   (polyphase: p = 2 (q + tap' - 1) + phase)
        dx[q, ci]      = sum_tap' s[r(p), ci] T[q, tap', ci]
        ds[b, r, ci]  += sum_{q, tap': r(p) = r} x[q, ci] T[q, tap', ci]"""
    gz, wt, x, s, d = (np.asarray(a.double()) for a in (gz, wt, x, s, d))
    reg = np.asarray(reg)
    B, H, W, Cx = x.shape
    os_ = 2 if ncls == 4 else 1
    bi = np.arange(B)[:, None, None]
    s, d = s.reshape(B, R, -1), d.reshape(B, R, -1)
    dx, ds = np.zeros_like(x), np.zeros((B, R, Cx))
    for ph in range(ncls):
        gz_ph, r_ph = gz[:, (ph >> 1)::os_, (ph & 1)::os_], reg[:, (ph >> 1)::os_, (ph & 1)::os_]
        for tp in range(9):
            ty, tx = tp // 3 - 1, tp % 3 - 1
            yq, xq = slice(max(0, -ty), min(H, H - ty)), slice(max(0, -tx), min(W, W - tx))              # q with q + tap' - 1 inside
            yp, xp = slice(yq.start + ty, yq.stop + ty), slice(xq.start + tx, xq.stop + tx)
            r_p = r_ph[:, yp, xp]
            T = np.einsum("bhwo,co->bhwc", gz_ph[:, yp, xp] * d[bi, r_p], wt[ph, tp])
            dx[:, yq, xq] += s[bi, r_p] * T
            np.add.at(ds, (np.broadcast_to(bi, r_p.shape), r_p), x[:, yq, xq] * T)
    return dx, ds.reshape(B * R, Cx)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _smallest(ncls):
    mine = [i for i, c in enumerate(cc.CASES) if c["ncls"] == ncls and c["pattern"] not in (None, "one") and c["form"] == "sd"]
    return min(mine, key=lambda i: cc.geometry(cc.CASES[i])["ndx"] * cc.CASES[i]["Cy"] * cc.CASES[i]["B"])


@pytest.mark.parametrize("ncls", [1, 4])
def test_autograd_yardstick_equals_the_loop_form_of_the_kernel_header(ncls):
    t = cc.build(_smallest(ncls), "random")
    dx, ds = _loop_form(t["gz"], t["wt"], t["x"], t["s"], t["d"], t["reg"], t["R"], ncls)
    assert _rel(dx, t["dx"]) < 1e-12 and _rel(ds, t["ds"]) < 1e-12, (_rel(dx, t["dx"]), _rel(ds, t["ds"]))
    # S_abs really is the sum of the absolute values of the same terms
    ax, asum = _loop_form(t["gz"].abs(), t["wt"].abs(), t["x"].abs(), t["s"].abs(), t["d"].abs(), t["reg"], t["R"], ncls)
    assert _rel(ax, t["dx_abs"]) < 1e-12 and _rel(asum, t["ds_abs"]) < 1e-12


def test_unmasked_yardstick_equals_conv2d_input():
    mine = [i for i, c in enumerate(cc.CASES) if c["form"] == "none" and c["ncls"] == 1]
    assert mine
    for i in mine:
        t = cc.build(i, "random")
        co, ci = t["W"].shape[2:]
        w = t["W"][0].double().reshape(3, 3, co, ci).permute(2, 3, 0, 1)
        want = torch.nn.grad.conv2d_input(t["x"].permute(0, 3, 1, 2).shape, w, t["gz"].double().permute(0, 3, 1, 2), padding=1)
        assert t["ds"] is None and _rel(t["dx"].permute(0, 3, 1, 2), want) < 1e-12


@pytest.mark.parametrize("index", _ALL, ids=_IDS)
def test_dyadic_cases_are_exact_in_fp32(index):
    """S_abs / quantum < 2^24 per output element: every partial sum, in any order, is an fp32 number, so exactness on the GPU is a
    property of the data."""
    t = cc.build(index, "dyadic")
    for out in ("dx", "ds"):
        if t[out] is None:
            continue
        k = 2.0 ** cc.QUANTUM_LOG2[out]
        assert torch.equal(t[out] * k, (t[out] * k).round()), out
        assert float(t[out + "_abs"].max()) * k < 2 ** 24, (out, float(t[out + "_abs"].max()) * k)
        assert bool((t[out + "_abs"] >= t[out].abs()).all())
        assert torch.equal(t[out].float().double(), t[out])
    for key in ("s", "d"):
        if t[key] is not None:
            assert set(t[key].abs().unique().tolist()) <= {0.5, 1.0, 2.0}


@pytest.mark.parametrize("index", _ALL, ids=_IDS)
def test_an_fp32_evaluation_in_another_order_is_within_the_bound(index):
    t = cc.build(index, "random")
    dx, ds = cc.grads(t["gz"], t["W"], t["x"], t["s"], t["d"], t["reg"], t["case"]["ncls"], dtype=torch.float32)
    assert bool(((dx.double() - t["dx"]).abs() <= cc.bound(t["dx_abs"], t["n_dx"], cc.C_DX)).all())
    if ds is not None:
        assert bool(((ds.double() - t["ds"]).abs() <= cc.bound(t["ds_abs"], t["n_ds"], cc.C_DS)).all())
    assert 0 < t["n_dx"] + cc.C_DX <= 4095 and int(t["n_ds"].max()) + cc.C_DS <= 4095          # where (k + 1) u bounds k u / (1 - k u)


@pytest.mark.parametrize("mutate", ["region_of_q", "drop_tap"])
@pytest.mark.parametrize("index", _ALL, ids=_IDS)
def test_the_yardstick_and_the_bound_see_the_mistakes_this_kernel_can_make(index, mutate):
    c = cc.CASES[index]
    if mutate == "region_of_q" and c["pattern"] in (None, "one"):
        return                                    # one region (or none) per sample: both pixels are in it
    for kind in cc.KINDS:
        t = cc.build(index, kind)
        dx, ds = cc.grads(t["gz"], t["W"], t["x"], t["s"], t["d"], t["reg"], c["ncls"], mutate=mutate)
        if kind == "dyadic":
            assert not torch.equal(dx, t["dx"])
            assert ds is None or not torch.equal(ds, t["ds"])
        else:
            seen = bool(((dx - t["dx"]).abs() > cc.bound(t["dx_abs"], t["n_dx"], cc.C_DX)).any())
            assert seen
            if ds is not None:
                assert bool(((ds - t["ds"]).abs() > cc.bound(t["ds_abs"], t["n_ds"], cc.C_DS)).any())


def test_case_lists_reach_every_path():
    geo = [cc.geometry(c) for c in cc.CASES]
    both = list(zip(cc.CASES, geo))
    assert {g["BN"] for g in geo} == {32, 64}
    assert {g["ntn"] for g in geo if g["BN"] == 32} >= {1, 3} and {g["ntn"] for g in geo if g["BN"] == 64} >= {1, 2}
    assert {g["ntn"] for g in geo} >= {1, 2, 3}
    assert {g["nchunk"] for g in geo} == {1, 2}
    assert any(g["nchunk"] == 2 and g["gsplit"] > 1 for g in geo)                     # more than one K chunk together with a split
    assert {g["situation"] for g in geo} >= {"one", "all", "uneven", "idle"}
    assert {c["ncls"] for c, g in both if g["situation"] == "idle"} == {1, 4}
    ds_cases = [(c, g) for c, g in both if "s" in c["form"]]
    assert {g["two_level"] for c, g in ds_cases} == {False, True}
    assert any(g["situation"] == "one" and g["blocks"] == 256 for c, g in ds_cases)
    # the issue's two idle splits, by the restated rule
    idle = {(c["ncls"], c["B"]): g for c, g in both if g["situation"] == "idle"}
    assert (idle[(4, 1)]["blocks"], idle[(4, 1)]["gsplit"], idle[(4, 1)]["groups"].count(0)) == (20, 25, 7)
    assert (idle[(1, 4)]["blocks"], idle[(1, 4)]["gsplit"], idle[(1, 4)]["groups"].count(0)) == (80, 6, 1)
    # tiles: one full, one partial, ragged both ways with several tiles
    assert any(c["grid"] == (8, 16) and g["per_img"] == 1 for c, g in both)
    assert any(c["grid"] == (5, 7) for c in cc.CASES) and any(c["grid"] == (13, 37) and g["per_img"] == 6 for c, g in both)
    for ncls in (1, 4):
        mine = [c for c in cc.CASES if c["ncls"] == ncls and c["pattern"] is not None]
        assert {c["rel"] for c in mine} == {"larger", "equal", "smaller"}
        assert {c["grid"] for c in mine} >= {(5, 7), (16, 24), (13, 37)}
    assert {c["pattern"] for c in cc.CASES} == set(cc.PATTERNS) | {None}
    assert {c["R"] for c in cc.CASES if c["pattern"] is not None} >= {3, 12, 16}
    assert {c["form"] for c in cc.CASES} == set(cc.FORMS)
    assert any(c["form"] == "none" and g["gsplit"] > 1 for c, g in both)              # the encoder's call with a dx workspace
    # batch invariance has cases to look at, for both ncls
    assert {c["ncls"] for c in cc.CASES if c["B"] == 3 and cc.geometry(c, 1)["gsplit"] == cc.geometry(c, 3)["gsplit"]} == {1, 4}
    # the workspace restatement is consistent with itself
    for c, g in both:
        for want_ds in (True, False):
            used = cc.ws_used(c, want_ds)
            assert all(a < b for a, b in used) and (not used or used[-1][1] <= cc.ws_floats(c, want_ds))


def test_absent_pattern_leaves_rows_without_a_pixel():
    for i, c in enumerate(cc.CASES):
        if c["pattern"] == "absent":
            t = cc.build(i, "random")
            assert int((t["count"] == 0).sum()) >= 2
            assert bool((t["ds"][t["count"] == 0] == 0).all())


def test_reduce_parts_restatement():
    for nparts in cc.REDUCE_NPARTS:
        for n in cc.REDUCE_N:
            parts = cc.reduce_parts_data(nparts, n, "dyadic")
            for scale in cc.REDUCE_SCALES:
                assert np.array_equal(cc.reduce_parts_ref(parts.numpy(), scale).astype(np.float64), (parts.double().sum(0) * scale).numpy())
    # in order: with 1e8, 1, -1e8 the parts cancel only in index order
    assert cc.reduce_parts_ref(np.array([[1e8], [-1e8], [1.0]], dtype=np.float32), 1.0)[0] == 1.0
    assert cc.reduce_parts_ref(np.array([[1e8], [1.0], [-1e8]], dtype=np.float32), 1.0)[0] == 0.0
    # chunks of 64 first: 64 parts of 1e8, one of 1, 64 of -1e8 would give 0 in plain index order
    rows = np.array([[1.0]] + [[1e8]] * 63 + [[-1e8]] * 63 + [[1.0]], dtype=np.float32)
    plain = np.float32(0)
    for r in rows[:, 0]:
        plain = np.float32(plain + r)
    assert cc.reduce_parts_ref(rows, 1.0)[0] != plain


def test_pack_and_shift_scale_restatements_against_loops():
    g = torch.Generator().manual_seed(3)
    W = cc.operand((4, 9, 3, 2), "random", g)
    wt = cc.pack_bwd_ref(W)
    assert wt.shape == (4, 9, 2, 3)
    for cls in range(4):
        for tp in range(9):
            assert torch.equal(wt[cls, tp], W[cls, 8 - tp].t())
    x, tab = cc.operand(cc.SHIFT_X, "random", g), cc.operand((cc.SHIFT_X[0] * cc.SHIFT_R, cc.SHIFT_X[3]), "random", g)
    labels = cc.make_labels("noise", cc.SHIFT_X[0], *cc.SHIFT_MAP, cc.SHIFT_R, seed=1)
    for c in cc.SHIFT_CASES[:10:3]:
        got = cc.shift_scale_ref(x, tab, labels, cc.SHIFT_R, c["anchors"], c["istride"], c["dy"], c["dx"], c["os"], c["py"], c["px"])
        (Ha, Wa), os_ = c["anchors"], c["os"]
        reg = cc.region_map(labels, Ha * os_, Wa * os_)
        for b in range(x.shape[0]):
            for ay in range(Ha):
                for ax in range(Wa):
                    iy, ix = ay * c["istride"] + c["dy"], ax * c["istride"] + c["dx"]
                    inside = 0 <= iy < x.shape[1] and 0 <= ix < x.shape[2]
                    r = int(reg[b, ay * os_ + c["py"], ax * os_ + c["px"]])
                    want = x[b, iy, ix] * tab[b * cc.SHIFT_R + r] if inside else torch.zeros(x.shape[3])
                    assert torch.equal(got[b, ay, ax], want)
    assert any(c["dy"] < 0 and c["dx"] < 0 for c in cc.SHIFT_CASES) and any(c["dy"] > 0 and c["dx"] > 0 for c in cc.SHIFT_CASES)
    assert {c["istride"] for c in cc.SHIFT_CASES} == {1, 2} and {c["labels"] for c in cc.SHIFT_CASES} == {True, False}
    assert {(c["os"], c["py"], c["px"]) for c in cc.SHIFT_CASES} == {(1, 0, 0), (2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1)}
