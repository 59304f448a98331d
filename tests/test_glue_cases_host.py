"""The yardsticks of tests/glue_cases.py, checked on the CPU (no GPU, no native library): every fp64 reference against an independent
statement (explicit loops on a small case, the oracle's upfirdn2d and fused_bias_act, ATen in fp64); the dyadic precondition per case;
every bound of a summed output against the same sum restated in plain fp32 in three orders (ascending, descending, lane-strided), which
also equal the reference on dyadic data; the dispatch predicates against the ids of the cases and the constants against the sources;
the region-plan checker against a correct plan and three broken ones; and the empty-output form of kernels.upfirdn2d_raw, which may not
reach the library."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_cases as gl
from oracle import e4s_oracle as orc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "e4s_amd", "csrc")


def _close(a, b, what, tol=1e-12):
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), what


# ---- the three fp32 orders -----------------------------------------------------------------------------------------------------------------
def _seq(t):
    """the fp32 sum over axis 0, one term after the other"""
    return np.add.accumulate(np.ascontiguousarray(t, dtype=np.float32), axis=0, dtype=np.float32)[-1]


def _orders(terms, lanes=64):
    """fp32 terms [N, ...] -> their sum ascending, descending and lane-strided (lane l adds terms l, l + lanes, ...; then the lanes)"""
    t = np.ascontiguousarray(terms.numpy() if isinstance(terms, torch.Tensor) else terms, dtype=np.float32)
    n = t.shape[0]
    pad = (-n) % lanes
    tp = np.concatenate([t, np.zeros((pad,) + t.shape[1:], dtype=np.float32)]) if pad else t
    strided = _seq(_seq(tp.reshape((-1, lanes) + t.shape[1:])))
    return {"ascending": _seq(t), "descending": _seq(t[::-1]), "lane-strided": strided}


def _check_orders(terms, ref, bound, exact, what, scale=None):
    for name, s in _orders(terms).items():
        s = torch.from_numpy(np.asarray(s)).reshape(ref.shape)
        if scale is not None:
            s = scale(s)
        if exact:
            assert torch.equal(s, ref.float()), f"{what}: the {name} fp32 sum of dyadic data is not the reference"
        else:
            err = (s.double() - ref).abs()
            assert bool((err <= bound).all()), f"{what}: the {name} fp32 sum leaves the bound by {float((err - bound).max()):.3e}"


# ---- references against independent statements ---------------------------------------------------------------------------------------------
def test_fused_bias_act_reference_is_the_oracles_and_a_loop():
    for index in range(5):
        for kind in gl.KINDS:
            t = gl.fba_case(index, kind)
            for (act, grad, has_b), (ref, bound) in t["refs"].items():
                x = (t["xb"] if has_b else t["x"]).double()
                want = orc.fused_bias_act(x, t["bias"].double() if has_b else None, t["ref"].double(), act, grad, t["alpha"], t["scale"])
                _close(ref, want, f"fused_bias_act {t['case']['tag']} {act}{grad}")
                assert bool((bound >= 0).all())
    t = gl.fba_case(1, "random")          # explicit loop, code 31 with a bias, [1, 3, 5, 7]
    ref, _ = t["refs"][(3, 1, True)]
    x, r, b = t["xb"].view(-1).tolist(), t["ref"].view(-1).tolist(), t["bias"].tolist()
    for i in range(t["n"]):
        v = x[i] + b[(i // t["step_b"]) % 3]
        want = (v if r[i] > 0 else v * t["alpha"]) * t["scale"]
        assert abs(float(ref.view(-1)[i]) - want) <= 1e-12
    # the planted zeros: ref = +-0.0 takes the alpha branch (strict >)
    assert float(ref.view(-1)[2]) == pytest.approx((0.75 + b[0]) * t["alpha"] * t["scale"], rel=1e-12)


def test_upfirdn_reference_is_the_oracles_and_a_loop():
    seen = 0
    for index, c in enumerate(gl.UFD_CASES):
        (ux, uy), (dx, dy), (px0, px1, py0, py1) = c["up"], c["down"], c["pad"]
        if ux != uy or dx != dy or (px0, px1) != (py0, py1) or c["size"][0] * c["size"][1] * c["minor"] > 40000:
            continue
        t = gl.ufd_case(index, "random")
        want = orc.upfirdn2d(t["x"].double().permute(0, 3, 1, 2), t["k"].double(), up=ux, down=dx, pad=(px0, px1)).permute(0, 2, 3, 1)
        _close(t["ref"], want, "upfirdn2d " + c["tag"])
        seen += 1
    assert seen >= 6
    # explicit loops (upfirdn2d_kernel.cu:52-137) on a geometry with every parameter different per axis
    g = torch.Generator().manual_seed(5)
    x, k = torch.randn(2, 3, 4, 2, generator=g), torch.randn(2, 3, generator=g)
    up, down, pad = (2, 3), (2, 1), (1, 0, -1, 2)
    y, sabs, T = gl.upfirdn_ref(x, k, up, down, pad)
    oh, ow = (3 * 3 - 1 + 2 - 2) // 1 + 1, (4 * 2 + 1 + 0 - 3) // 2 + 1
    assert tuple(y.shape) == (2, oh, ow, 2)
    for m in range(2):
        for oy in range(oh):
            for ox in range(ow):
                for c in range(2):
                    acc, mag, n = 0.0, 0.0, 0
                    for ky in range(2):
                        for kx in range(3):
                            qy, qx = oy * down[1] - pad[2] + ky, ox * down[0] - pad[0] + kx
                            if qy % up[1] or qx % up[0] or not (0 <= qy // up[1] < 3 and 0 <= qx // up[0] < 4):
                                continue
                            p = float(x[m, qy // up[1], qx // up[0], c]) * float(k[1 - ky, 2 - kx])
                            acc, mag, n = acc + p, mag + abs(p), n + 1
                    assert abs(float(y[m, oy, ox, c]) - acc) <= 1e-12 and abs(float(sabs[m, oy, ox, c]) - mag) <= 1e-12
                    assert int(T[m, oy, ox, c]) == n


def test_the_other_references_against_aten_and_loops():
    for kind in gl.KINDS:
        t = gl.csum_case(15, 3, 3, kind)
        for c in range(3):
            assert float(t["ref"][c]) == pytest.approx(sum(float(v) for o in range(3) for v in t["x"][o, c]), abs=1e-9)
        t = gl.c1_case(3, 4, (7, 9), kind)
        y, _ = t["refs"][(True, 1)]
        v = F.conv2d(t["x"].double(), t["w"].double()[:, :, None, None] * t["scale"], t["bias"].double())
        _close(y, (F.leaky_relu(v, t["alpha"]) * t["gain"]).permute(0, 2, 3, 1), "conv1x1_small")
        t = gl.nh_case(4, kind)
        _close(t["ref"], F.leaky_relu(t["nw"] * t["feat"].double() + t["bias"].double(), t["alpha"]) * t["gain"], "noise_half")
        t = gl.pn_case(4, 63, kind)
        xd = t["x"].double()
        _close(t["ref"], xd / torch.sqrt((xd * xd).sum(1, keepdim=True) / 63 + gl.EPS8), "pixelnorm")
        assert float(t["ref"][3].abs().max()) == 0
        # model.py:783-790 on the NCHW tensor
        t = gl.ms_case(8, 4, (4, 4), 20, kind)
        out = t["x"].double().permute(0, 3, 1, 2)
        sd = out.view(4, -1, 1, 20, 4, 4)
        sd = torch.sqrt(sd.var(0, unbiased=False) + gl.EPS8).mean([2, 3, 4], keepdims=True).squeeze(2).repeat(4, 1, 4, 4)
        _close(t["stat"], sd[:, 0, 0, 0], "minibatch_stddev")
        t = gl.rd_case(9, 5, 260, kind)
        _close(t["mode0"][0], F.linear(t["style"].double(), t["M"].double() * gl.rd_scale(260), t["bias"].double()), "rowdot mode 0")
        cs = t["conv_scale"]
        wmod = cs * t["wsq"].double().sqrt()[None] * t["style"].double()[:, None]            # |scale W s|, [G, O, K]
        _close(t["mode1"][0], cs * torch.rsqrt(wmod.pow(2).sum(2) + gl.EPS8), "rowdot mode 1")
        t = gl.rd_latent_case(260, 3, kind)
        st = t["latent"][:, :, 2].reshape(6, 260).double()
        _close(t["refs"][(2, True)][0], F.linear(st, t["M"].double() * gl.rd_scale(260), t["bias"].double()), "modulate")
        _close(t["refs"][(1, False)][0], F.linear(t["latent"][:, 0, 1].double(), t["M"].double() * gl.rd_scale(260), t["bias"].double()), "modulate")
        t = gl.ws_case((3, 4), 9, kind)
        _close(t["ref"], torch.tensor([[sum(float(v) ** 2 for v in t["w"][o, i].flatten()) for i in range(4)] for o in range(3)], dtype=torch.float64), "weight_sqsum")
        t = gl.nb_case(3, kind)
        for mode in gl.NB_NOISE:
            nz = 0 if mode == "none" else t["nw"] * (t["noise"][:1] if mode == "shared" else t["noise"]).double()[..., None]
            _close(t["refs"][mode][0], F.leaky_relu(t["x"].double() + nz + t["bias"].double(), t["alpha"]) * t["gain"], "noise_bias_act " + mode)
        t = gl.mm_case((5, 7), "smaller", True, kind)
        hm, wm = gl.MAPS[(5, 7)]["smaller"]
        for b in range(gl.MM_B):          # nearest as floor(dst * in / out), the definition of ATen's legacy "nearest"
            for yy in range(5):
                for xx in range(7):
                    m = float(t["mask"][b, 2, yy * hm // 5, xx * wm // 7])
                    assert float((t["refs"][2][0][b, yy, xx] - t["y"][b, yy, xx].double() * m).abs().max()) <= 1e-12
        t = gl.as_case(1020, kind)
        assert torch.equal(t["ref1"].float(), t["a"] + t["b"]), "the fp32 sum is the rounded fp64 sum"


# ---- the dyadic precondition and the bounds --------------------------------------------------------------------------------------------------
def test_dyadic_sums_are_exact_in_fp32():
    lim = 2.0 ** 24
    for step in gl.CSUM_STEPS:
        t = gl.csum_case(step, 3, 64, "dyadic")
        assert float(t["sabs"].max()) / t["quantum"] < lim
    for index in range(len(gl.UFD_CASES)):
        t = gl.ufd_case(index, "dyadic")
        assert float(t["sabs"].max()) / t["quantum"] < lim, t["case"]["tag"]
    for K in gl.RD_K:
        t = gl.rd_case(24, 5, K, "dyadic")
        assert float(t["sabs"].max()) / t["quantum"] < lim
    for index in range(len(gl.COLSUM_CASES)):
        t = gl.colsum_case(index, "dyadic")
        assert float(t["sabs"].max()) / t["quantum"] < lim, t["case"]
    # conv1x1 (<= 4 products of 2^-4) and weight_sqsum (<= 9 squares) are far inside


@pytest.mark.parametrize("kind", gl.KINDS)
def test_bounds_hold_for_three_fp32_orders_of_the_sums(kind):
    for step in gl.CSUM_STEPS:
        for outer in gl.CSUM_OUTER:
            t = gl.csum_case(step, outer, 3, kind)
            _check_orders(t["x"].permute(0, 2, 1).reshape(-1, 3), t["ref"], t["bound"], t["exact"], f"channel_sum step{step} outer{outer}")
    for index, c in enumerate(gl.UFD_CASES):
        if c["minor"] > 24:          # the same arithmetic per channel: the narrow cases cover it
            continue
        t = gl.ufd_case(index, kind)
        (ux, uy), (dx, dy), (px0, px1, py0, py1) = c["up"], c["down"], c["pad"]
        x = t["x"].permute(0, 3, 1, 2).reshape(-1, 1, *c["size"])
        z = x.new_zeros(x.shape[0], 1, c["size"][0] * uy, c["size"][1] * ux)
        z[:, :, ::uy, ::ux] = x
        z = F.pad(z, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
        z = z[:, :, max(-py0, 0): z.shape[2] - max(-py1, 0), max(-px0, 0): z.shape[3] - max(-px1, 0)]
        cols = F.unfold(z, c["k"], stride=(dy, dx))                                          # [P, taps, L]
        terms = (cols * torch.flip(t["k"], [0, 1]).reshape(1, -1, 1)).permute(1, 0, 2)       # fp32 products, [taps, P, L]
        ref = t["ref"].permute(0, 3, 1, 2).reshape(x.shape[0], -1)
        bound = t["bound"].permute(0, 3, 1, 2).reshape(x.shape[0], -1)
        _check_orders(terms, ref, bound, t["exact"], "upfirdn2d " + c["tag"])
    for cin in gl.C1_CIN:
        t = gl.c1_case(cin, 36, (7, 9), kind)
        terms = torch.einsum("bchw,oc->cbhwo", t["x"], t["w"])
        for (has_b, act), (ref, bound) in t["refs"].items():
            def epi(a, has_b=has_b, act=act):
                v = a * np.float32(t["scale"]) + (t["bias"] if has_b else 0)
                return torch.where(v > 0, v, v * np.float32(t["alpha"])) * np.float32(t["gain"]) if act else v
            _check_orders(terms, ref, bound, t["exact"], f"conv1x1_small Cin{cin}", scale=epi)
    for K in gl.RD_K:
        t = gl.rd_case(9, 5, K, kind)
        terms = (t["style"][:, None, :] * t["M"][None]).permute(2, 0, 1)
        _check_orders(terms, *t["mode0"], t["exact0"], f"rowdot K{K}", scale=lambda a, t=t, K=K: a * np.float32(gl.rd_scale(K)) + t["bias"])
    for shape in gl.WS_SHAPES:
        t = gl.ws_case(shape, 9, kind)
        _check_orders(t["terms"].permute(2, 0, 1), t["ref"], t["bound"], t["exact"], f"weight_sqsum {shape}")
    for index, c in enumerate(gl.COLSUM_CASES):
        if c["rows"] * c["C"] > 600000:
            continue
        t = gl.colsum_case(index, kind)
        _check_orders(t["x"], t["ref"], t["bound"], t["exact"], f"colsum {c}")


def test_elementwise_bounds_hold_for_the_fp32_chain():
    """the elementwise kernels restated in torch fp32 (one rounding per operation, no contraction) stay inside their bounds"""
    for kind in gl.KINDS:
        t = gl.fba_case(0, kind)
        a, s = np.float32(t["alpha"]), np.float32(t["scale"])
        for (act, grad, has_b), (ref, bound) in t["refs"].items():
            v = (t["xb"] + t["bias"].view(1, -1, 1, 1)) if has_b else t["x"]
            code = act * 10 + grad
            y = torch.zeros_like(v) if code in (12, 32) else torch.where(v > 0, v, v * a) * s if code == 30 else \
                torch.where(t["ref"] > 0, v, v * a) * s if code == 31 else v * s
            assert bool(((y.double() - ref).abs() <= bound).all()), (kind, code, has_b)
            if t["exact"]:
                assert torch.equal(y, ref.float())
        t = gl.pn_case(5, 1000, kind)
        x = t["x"]
        y = x * torch.rsqrt((x * x).sum(1, keepdim=True) / 1000 + np.float32(1e-8))
        assert bool(((y.double() - t["ref"]).abs() <= t["bound"]).all())
        t = gl.as_case(1020, kind)
        assert bool(((((t["a"] + t["b"]) * np.float32(gl.AS_SCALE)).double() - t["ref"]).abs() <= t["bound"]).all())
        for B, group in gl.MS_GROUPS:
            t = gl.ms_case(B, group, (4, 4), 20, kind)
            xs = t["x"].view(group, B // group, -1)
            mean = xs[0].clone()
            for g_ in range(1, group):
                mean = mean + xs[g_]
            mean = mean / group
            var = torch.zeros_like(mean)
            for g_ in range(group):
                var = var + (xs[g_] - mean) * (xs[g_] - mean)
            sd = torch.sqrt((var / group + np.float32(1e-8)).double()).float().double().mean(1).float().repeat(group)          # sqrtf, correctly rounded
            assert bool(((sd.double() - t["stat"]).abs() <= t["bound"]).all()), (kind, B, group)
            t = gl.ms_case(B, group, (4, 4), 20, kind, identical=True)
            if gl.ms_identical_exact(group, kind):
                assert bool((t["stat"].float() == gl.ROOT_EPS8).all())


# ---- dispatch predicates and constants -------------------------------------------------------------------------------------------------------
def test_every_case_reaches_the_launch_form_its_id_names():
    paths = [gl.upfirdn_path(c) for c in gl.UFD_CASES]
    assert paths == gl.UFD_EXPECT
    for c, p in zip(gl.UFD_CASES, paths):
        assert c["tag"].startswith(p), c["tag"]
        if "multitile" in c["tag"]:
            assert p == "generic" and c["out"][0] > gl.TOH and c["out"][1] > gl.TOW, c["tag"]
    for p in ("generic", "fir_nhwc", "fir_nhwc_fixed44"):
        assert paths.count(p) >= 2
    assert any("multitile-down2" in c["tag"] and c["down"] == (2, 2) for c in gl.UFD_CASES)
    assert {(c["up"], c["down"]) for c in gl.UFD_GENERIC} >= {((u, u), (d, d)) for u, d in ((1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (2, 3))}
    for c in gl.FBA_CASES:
        n, step = int(np.prod(c["shape"])), gl.fba_step(c["shape"])
        assert (gl.fba_form(n, step, True, c["offset"]), gl.fba_form(n, step, False, c["offset"])) == c["forms"], c["tag"]
        assert ("gridstride" in c["tag"]) == c["forms"][0].endswith("+loop")
    assert {f for c in gl.FBA_CASES for f in c["forms"]} == {"v4", "scalar", "v4+loop", "scalar+loop"}
    want = {"batch_sum": ("batch_sum", None), "first-colsum": ("colsum", 1), "one-block": ("colsum", 1), "two-blocks": ("colsum", 1),
            "one-level-64-parts": ("colsum", 1), "second-level": ("colsum", 2), "rpb-doubles": ("colsum", 2)}
    for c in gl.COLSUM_CASES:
        path, rpb, parts, levels = gl.colsum_levels(c["rows"], c["C"])
        key = "batch_sum" if c["tag"].startswith("batch_sum") else c["tag"]
        assert path == want[key][0] and (want[key][1] is None or levels == want[key][1]), c
        if key == "rpb-doubles":
            assert rpb == 2 * gl.COLSUM_RPB and gl.colsum_levels(c["rows"] - 1, c["C"])[1] == gl.COLSUM_RPB
        if key == "second-level":
            assert parts == gl.RCHUNK + 1
        if key == "one-block":
            assert parts == 1


def test_the_constants_are_those_of_the_sources():
    optim = open(os.path.join(CSRC, "optim.hip")).read()
    ops = open(os.path.join(CSRC, "ops.hip")).read()
    assert int(re.search(r"constexpr int RCHUNK = (\d+);", optim).group(1)) == gl.RCHUNK
    body = optim[optim.index("inline int colsum_rpb"):]
    assert int(re.search(r"int64_t rpb = (\d+);", body).group(1)) == gl.COLSUM_RPB
    assert int(re.search(r"/ rpb > (\d+)\) rpb \*= 2;", body).group(1)) == gl.COLSUM_MAX_PARTS
    assert re.search(r"if \(nparts > RCHUNK\) \{", optim)
    m = re.search(r"constexpr int TOH = (\d+), TOW = (\d+);", ops)
    assert (int(m.group(1)), int(m.group(2))) == (gl.TOH, gl.TOW)
    assert ops.count("< 8192 ?") == 2 and "const int block = 256;" in ops
    kern = open(os.path.join(os.path.dirname(CSRC), "kernels.py")).read()
    assert "if rows <= 64 or c % 4 or c > 1024:" in kern and re.search(r"^BM = 128\b", kern, re.M) and gl.BM == 128


# ---- the region-plan checker -----------------------------------------------------------------------------------------------------------------
def test_plan_checker_accepts_a_correct_plan_and_rejects_broken_ones():
    for c in gl.PLAN_CASES:
        for pattern in gl.gc.PATTERNS:
            lab = gl.plan_labels(c, pattern)
            args = (lab, c["B"], c["R"], c["anchors"][0], c["anchors"][1], c["nphase"])
            rows, tiles, meta = gl.plan_numpy(*args)
            gl.check_plan(rows, tiles, meta, *args)
    c = dict(anchors=(13, 37), rel="smaller", nphase=4, B=3, R=12)
    lab = gl.plan_labels(c, "blocks")
    args = (lab, 3, 12, 13, 37, 4)
    rows, tiles, meta = gl.plan_numpy(*args)
    t = tiles[:meta[0] * 4].reshape(-1, 4)
    # two tiles of the same phase and different groups
    i = 0
    j = next(n for n in range(1, len(t)) if t[n][2] == t[i][2] and t[n][1] != t[i][1])
    moved = rows.copy()
    moved[t[i][0]], moved[t[j][0]] = rows[t[j][0]], rows[t[i][0]]          # one anchor each moved to a neighbouring group
    doubled = rows.copy()
    doubled[t[i][0] + 1] = rows[t[i][0]]                                    # one anchor twice (and its neighbour lost)
    dropped = rows.copy()
    dropped[t[i][0] + t[i][3] - 1] = -1                                     # the last anchor of a tile dropped
    for bad, what in ((moved, "moved"), (doubled, "duplicated"), (dropped, "dropped")):
        with pytest.raises(AssertionError):
            gl.check_plan(bad, tiles, meta, *args)
    short = tiles.copy()
    short[3] -= 1
    with pytest.raises(AssertionError):
        gl.check_plan(rows, short, meta, *args)
    # the region is that of the OUTPUT pixel: on a noise map of the output grid's size, phase 3 of some anchor is not in its phase-0 region
    lab = gl.plan_labels(dict(c, rel="equal"), "noise")
    g4 = gl.plan_groups(lab, 3, 12, 13, 37, 4)
    region_of = lambda ph: {a: k // 4 for k, v in g4.items() if k % 4 == ph for a in v}          # noqa: E731
    assert region_of(0) != region_of(3)


# ---- the empty output of upfirdn2d -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_hw, k, down, pad, want", [((3, 9), (4, 4), 2, 0, (0, 3)), ((9, 3), (4, 4), 2, 0, (3, 0)),
                                                       ((2, 2), (4, 4), 1, 0, (0, 0)), ((3, 3), (4, 4), 3, 0, (0, 0)),
                                                       ((2, 8), (5, 3), 2, 0, (0, 3))])
def test_upfirdn2d_raw_returns_the_empty_tensor_without_calling_the_library(monkeypatch, in_hw, k, down, pad, want):
    """in up + pad0 + pad1 - k < 0: Python's flooring division gives an extent <= 0 where C's truncating one gave 1.  The wrapper may not
    hand such a geometry to the library (which now returns before any launch as well)."""
    from e4s_amd import kernels as K

    def refuse(*a):
        raise AssertionError("the library was called")

    monkeypatch.setattr(K, "call", refuse)
    y = K.upfirdn2d_raw(torch.zeros(2, in_hw[0], in_hw[1], 8), torch.ones(k), 1, 1, down, down, pad, pad, pad, pad)
    assert tuple(y.shape) == (2, want[0], want[1], 8) and y.numel() == 0
    src = open(os.path.join(CSRC, "ops.hip")).read()
    assert "if (num_h < 0 || num_w < 0 || major <= 0 || minor <= 0) return 0;" in src
