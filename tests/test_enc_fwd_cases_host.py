"""The yardsticks of tests/test_gpu_encoder_forward_kernels.py checked on the CPU, before any kernel is involved (tests/enc_fwd_cases.py)."""
import pytest
import torch
import torch.nn.functional as F

import enc_fwd_cases as ef
from oracle import e4s_oracle as orc

U = ef.U


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _cases(name):
    return [(i, c) for i, c in enumerate(ef.CASES[name])]


def _ids(name):
    return [ef.case_id(c) for c in ef.CASES[name]]


def _same(a32, ref64):
    assert a32.dtype == torch.float32 and ref64.dtype == torch.float64
    return torch.equal(a32.double(), ref64)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _stats64(x, eps=ef.EPS):
    r = ef.stats_ref(x, eps)
    return torch.stack([r["mean"], r["rstd"]], -1)


# ---- every reference against torch's own fp64 operator -------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-5, 1e-3])
def test_stats_apply_and_pooled_refs_are_F_instance_norm(eps):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 7, 6, generator=g) * 0.03 + 1                               # variance ~ 1e-3: eps matters
    x[0, :, :, 0] = 0.3                                                                # variance 0: eps alone under the root
    e32 = ef.f32(eps)
    want = _nhwc(F.instance_norm(_nchw(x.double()), eps=e32))
    st = _stats64(x, eps)
    got, bound = ef.apply_ref(x, st)
    assert _rel(got, want) < 1e-12 and (bound >= 0).all()
    assert float(st[0, 0, 1]) == pytest.approx(e32 ** -0.5, rel=1e-12) and float(ef.stats_ref(x, eps)["var"][0, 0]) < 1e-30
    # the unbiased variance and an eps outside the root are other numbers, far outside the bound
    r = ef.stats_ref(x, eps)
    unbiased = (x.double().var((1, 2), unbiased=True) + e32).rsqrt()
    outside = 1 / (x.double().var((1, 2), unbiased=False).sqrt() + e32)
    assert ((unbiased - r["rstd"]).abs()[:, 1:] > 100 * r["rstd_bound"][:, 1:]).all()
    assert ((outside - r["rstd"]).abs() > 100 * r["rstd_bound"]).all()
    # pooled: the mean of the tensor normalised with the fp32 statistics = (mean - mf) rstd
    st32 = st.float()
    pooled, pb = ef.pooled_ref(x, st32)
    want_p = (r["mean"] - st32[..., 0].double()) * st32[..., 1].double()
    assert ((pooled - want_p).abs() <= pb).all() and (pooled.abs() > 100 * pb).sum() > 6          # and the bound is far below its size
    assert _rel(ef.host_stats(x).double(), _stats64(x, 1e-5)) < 1e-6


@pytest.mark.parametrize("o", ef.APPLY_OPTIONS, ids=[ef.option_id(o) for o in ef.APPLY_OPTIONS])
def test_apply_ref_is_the_gated_norm_plus_shortcut_plus_prelu(o):
    g = torch.Generator().manual_seed(11)
    B, H, W, C = 2, 3, 5, 4
    rs = 2 if o["res"] == "rs2" else 1
    x, res = torch.randn(B, H, W, C, generator=g) * 2 + 1, torch.randn(B, H * rs, W * rs, C, generator=g) - 0.5
    gate, slope = torch.rand(B, C, generator=g) + 0.1, torch.randn(C, generator=g)
    xd, rd = _nchw(x.double()), _nchw(res.double())
    y = F.instance_norm(xd, eps=ef.f32(ef.EPS))
    if o["gate"]:
        y = y * gate.double()[:, :, None, None]
    sc = None
    if o["res"] is not None:
        sc = F.max_pool2d(rd, 1, rs)                                                   # MaxPool2d(1, stride)
        if o["res"] == "rs1_stats":
            sc = F.instance_norm(sc, eps=ef.f32(ef.EPS))
        y = y + sc
    if o["slope"]:
        y = F.prelu(y, slope.double())
    got, bound = ef.apply_ref(x, _stats64(x), gate if o["gate"] else None, None if o["res"] is None else res,
                              _stats64(res) if o["res"] == "rs1_stats" else None, slope if o["slope"] else None, rs)
    assert _rel(got, _nhwc(y)) < 1e-12 and (bound > 0).all()


@pytest.mark.parametrize("C, Cr", ef.SE_SHAPES)
def test_se_ref_is_a_torch_nn_se_module(C, Cr):
    g = torch.Generator().manual_seed(C + Cr)
    pooled, fc1, fc2 = torch.randn(3, C, generator=g), torch.randn(Cr, C, generator=g) / C ** 0.5, torch.randn(C, Cr, generator=g)
    se = torch.nn.Sequential(torch.nn.Conv2d(C, Cr, 1, bias=False), torch.nn.ReLU(), torch.nn.Conv2d(Cr, C, 1, bias=False), torch.nn.Sigmoid()).double()
    with torch.no_grad():
        se[0].weight.copy_(fc1.double()[:, :, None, None])
        se[2].weight.copy_(fc2.double()[:, :, None, None])
        want = se(pooled.double()[:, :, None, None])[:, :, 0, 0]
    ref = ef.se_ref(pooled, fc1, fc2)
    assert _rel(ref["gate"], want) < 1e-12
    assert (ref["a_abs"] >= ref["a"].abs() - 1e-12).all() and (ref["bound"] >= ref["a_bound"] / 4).all() and (ref["a_bound"] > 0).all()


@pytest.mark.parametrize("index, c", _cases("resize"), ids=_ids("resize"))
def test_resize_ref_is_F_interpolate(index, c):
    for kind in ef.KINDS:
        t = ef.build("resize", index, kind)
        want = _nhwc(F.interpolate(t["x"].double(), size=c["dst"], mode="bilinear", align_corners=False))
        assert float((t["ref"] - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), kind
        assert (t["bound"] >= 0).all() and t["ref"].shape == (c["B"],) + c["dst"] + (c["C"],)
        if c["exact"] == "copy":
            assert torch.equal(t["ref"], _nhwc(t["x"]).double())
    assert t["exact"] == (c["exact"] == "copy")                                        # random data: only the copy is held to equality


def test_conv_ref_is_the_sum_over_the_nine_taps():
    t = ef.build("conv", 1, "random")
    x, w = t["x"].double(), t["w"].double()
    B, H, W, Cin = x.shape
    xp = F.pad(_nchw(x), (1, 1, 1, 1))
    want = sum(torch.einsum("bchw,oc->bhwo", xp[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx]) for ky in range(3) for kx in range(3))
    assert _rel(t["ref"], want) < 1e-12 and (t["bound"] > 0).all()
    assert t["bound"].shape == t["ref"].shape == (B, H, W, w.shape[0])


def test_slots_describe_their_rows():
    for i, c in _cases("finalize"):
        t = ef.build("finalize", i, "random")
        s = t["slots"]
        assert s.shape == (c["B"] * c["C"], c["nslots"], 2) and s.dtype == torch.float64
        assert _rel(s[..., 0].sum(1) / ef.FINALIZE_HW, t["ref"]["mean"].flatten()) < 1e-12
        var = s[..., 1].sum(1) / ef.FINALIZE_HW - (s[..., 0].sum(1) / ef.FINALIZE_HW) ** 2
        assert float((var - t["ref"]["var"].flatten()).abs().max()) <= 1e-9 * float(t["ref"]["var"].max())
    assert {c["nslots"] for c in ef.FINALIZE_CASES} == {1, 7, 9, 64} and {c["B"] * c["C"] for c in ef.FINALIZE_CASES} == {192, 256, 300}


# ---- dyadic data: the formulas evaluated in fp32 give the fp64 reference bit for bit ------------------------------------------------------
def _sums_f32(terms):
    """fp32 sums over dim 1 of fp32 terms [B, N, ...] in several orders: torch's, front to back, back to front, shuffled, in blocks of 16"""
    n = terms.shape[1]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    blocks = torch.stack([terms[:, i::16].sum(1) for i in range(min(16, n))], 1)
    return [terms.sum(1), terms.cumsum(1)[:, -1], terms.flip(1).cumsum(1)[:, -1], terms[:, perm].cumsum(1)[:, -1], blocks.cumsum(1)[:, -1]]


def test_dyadic_means_are_exact_in_fp32_on_power_of_two_maps():
    seen = 0
    for name in ("stats", "finalize"):
        for i, c in _cases(name):
            t = ef.build(name, i, "dyadic")
            x = t["x"]
            hw = x.shape[1] * x.shape[2]
            exact = t["exact_mean"] if name == "stats" else True
            assert exact == ef.is_pow2(hw)
            if not exact:
                continue
            seen += 1
            for s in _sums_f32(x.reshape(x.shape[0], hw, -1)):
                assert _same(s / hw, t["ref"]["mean"]), ef.case_id(c)
            pooled, _ = ef.pooled_ref(x, torch.stack([t["ref"]["mean"], t["ref"]["rstd"]], -1).float())
            assert (pooled == 0).all()                                                 # the mean is an fp32 number: no residue
    assert seen >= 6 + len(ef.FINALIZE_CASES)
    assert {c["grid"][0] * c["grid"][1] for c in ef.STATS_CASES if ef.is_pow2(c["grid"][0] * c["grid"][1])} == {1, 16, 128, 1024}


@pytest.mark.parametrize("name", ["apply", "apply_stats"])
def test_dyadic_apply_is_exact_in_fp32(name):
    for i, c in _cases(name):
        t = ef.build(name, i, "dyadic")
        for o in ef.APPLY_OPTIONS:
            kw = ef.apply_operands(t, o)
            ref, _ = ef.apply_ref(t["x"], t["stats"], **kw)
            y = (t["x"] - t["stats"][:, None, None, :, 0]) * t["stats"][:, None, None, :, 1]
            if kw["gate"] is not None:
                y = y * kw["gate"][:, None, None]
            if kw["res"] is not None:
                r = kw["res"][:, ::kw["rs"], ::kw["rs"]]
                if kw["res_stats"] is not None:
                    r = (r - kw["res_stats"][:, None, None, :, 0]) * kw["res_stats"][:, None, None, :, 1]
                y = y + r
            if kw["slope"] is not None:
                y = torch.where(y > 0, y, y * kw["slope"])
            assert _same(y, ref), (ef.case_id(c), ef.option_id(o))
        assert set(t["stats"][..., 1].flatten().tolist()) <= {0.5, 1.0, 2.0, 4.0} and set(t["gate"].flatten().tolist()) <= {0.5, 1.0, 2.0}
        assert float((t["stats"][..., 0] * 4).frac().abs().max()) == 0 and float(t["stats"][..., 0].abs().max()) <= 0.5


def test_dyadic_se_pre_activations_are_exact_in_fp32():
    amax = 0.0
    for i, c in _cases("se"):
        if "dyadic" not in ef.kinds_of("se", c):
            continue
        t = ef.build("se", i, "dyadic")
        ref = t["ref"]
        # every term is a multiple of 2^-6 (fc1 p) resp. 2^-8 (fc2 hidden): any partial sum of any order is an fp32 number
        assert float(ref["h_abs"].max()) * 2 ** 6 < 2 ** 24 and float(ref["a_abs"].max()) * 2 ** 8 < 2 ** 24
        for h in _sums_f32(t["pooled"][:, :, None] * t["fc1"].t()[None]):                    # [B, C, Cr] summed over C
            hid = torch.relu(h)
            for a in _sums_f32(hid[:, :, None] * t["fc2"].t()[None]):                        # [B, Cr, C] summed over Cr
                assert _same(a, ref["a"]), ef.case_id(c)
        amax = max(amax, float(ref["a"].abs().max()))
    assert 8 < amax < 40                                                               # the range the sigmoid residue is measured over


def test_dyadic_resize_and_conv_are_exact_in_fp32():
    for i, c in _cases("resize"):
        t = ef.build("resize", i, "dyadic")
        got = _nhwc(F.interpolate(t["x"], size=c["dst"], mode="bilinear", align_corners=False))
        assert t["exact"] == (c["exact"] is not None)
        if t["exact"]:
            assert _same(got.contiguous(), t["ref"]), ef.case_id(c)
    assert sum(c["exact"] == "dyadic" for c in ef.RESIZE_CASES) == 3
    for i, c in _cases("conv"):
        t = ef.build("conv", i, "dyadic")
        got = _nhwc(F.conv2d(_nchw(t["x"]), t["w"], padding=1))
        assert _same(got.contiguous(), t["ref"]), ef.case_id(c)
        assert float(t["bound"].max()) / ((9 * c["Cin"] + 2) * U) * 2 ** 4 < 2 ** 24          # sum |x| |w| in multiples of 2^-4


# ---- the preconditions of the bounds -----------------------------------------------------------------------------------------------------
def test_random_statistics_keep_the_conditions_of_their_bounds():
    for name in ("stats", "finalize"):
        for i, c in _cases(name):
            t = ef.build(name, i, "random")
            r, cid = t["ref"], ef.case_id(c)
            hw = t["x"].shape[1] * t["x"].shape[2]
            assert (r["cancel"] < U).all(), cid                                        # the cancellation term of the rstd bound
            assert (hw * 2.0 ** -53 * r["mabs"] <= 2.0 ** -10 * U * r["mean"].abs()).all(), cid          # the double additions under the mean's cast
            assert (r["rstd_bound"] <= r["rstd"] * (ef.RSTD_CAP_U + 0.5) * U).all(), cid
            if name == "stats":
                e32 = ef.f32(c["eps"])
                assert float(r["var"][0, 0]) < 1e-30 and float(r["rstd"][0, 0]) == pytest.approx(e32 ** -0.5, rel=1e-12), cid
                std = r["var"][:, 1:].sqrt()
                if hw >= 49:
                    assert float(std.min()) < 0.1 and float(std.max()) > 10 and float(r["mean"].abs().max()) > 100, cid
    assert ef.RSQRT_U + 1 <= ef.RSTD_CAP_U == 8
    assert {c["eps"] for c in ef.STATS_CASES} == {1e-5, 1e-3}


def test_the_outputs_of_the_fused_apply_keep_the_conditions_too():
    for i, c in _cases("apply_stats"):
        t = ef.build("apply_stats", i, "random")
        for o in ef.APPLY_OPTIONS:
            y, _ = ef.apply_ref(t["x"], t["stats"], **ef.apply_operands(t, o))
            r = ef.stats_ref(y.float())
            assert (r["cancel"] < U / 16).all(), (ef.case_id(c), ef.option_id(o))


def test_random_gates_move():
    regimes = set()
    for i, c in _cases("se"):
        t = ef.build("se", i, "random")
        assert float((t["ref"]["gate"] - 0.5).abs().max()) > 1e-4, ef.case_id(c)
        scale = float(t["pooled"].abs().max())
        assert (scale < 1e-7) == (c["regime"] == "residue")
        regimes.add(c["regime"])
    assert regimes == {"residue", "unit"}


# ---- the case lists reach every named path ------------------------------------------------------------------------------------------------
def test_case_lists_reach_every_path():
    hw = lambda c: c["grid"][0] * c["grid"][1]                                          # noqa: E731
    paths = {ef.stats_path(c["B"], hw(c), c["C"]) for c in ef.STATS_CASES}
    assert paths == {"small", "single", "even", "ragged"}
    assert {ef.split_path(hw(c), ef.instnorm_nsplit(c["B"], hw(c), c["C"])) for c in ef.APPLY_STATS_CASES} == {"single", "even", "ragged"}
    # H W < 16 falls through to the split path with one split
    assert {hw(c) for c in ef.STATS_CASES if ef.stats_path(c["B"], hw(c), c["C"]) == "single"} == {1, 15}
    # 4225 pixels at 64 splits: 63 of 67 and 4 left over
    assert ef.instnorm_nsplit(1, 4225, 64) == 64 and -(-4225 // 64) == 67 and 4225 - 63 * 67 == 4
    assert any(c == dict(C=64, grid=(65, 65), B=1, eps=ef.EPS) for c in ef.STATS_CASES) and dict(C=64, grid=(65, 65), B=1) in ef.APPLY_STATS_CASES
    # the batch term decides at B = 8, C = 512
    assert ef.instnorm_nsplit(8, 4225, 512) == 32 != ef.instnorm_nsplit(1, 4225, 512) == 64
    assert ef.split_path(4225, 32) == "ragged"
    # everywhere else a sample's split does not depend on the batch: the batch-independence check of the GPU test holds for these
    for name in ("stats", "apply_stats"):
        for c in ef.CASES[name]:
            if c["B"] != 8:
                assert ef.instnorm_nsplit(c["B"], hw(c), c["C"]) == ef.instnorm_nsplit(1, hw(c), c["C"]), ef.case_id(c)
    assert sum(c["B"] == 8 for c in ef.STATS_CASES) == 1
    # the one-launch kernel: tail only, an unrolled pass and a tail, unrolled passes only
    small = {(ef.small_has_unrolled_pass(hw(c)), ef.small_has_tail(hw(c))) for c in ef.STATS_CASES if ef.stats_is_small(hw(c))}
    assert small == {(False, True), (True, True), (True, False)}
    assert {16, 17, 49, 113, 128, 1023, 1024} == {hw(c) for c in ef.STATS_CASES if ef.stats_is_small(hw(c))}
    assert {c["C"] for c in ef.STATS_CASES} == {64, 128, 512} and {c["B"] for c in ef.STATS_CASES} == {1, 3, 8}
    # SE: the float4 and the scalar fc2 loop, fewer than 64 lanes per row, more rows than threads, C no multiple of 64
    crs = [cr for _, cr in ef.SE_SHAPES]
    assert any(cr % 4 == 0 for cr in crs) and any(cr % 4 for cr in crs) and any(cr > 512 for cr in crs) and any(8 < cr <= 512 for cr in crs)
    assert any(C % 64 for C, _ in ef.SE_SHAPES) and all((C + cr) * 4 <= 48 * 1024 for C, cr in ef.SE_SHAPES)
    # apply: the whole lattice, a channel count only the plain kernel takes
    assert len(ef.APPLY_OPTIONS) == 16 and {c["C"] for c in ef.APPLY_CASES} == {4, 68, 64, 128}
    assert {c["grid"] for c in ef.APPLY_CASES} == {(1, 1), (5, 7), (33, 31)} and any(hw(c) < 64 for c in ef.APPLY_STATS_CASES)
    # the grid-stride stem kernel takes a second lap
    big = [c for c in ef.CONV_CASES if c["grid"] == (257, 256)][0]
    assert big["B"] * 257 * 256 * (big["Cout"] // 4) > 4096 * 256
    assert all(c["tiled"] == (c["Cin"] == 3 and c["Cout"] == 64 and c["grid"][0] % 16 == 0 and c["grid"][1] % 16 == 0) for c in ef.CONV_CASES)


# ---- the yardsticks chained into a bottleneck unit are the oracle's unit ------------------------------------------------------------------
@pytest.mark.parametrize("cin, depth, stride", [(8, 8, 2), (8, 8, 1), (4, 8, 2)], ids=["maxpool-s2", "maxpool-s1", "conv-norm-s2"])
def test_the_references_compose_to_the_oracle_encoder_unit(cin, depth, stride):
    g = torch.Generator().manual_seed(13 + cin + stride)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                    # noqa: E731
    sd = {"res_layer.1.weight": rnd(depth, cin, 3, 3) / 6, "res_layer.2.weight": rnd(depth) * 0.3,
          "res_layer.3.weight": rnd(depth, depth, 3, 3) / 6, "res_layer.5.fc1.weight": rnd(2, depth, 1, 1),
          "res_layer.5.fc2.weight": rnd(depth, 2, 1, 1)}
    if cin != depth:
        sd["shortcut_layer.0.weight"] = rnd(depth, cin, 1, 1)
    x = rnd(2, 8, 6, cin) * 1.7 + 0.3                                                  # NHWC
    want = _nhwc(orc.encoder_unit(sd, "", _nchw(x), cin, depth, stride))

    def stats(t):
        r = ef.stats_ref(t)
        return torch.stack([r["mean"], r["rstd"]], -1)

    n, _ = ef.apply_ref(x, stats(x))                                                   # statistics -> apply
    u, _ = ef.conv_ref(n, sd["res_layer.1.weight"])                                    # -> conv
    ident = torch.stack([torch.zeros(2, depth), torch.ones(2, depth)], -1).double()
    r1, _ = ef.apply_ref(u, ident, slope=sd["res_layer.2.weight"])                     # PReLU
    r2 = ef.conv_ref(r1, sd["res_layer.3.weight"])[0][:, ::stride, ::stride].contiguous()          # a stride-s conv is every s-th output
    st_r = stats(r2)
    pooled, _ = ef.pooled_ref(r2, st_r)
    gate = ef.se_ref(pooled, sd["res_layer.5.fc1.weight"][:, :, 0, 0], sd["res_layer.5.fc2.weight"][:, :, 0, 0])["gate"]
    if cin == depth:
        got, _ = ef.apply_ref(r2, st_r, gate, res=x, rs=stride)
    else:
        sc = (x[:, ::stride, ::stride] @ sd["shortcut_layer.0.weight"][:, :, 0, 0].t()).contiguous()
        got, _ = ef.apply_ref(r2, st_r, gate, res=sc, res_stats=stats(sc))
    # eps: the fp32 1e-5 here, the double 1e-5 there (a relative 2e-8 of eps under the root)
    assert got.shape == want.shape and _rel(got, want) < 1e-9


# ---- K.instnorm_apply looks at its operands before anything touches a device ---------------------------------------------------------------
def test_instnorm_apply_refuses_mismatched_operands_on_the_host():
    from e4s_amd import kernels as K
    x, st = torch.zeros(2, 8, 8, 64), torch.ones(2, 64, 2)
    for kw in (dict(res=torch.zeros(2, 15, 15, 64), rs=2), dict(res=torch.zeros(2, 8, 8, 64), rs=2), dict(res=torch.zeros(2, 8, 8, 32)),
               dict(res=torch.zeros(2, 8, 8, 64), res_stats=torch.ones(1, 64, 2)), dict(gate=torch.ones(2, 32)), dict(slope=torch.ones(63))):
        for want_stats in (False, True):
            with pytest.raises(ValueError):
                K.instnorm_apply(x, st, want_stats=want_stats, **kw)
    with pytest.raises(ValueError):
        K.instnorm_apply(x, torch.ones(2, 64))
    with pytest.raises(RuntimeError):          # operands that fit get as far as the device pointer of a CPU tensor
        K.instnorm_apply(x, st, res=torch.zeros(2, 16, 16, 64), rs=2, gate=torch.ones(2, 64), slope=torch.ones(64))
