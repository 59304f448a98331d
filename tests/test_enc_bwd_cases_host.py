"""The yardsticks of tests/test_gpu_encoder_backward_kernels.py checked on the CPU, before any kernel is involved (tests/enc_bwd_cases.py)."""
import pytest
import torch
import torch.nn.functional as F

import enc_bwd_cases as ec


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _cases(name):
    return [(i, c) for i, c in enumerate(ec.CASES[name])]


# ---- every reference against fp64 autograd of the plainly written op ---------------------------------------------------------------------
@pytest.mark.parametrize("gate, acc", [(False, False), (True, False), (False, True), (True, True)])
def test_in_ref_equals_autograd_of_gated_instance_norm(gate, acc):
    B, H, W, C = 2, 5, 7, 6
    g = torch.Generator().manual_seed(3 + 2 * gate + acc)
    dy, x = torch.randn(B, H, W, C, generator=g), torch.randn(B, H, W, C, generator=g) * 3 + 1
    gt = torch.rand(B, C, generator=g) - 0.3 if gate else None
    ac = torch.randn(B, H, W, C, generator=g) if acc else None
    xd = x.double().permute(0, 3, 1, 2).requires_grad_(True)                       # NCHW for F.instance_norm
    gd = (torch.ones(B, C) if gt is None else gt).double().requires_grad_(True)
    bias = torch.zeros(B, C, dtype=torch.float64, requires_grad=True)
    y = gd[:, :, None, None] * F.instance_norm(xd, eps=ec.EPS) + bias[:, :, None, None]
    dxa, dga, dba = torch.autograd.grad((y * dy.double().permute(0, 3, 1, 2)).sum(), (xd, gd, bias))
    mean, var = xd.detach().mean((2, 3)), xd.detach().var((2, 3), unbiased=False)
    stats = torch.stack([mean, (var + ec.EPS).rsqrt()], -1)                        # exact (fp64) statistics
    ref = ec.in_ref(dy, x, stats, gt, ac)
    want = dxa.permute(0, 2, 3, 1) + (0 if ac is None else ac.double())
    assert _rel(ref["dx"], want) < 1e-12
    assert _rel(ref["sums"][..., 0], dba) < 1e-12 and _rel(ref["sums"][..., 1], dga) < 1e-12          # dL/dbias and dL/dgate
    assert _rel(ec.host_stats(x).double(), stats) < 1e-6


def test_prelu_ref_equals_autograd_of_F_prelu():
    B, H, W, C = 2, 3, 5, 6
    g = torch.Generator().manual_seed(7)
    dy, u, slope = torch.randn(B, H, W, C, generator=g), torch.randn(B, H, W, C, generator=g), torch.randn(C, generator=g)
    u[0, 0, 0, 0], u[0, 0, 1, 0] = 0.0, -0.0
    ud, sd = u.double().permute(0, 3, 1, 2).requires_grad_(True), slope.double().requires_grad_(True)
    y = F.prelu(ud, sd)
    du, ds = torch.autograd.grad((y * dy.double().permute(0, 3, 1, 2)).sum(), (ud, sd))
    ref = ec.prelu_ref(dy, u, slope)
    assert torch.equal(ref["y"], y.detach().permute(0, 2, 3, 1))
    assert _rel(ref["du"], du.permute(0, 2, 3, 1)) < 1e-12 and _rel(ref["dslope"], ds) < 1e-12
    assert int(ref["n"].sum()) == int((u <= 0).sum()) and (ref["dslope_abs"] >= ref["dslope"].abs()).all()
    assert float(ref["du"][0, 0, 0, 0]) == float(dy[0, 0, 0, 0]) * float(slope[0])          # u == 0 takes the slope branch


@pytest.mark.parametrize("s", [1, 2, 3])
def test_scatter_ref_equals_autograd_of_strided_slicing(s):
    g = torch.Generator().manual_seed(s)
    src, prior = torch.randn(2, 3, 5, 4, generator=g), torch.randn(2, 3 * s, 5 * s, 4, generator=g)
    X = torch.zeros(2, 3 * s, 5 * s, 4, dtype=torch.float64, requires_grad=True)
    dX, = torch.autograd.grad((X[:, ::s, ::s] * src.double()).sum(), X)
    zero, hit = ec.scatter_ref(src, s)
    assert torch.equal(zero.double(), dX) and int(hit.sum()) == 15
    accum, _ = ec.scatter_ref(src, s, prior)
    assert torch.equal(accum[:, ~hit], prior[:, ~hit]) and torch.equal(accum[:, hit], prior[:, hit] + src.reshape(2, 15, 4))
    assert _rel(accum.double(), prior.double() + dX) < 1e-7


@pytest.mark.parametrize("index, c", _cases("place"), ids=[ec.case_id(c) for c in ec.PLACE_CASES])
def test_place_ref_equals_autograd_of_a_stride_s_padding_0_slicing(index, c):
    t = ec.build("place", index, "random")
    (H, W), s, (Ho, Wo) = c["grid"], c["s"], t["out_hw"]
    X = torch.zeros(c["B"], Ho, Wo, c["C"], dtype=torch.float64, requires_grad=True)
    dX, = torch.autograd.grad((X[:, c["oy"]::s, c["ox"]::s][:, :H, :W] * t["src"].double()).sum(), X)
    assert torch.equal(t["ref"].double(), dX)
    assert Ho >= ec.place_min_hw(c)[0] and Wo >= ec.place_min_hw(c)[1]


def test_place_cases_hold_the_minimum_an_odd_and_a_larger_grid_and_both_discriminator_forms():
    forms = {(c["s"], c["oy"], c["ox"]) for c in ec.PLACE_CASES}
    assert {(2, 1, 1), (2, 0, 0)} <= forms and any(f[0] == 3 for f in forms)
    hw = [(ec.build("place", i, "random")["out_hw"], ec.place_min_hw(c)) for i, c in _cases("place")]
    assert any(o == m for o, m in hw) and any(o[0] % 2 and o[1] % 2 for o, m in hw) and any(o[0] > m[0] and o[1] > m[1] for o, m in hw)


def test_unshuffle_ref_is_the_docstring_formula():
    x = torch.arange(2 * 6 * 10 * 4, dtype=torch.float32).reshape(2, 6, 10, 4)
    ref = ec.unshuffle_ref(x)
    assert ref.shape == (2, 3, 5, 16)
    for b in range(2):
        for a in range(3):
            for cc in range(5):
                for py in range(2):
                    for px in range(2):
                        assert torch.equal(ref[b, a, cc, (py * 2 + px) * 4:(py * 2 + px + 1) * 4], x[b, 2 * a + py, 2 * cc + px])
    # and it undoes F.pixel_shuffle, whose NCHW channel order is c 4 + py 2 + px
    nchw = ref.reshape(2, 3, 5, 4, 4).permute(0, 4, 3, 1, 2).reshape(2, 16, 3, 5)
    assert torch.equal(F.pixel_shuffle(nchw, 2).permute(0, 2, 3, 1), x)


@pytest.mark.parametrize("acc", [False, True])
def test_region_ref_equals_autograd_of_the_one_hot_masked_mean(acc):
    B, H, W, C, R, off = 2, 6, 7, 4, 5, 8
    g = torch.Generator().manual_seed(9 + acc)
    labels = ec.make_labels("noise", B, 5, 9, R, seed=1)
    labels[0, 0, 0], labels[1, 2, 3] = R, 255                                      # no region: no term in any mean
    reg = ec.region_map(labels, H, W)
    assert (reg >= R).any()
    dcodes = torch.randn(B, R, off + C + 4, generator=g)
    ac = torch.randn(B, H, W, C, generator=g) if acc else None
    feat = torch.randn(B, H * W, C, generator=g).double().requires_grad_(True)
    onehot = torch.stack([(reg.reshape(B, -1) == r) for r in range(R)], -1).double()              # [B, P, R]
    codes = torch.einsum("bpr,bpc->brc", onehot, feat) / onehot.sum(1).clamp(min=1)[..., None]
    dfeat, = torch.autograd.grad((codes * dcodes.double()[..., off:off + C]).sum(), feat)
    ref = ec.region_ref(dcodes, reg, R, C, off, ac)
    want = dfeat.reshape(B, H, W, C) + (0 if ac is None else ac.double())
    assert _rel(ref["dfeat"], want) < 1e-12
    assert torch.equal(ref["counts"], onehot.sum(1).long())
    assert (ref["dfeat"][~ref["valid"]] == (0 if ac is None else ac.double()[~ref["valid"]])).all()
    assert (ref["bound"][~ref["valid"]] == 0).all()


def test_unmasked_torgb_ref_is_the_plain_contraction():
    t = ec.build("torgbw", 0, "random")
    B, C = t["case"]["B"], t["case"]["C"]
    want = torch.einsum("bkp,bpc->bkc", t["drgb"].double().reshape(B, 3, -1), t["x"].double().reshape(B, -1, C))
    assert _rel(t["ref"]["dws"], want) < 1e-12 and t["ref"]["dws"].shape == (B, 3, C)


# ---- dyadic data: the formulas evaluated in fp32 give the fp64 reference bit for bit ------------------------------------------------------
def _sums_f32(terms):
    """fp32 sums over dim 1 of fp32 terms [B, N, ...] in several orders: torch's, front to back, back to front, shuffled, in blocks of 69"""
    n = terms.shape[1]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    blocks = torch.stack([terms[:, i:i + 69].sum(1) for i in range(0, n, 69)], 1)
    return [terms.sum(1), terms.cumsum(1)[:, -1], terms.flip(1).cumsum(1)[:, -1], terms[:, perm].cumsum(1)[:, -1], blocks.cumsum(1)[:, -1]]


def _same(a32, ref64):
    assert a32.dtype == torch.float32 and ref64.dtype == torch.float64
    return torch.equal(a32.double(), ref64)


@pytest.mark.parametrize("index, c", _cases("in"), ids=[ec.case_id(c) for c in ec.IN_CASES])
def test_dyadic_instnorm_is_exact_in_fp32(index, c):
    t = ec.build("in", index, "dyadic")
    ref, (B, (H, W), C) = t["ref"], (c["B"], c["grid"], c["C"])
    N = H * W
    dy, x = t["dy"].reshape(B, N, C), t["x"].reshape(B, N, C)
    mean, rstd = t["stats"][:, None, :, 0], t["stats"][:, None, :, 1]
    xh = (x - mean) * rstd
    for a in _sums_f32(dy):
        assert _same(a, ref["sums"][..., 0])
    for q in _sums_f32(dy * xh):
        assert _same(q, ref["sums"][..., 1])
    assert float(ref["S_abs"].max()) * 2 ** 5 < 2 ** 24 and float(ref["A_abs"].max()) * 2 ** 2 < 2 ** 24          # any order, any partial sum
    assert t["exact_dx"] == ec.is_pow2(N)
    if not t["exact_dx"]:
        return
    s0, s1 = ref["sums"][:, None, :, 0].float(), ref["sums"][:, None, :, 1].float()
    gt = torch.ones_like(rstd) if t["gate"] is None else t["gate"][:, None]
    invn = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(N), dtype=torch.float32)
    acc = 0 if t["acc"] is None else t["acc"].reshape(B, N, C)
    want = ref["dx"].reshape(B, N, C)
    kernel_order = rstd * gt * (dy - s0 * invn - xh * s1 * invn) + acc
    other_order = (acc + rstd * (gt * ((dy - xh * (s1 * invn)) - s0 / N))) if t["acc"] is not None else rstd * (gt * ((dy - xh * (s1 * invn)) - s0 / N))
    assert _same(kernel_order, want) and _same(other_order, want)


@pytest.mark.parametrize("name", ["prelu", "scatter", "region", "torgbw"])
def test_other_dyadic_cases_are_exact_in_fp32(name):
    for i, c in _cases(name):
        t = ec.build(name, i, "dyadic")
        cid = ec.case_id(c)
        if name == "prelu":
            C, ref = c["C"], t["ref"]
            u, dy, a = t["u"].reshape(-1, C), t["dy"].reshape(-1, C), t["slope"]
            pos = u > 0
            assert _same(torch.where(pos, u, u * a), ref["y"].reshape(-1, C)) and _same(torch.where(pos, dy, dy * a), ref["du"].reshape(-1, C)), cid
            for s in _sums_f32(torch.where(pos, torch.zeros_like(u), dy * u)[None]):
                assert _same(s[0], ref["dslope"]), cid
            assert float(ref["dslope_abs"].max()) * 2 ** 4 < 2 ** 24
        elif name == "scatter":
            assert _same(t["accum"], t["prior"].double() + t["zero"].double()), cid
        elif name == "region":
            assert t["exact"] == (c["pattern"] == "pow2"), cid
            if t["exact"]:
                ref, B = t["ref"], c["B"]
                bi = torch.arange(B)[:, None, None]
                inv = 1.0 / ref["counts"].float()                                          # one fp32 rounding, as in the kernel
                got = t["dcodes"][bi, t["reg"]][..., c["off"]:c["off"] + c["C"]] * inv[bi, t["reg"]][..., None]
                assert _same(got if t["acc"] is None else got + t["acc"], ref["dfeat"]), cid
        else:
            B, C, ref = c["B"], c["C"], t["ref"]
            terms = t["drgb"].reshape(B, 3, -1).transpose(1, 2)[..., None] * t["x"].reshape(B, -1, 1, C)
            for s in _sums_f32(terms):
                assert _same(s, ref["dws"]), cid
            assert float(ref["dws_abs"].max()) * 2 ** 4 < 2 ** 24


def test_random_instnorm_sums_keep_the_condition_of_their_bound():
    """2u |A| bounds the cast AND the double additions as long as N 2^-53 sum|dy| <= u |A| (enc_bwd_cases docstring)."""
    for i, c in _cases("in"):
        t = ec.build("in", i, "random")
        ref = ec.in_ref(t["dy"], t["x"], ec.host_stats(t["x"]), t["gate"], t["acc"])
        n = c["grid"][0] * c["grid"][1]
        assert (n * 2.0 ** -53 * ref["A_abs"] <= ec.U * ref["sums"][..., 0].abs()).all(), ec.case_id(c)
        assert (ref["dx_bound"] > 0).all() and (ref["sums_bound"] >= 0).all()


# ---- label maps ----------------------------------------------------------------------------------------------------------------------------
def test_region_label_maps_keep_their_promises():
    seen = set()
    for i, c in _cases("region"):
        t = ec.build("region", i, "random")
        lab, reg, R, B, cid = t["labels"], t["reg"], c["R"], c["B"], ec.case_id(c)
        counts = t["ref"]["counts"]
        seen.add(c["pattern"])
        assert lab.dtype == torch.uint8 and reg.shape == (B,) + c["grid"]
        if c["pattern"] == "out_of_range":
            vals = set(reg.flatten().tolist())
            assert R in vals and 255 in vals and min(v for v in vals if v >= R) == R, cid
            assert int(counts.sum()) == int((reg < R).sum()) < reg.numel()
        else:
            assert int(lab.max()) < R and int(reg.max()) < R, cid
            assert int(counts.sum()) == reg.numel()
        if c["pattern"] == "absent":
            assert int(counts[0, R - 1]) == 0 and int(counts[-1, 0]) == 0, cid
        if c["pattern"] == "pow2":
            assert all(ec.is_pow2(int(n)) for n in counts.flatten() if n > 0), cid
            assert B == 1 or not torch.equal(counts[0], counts[1]), cid                   # the neighbouring sample's count is another number
        if c["pattern"] == "one":
            assert int(counts[0, R - 1]) == reg[0].numel()
        # what the kernel must not read is NaN, what it must read is finite
        assert torch.isnan(t["dcodes"][counts == 0]).all() and torch.isfinite(t["dcodes"][counts > 0][:, c["off"]:c["off"] + c["C"]]).all()
        assert torch.isfinite(t["ref"]["dfeat"]).all(), cid
    assert seen == {"blocks", "noise", "absent", "one", "pow2", "out_of_range"}
    rows = [c for c in ec.REGION_CASES if c["pattern"] == "blocks"]
    assert {c["C"] for c in rows} == {64, 256} and {c["R"] for c in rows} == {3, 12, 16} and {c["off"] for c in rows} == {0, 64}
    assert {c["rel"] for c in rows} == {"larger", "equal", "smaller"} and {c["acc"] for c in rows} == {False, True}


def test_interpolate_nearest_is_the_integer_floor_on_every_grid_used():
    pairs = {(c["grid"], tuple(ec.build("region", i, "random")["labels"].shape[1:])) for i, c in _cases("region")}
    assert len(pairs) == 12
    for (H, W), (hm, wm) in sorted(pairs):
        idx = (torch.arange(hm)[:, None] * wm + torch.arange(wm)[None]).float()           # every map pixel its own value (< 2^24)
        got = F.interpolate(idx[None, None], size=(H, W), mode="nearest")[0, 0].long()
        want = (torch.arange(H) * hm // H)[:, None] * wm + (torch.arange(W) * wm // W)[None]
        assert torch.equal(got, want), ((H, W), (hm, wm))


# ---- split arithmetic ----------------------------------------------------------------------------------------------------------------------
def test_case_lists_reach_every_split_path():
    in_paths = {ec.split_path(c["grid"][0] * c["grid"][1], ec.in_nsplit(c["B"], c["grid"][0] * c["grid"][1], c["C"])) for c in ec.IN_CASES}
    pr_paths = {ec.split_path(c["B"] * c["grid"][0] * c["grid"][1], ec.prelu_nsplit(c["B"] * c["grid"][0] * c["grid"][1], c["C"]))
                for c in ec.PRELU_CASES if c["bwd"]}
    assert in_paths == {"single", "even", "ragged", "empty"} and pr_paths == {"single", "even", "ragged", "empty"}
    assert ec.in_nsplit(1, 65 * 65, 64) == 66 and ec.split_path(65 * 65, 66) == "empty"
    assert ec.in_nsplit(1, 13 * 37, 128) == 7 and -(-13 * 37 // 7) == 69 and ec.split_path(13 * 37, 7) == "ragged"
    for c in ec.IN_CASES:          # the split count of these cases does not depend on B: sample i of a batch is added in the same order
        hw = c["grid"][0] * c["grid"][1]
        assert ec.in_nsplit(c["B"], hw, c["C"]) == ec.in_nsplit(1, hw, c["C"])
    assert {c["C"] for c in ec.IN_CASES} == {64, 128, 192} == {c["C"] for c in ec.PRELU_CASES if c["bwd"]}
    assert {(c["gate"], c["acc"]) for c in ec.IN_CASES} == {(False, False), (False, True), (True, False), (True, True)}
