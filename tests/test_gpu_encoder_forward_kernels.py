"""The forward glue of the regional style encoder (csrc/encoder.hip: instnorm_stats, e4s_instnorm_finalize_f32, instnorm_apply with and
without the fused output statistics, se_gate, e4s_instnorm_finalize_se_f32, resize_bilinear_to_nhwc, conv3x3_small and the tiled stem
conv), each on its own against the fp64 yardsticks of tests/enc_fwd_cases.py (checked on the CPU by tests/test_enc_fwd_cases_host.py; the
bounds are derived in that module's docstring).  The rest of the suite uses these kernels as the right-hand side of bitwise comparisons.

Per case, with dyadic data every output that can EQUALS the reference (no tolerance), with random data |got - ref| <= the derived bound
elementwise.  A second call reproduces every output bit for bit; sample i of a batch-3 call equals the batch-1 call on that sample
wherever the restated split does not depend on B -- every case but the B = 8, C = 512 statistics, whose split the batch term decides
(test_enc_fwd_cases_host.test_case_lists_reach_every_path); no element of an output or of a used fp64 workspace is left unwritten, and the
elements on either side of every tensor a wrapper allocates keep their sentinel.  Geometry the ABI does not take is refused before any
launch, and so are operands of instnorm_apply whose extents do not fit x (never run: the kernels would read past their end)."""
import ctypes

import pytest
import torch

import enc_fwd_cases as ef
from guarded_alloc import DEV, _GuardedTorch, unwritten

pytestmark = pytest.mark.gpu
U = ef.U
_WORST = {}                 # kernel output -> largest observed error / bound
_RESIDUE = {}               # intrinsic -> largest observed residue in u (enc_fwd_cases: RSQRT_U, SIGMOID_U)


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
        print(f"\n[enc-fwd] largest error / bound of {k}: {_WORST[k]:.3f}", end="")
    for k in sorted(_RESIDUE):
        print(f"\n[enc-fwd] largest residue of {k}: {_RESIDUE[k]:.3f} u", end="")
    print()


def _dev(t):
    return None if t is None else t.to(DEV)


def _ids(name):
    return [ef.case_id(c) for c in ef.CASES[name]]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ratio(key, got, ref, bound):
    err = (got.cpu().double() - ref).abs()
    live = bound > 0
    if bool(live.any()):
        _WORST[key] = max(_WORST.get(key, 0.0), float((err[live] / bound[live]).max()))
    return err


def _check(key, exact, got, ref, bound, what):
    """exact: got EQUALS the fp64 reference; else |got - ref| <= bound elementwise (0 where the bound is 0)."""
    assert got.shape == ref.shape, what
    assert unwritten(got) == 0, f"{what}: {unwritten(got)} elements were never written"
    if exact:
        assert torch.equal(got.cpu(), ref.float()), f"{what}: not equal to the fp64 reference"
        return
    err = _ratio(key, got, ref, bound)
    ok = err <= bound
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements outside the bound, worst error {float(err[~ok].max()):.3e}"


def _check_stats(key, stats, r, what, exact_mean=False, output=False, measure=False):
    """stats [B, C, 2] against stats_ref `r`.  output: the tensor is a kernel's output (the mean bound carries the double additions)."""
    assert stats.shape == r["mean"].shape + (2,), what
    _check(key + " mean", exact_mean, stats[..., 0], r["mean"], r["mean_bound_sum" if output else "mean_bound"], what + " mean")
    _check(key + " rstd", False, stats[..., 1], r["rstd"], r["rstd_bound"], what + " rstd")
    if measure:          # the intrinsic's own residue: everything else of the chain is fixed by the reference
        res = float(((stats[..., 1].cpu().double() - r["restated"]).abs() / (U * r["restated"])).max())
        _RESIDUE["rsqrtf (relative to rstd)"] = max(_RESIDUE.get("rsqrtf (relative to rstd)", 0.0), res)


def _hw(c):
    return c["grid"][0] * c["grid"][1]


@pytest.mark.parametrize("index", range(len(ef.STATS_CASES)), ids=_ids("stats"))
def test_instnorm_stats_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in ef.KINDS:
        t = ef.build("stats", index, kind)
        c, r = t["case"], t["ref"]
        B, C, HW, eps = c["B"], c["C"], _hw(c), c["eps"]
        what = f"instnorm_stats {ef.case_id(c)} {kind}"
        x = _dev(t["x"])
        stats, pooled = K.instnorm_stats(x, want_pooled=True, eps=eps)
        ws = guard.insides(torch.float64)[-1]
        # the one-launch kernel has no use for the workspace; the split path fills every slot
        assert ws.numel() == 2 * B * C * ef.instnorm_nsplit(B, HW, C), what
        assert unwritten(ws) == (ws.numel() if ef.stats_is_small(HW) else 0), what + ": the fp64 workspace"
        guard.check()
        _check_stats("instnorm_stats", stats, r, what, exact_mean=t["exact_mean"], measure=True)
        pref, pbound = ef.pooled_ref(t["x"], stats.cpu())
        _check("instnorm_stats pooled", False, pooled, pref, pbound, what + " pooled")
        if t["exact_mean"]:
            assert float(pooled.abs().max()) == 0.0, what + ": the mean is an fp32 number, its residue is 0"
        if kind == "random":          # true variance 0: the clamp yields rsqrt(eps)
            _ratio("instnorm_stats rstd", stats[0, 0, 1], r["rstd"][0, 0], r["rstd_bound"][0, 0])
            assert abs(float(stats[0, 0, 1]) - ef.f32(eps) ** -0.5) <= float(r["rstd_bound"][0, 0]), what + ": constant channel"
        only, none = K.instnorm_stats(x, eps=eps)
        assert none is None and _same_bits(only, stats), what + ": the statistics depend on want_pooled"
        stats2, pooled2 = K.instnorm_stats(x, want_pooled=True, eps=eps)
        assert _same_bits(stats, stats2) and _same_bits(pooled, pooled2), what + ": second call differs"
        if 1 < B <= 3:          # B = 8: the batch term of instnorm_nsplit decides the split there
            assert ef.stats_is_small(HW) or ef.instnorm_nsplit(B, HW, C) == ef.instnorm_nsplit(1, HW, C)
            for i in range(B):
                si, pi = K.instnorm_stats(x[i:i + 1], want_pooled=True, eps=eps)
                assert _same_bits(si[0], stats[i]) and _same_bits(pi[0], pooled[i]), what + f": sample {i} depends on the batch"
        guard.check()


def _finalize(guard, slots, B, HW, C, nslots, want_pooled):
    from e4s_amd.lib import call, fptr, ptr, stream
    stats = guard.empty(B, C, 2, device=DEV)
    pooled = guard.empty(B, C, device=DEV) if want_pooled else None
    call("e4s_instnorm_finalize_f32", ptr(slots), fptr(stats), fptr(pooled), B, HW, C, nslots, ef.EPS, stream())
    guard.check()
    return stats, pooled


@pytest.mark.parametrize("index", range(len(ef.FINALIZE_CASES)), ids=_ids("finalize"))
def test_instnorm_finalize_on_hand_made_slots(index, guard):
    for kind in ef.KINDS:
        t = ef.build("finalize", index, kind)
        c, r = t["case"], t["ref"]
        B, C, ns = c["B"], c["C"], c["nslots"]
        what = f"instnorm_finalize {ef.case_id(c)} {kind}"
        slots = _dev(t["slots"])
        stats, pooled = _finalize(guard, slots, B, ef.FINALIZE_HW, C, ns, True)
        _check_stats("instnorm_finalize", stats, r, what, exact_mean=t["exact"])
        pref, pbound = ef.pooled_ref(t["x"], stats.cpu())
        _check("instnorm_finalize pooled", False, pooled, pref, pbound, what + " pooled")
        if t["exact"]:
            assert float(pooled.abs().max()) == 0.0, what + ": dyadic slots leave no residue"
        only, none = _finalize(guard, slots, B, ef.FINALIZE_HW, C, ns, False)
        assert none is None and _same_bits(only, stats), what + ": the statistics depend on pooled"
        again, pagain = _finalize(guard, slots, B, ef.FINALIZE_HW, C, ns, True)
        assert _same_bits(again, stats) and _same_bits(pagain, pooled), what + ": second call differs"


def _apply_kw(t, o, sl=slice(None)):
    kw = ef.apply_operands(t, o)
    cpu = {k: (v if k in ("slope", "rs") or v is None else v[sl]) for k, v in kw.items()}
    return cpu, {k: (v if k == "rs" else _dev(v)) for k, v in cpu.items()}


@pytest.mark.parametrize("index", range(len(ef.APPLY_CASES)), ids=_ids("apply"))
def test_instnorm_apply_option_lattice_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in ef.KINDS:
        t = ef.build("apply", index, kind)
        c, B = t["case"], t["case"]["B"]
        x, stats = _dev(t["x"]), _dev(t["stats"])
        for o in ef.APPLY_OPTIONS:
            what = f"instnorm_apply {ef.case_id(c)} {ef.option_id(o)} {kind}"
            cpu, dev = _apply_kw(t, o)
            ref, bound = ef.apply_ref(t["x"], t["stats"], **cpu)
            y = K.instnorm_apply(x, stats, **dev)
            guard.check()
            _check("instnorm_apply y", t["exact"], y, ref, bound, what)
            assert _same_bits(y, K.instnorm_apply(x, stats, **dev)), what + ": second call differs"
            for i in range(B if B > 1 else 0):
                _, devi = _apply_kw(t, o, slice(i, i + 1))
                assert _same_bits(K.instnorm_apply(x[i:i + 1], stats[i:i + 1], **devi)[0], y[i]), what + f": sample {i} depends on the batch"
            guard.check()


@pytest.mark.parametrize("index", range(len(ef.APPLY_STATS_CASES)), ids=_ids("apply_stats"))
def test_instnorm_apply_with_fused_output_statistics(index, guard):
    from e4s_amd import kernels as K, lib
    from e4s_amd.lib import call, fptr, ptr, stream
    for kind in ef.KINDS:
        t = ef.build("apply_stats", index, kind)
        c, B, C, (H, W) = t["case"], t["case"]["B"], t["case"]["C"], t["case"]["grid"]
        HW, ns = H * W, ef.instnorm_nsplit(t["case"]["B"], H * W, t["case"]["C"])
        x, stats = _dev(t["x"]), _dev(t["stats"])
        for o in ef.APPLY_OPTIONS:
            what = f"instnorm_apply(want_stats) {ef.case_id(c)} {ef.option_id(o)} {kind}"
            cpu, dev = _apply_kw(t, o)
            plain = K.instnorm_apply(x, stats, **dev)
            guard.check()
            y, st = K.instnorm_apply(x, stats, want_stats=True, **dev)
            ws = guard.insides(torch.float64)[-1]
            assert ws.numel() == 2 * B * C * ns and unwritten(ws) == 0, what + ": a slot of the fp64 workspace was never written"
            guard.check()
            assert _same_bits(y, plain), what + ": y differs from the plain apply"
            ref, bound = ef.apply_ref(t["x"], t["stats"], **cpu)
            _check("instnorm_apply(want_stats) y", t["exact"], y, ref, bound, what)
            _check_stats("instnorm_apply(want_stats) out", st, ef.stats_ref(y.cpu()), what + " output statistics", output=True)
            # the ABI itself: the slot count it reports is the restated split, and finalising its slots gives the wrapper's statistics
            y2, ws2, n2 = guard.empty_like(x), guard.empty(lib.load().e4s_instnorm_ws_doubles(B, HW, C), device=DEV, dtype=torch.float64), ctypes.c_int(0)
            call("e4s_instnorm_apply_stats_f32", fptr(x), fptr(stats), fptr(dev["gate"]), fptr(dev["res"]), fptr(dev["res_stats"]),
                 fptr(dev["slope"]), fptr(y2), ptr(ws2), ctypes.byref(n2), B, H, W, C, dev["rs"], stream())
            assert n2.value == ns and ws2.numel() == 2 * B * C * ns, what + ": nslots"
            assert unwritten(ws2) == 0 and _same_bits(y2, y) and torch.equal(ws2, ws), what + ": the ABI call differs from the wrapper's"
            guard.check()
            st2, _ = _finalize(guard, ws2, B, HW, C, n2.value, False)
            assert _same_bits(st2, st), what + ": finalising the slots by hand"
            for i in range(B if B > 1 else 0):          # the split of these cases does not depend on B
                _, devi = _apply_kw(t, o, slice(i, i + 1))
                yi, sti = K.instnorm_apply(x[i:i + 1], stats[i:i + 1], want_stats=True, **devi)
                assert _same_bits(yi[0], y[i]) and _same_bits(sti[0], st[i]), what + f": sample {i} depends on the batch"
            guard.check()


@pytest.mark.parametrize("index", range(len(ef.SE_CASES)), ids=_ids("se"))
def test_se_gate_vs_f64_and_fused_with_the_finalisation(index, guard):
    from e4s_amd import kernels as K
    from e4s_amd.lib import call, fptr, ptr, stream
    c = ef.SE_CASES[index]
    B, C, Cr = c["B"], c["C"], c["Cr"]
    for kind in ef.kinds_of("se", c):
        t = ef.build("se", index, kind)
        ref = t["ref"]
        what = f"se_gate {ef.case_id(c)} {kind}"
        pooled, fc1, fc2 = _dev(t["pooled"]), _dev(t["fc1"]), _dev(t["fc2"])
        gate = K.se_gate(pooled, fc1, fc2)
        guard.check()
        _check(f"se_gate ({'exact pre-activation' if kind == 'dyadic' else c['regime']})", False, gate, ref["gate"], ref["bound"], what)
        if kind == "dyadic":          # the pre-activation is exact in fp32: what is left is the sigmoid's own error
            res = float((gate.cpu().double() - ref["gate"]).abs().max() / U)
            _RESIDUE["sigmoid (absolute)"] = max(_RESIDUE.get("sigmoid (absolute)", 0.0), res)
        else:
            assert float((gate - 0.5).abs().max()) > 1e-4, what + ": the gate does not move"
        assert _same_bits(gate, K.se_gate(pooled, fc1, fc2)), what + ": second call differs"
        for i in range(B if B > 1 else 0):
            assert _same_bits(K.se_gate(pooled[i:i + 1], fc1, fc2)[0], gate[i]), what + f": sample {i} depends on the batch"
        guard.check()
        if kind != "random":
            continue
        # the fused finalisation + gate on hand-made slots: the statistics of e4s_instnorm_finalize_f32 and the gate of se_gate on its pooled
        slots = _dev(t["slots"])
        st_f, pooled_f = _finalize(guard, slots, B, ef.FINALIZE_HW, C, ef.SE_NSLOTS, True)
        st_s, gate_s = guard.empty(B, C, 2, device=DEV), guard.empty(B, C, device=DEV)
        call("e4s_instnorm_finalize_se_f32", ptr(slots), fptr(st_s), fptr(fc1), fptr(fc2), fptr(gate_s), B, ef.FINALIZE_HW, C, Cr,
             ef.SE_NSLOTS, ef.EPS, stream())
        guard.check()
        assert unwritten(st_s) == 0 and unwritten(gate_s) == 0, what + ": finalize_se left an element unwritten"
        assert _same_bits(st_s, st_f), what + ": finalize_se statistics differ from finalize"
        assert _same_bits(gate_s, K.se_gate(pooled_f, fc1, fc2)), what + ": finalize_se gate differs from se_gate on that pooled"
        fref = ef.se_ref(pooled_f.cpu(), t["fc1"], t["fc2"])
        _check(f"finalize_se gate ({c['regime']})", False, gate_s, fref["gate"], fref["bound"], what + " finalize_se")
        if c["regime"] == "residue":
            assert float((gate_s - 0.5).abs().max()) > 1e-4, what + ": the fused gate does not move"
        guard.check()


@pytest.mark.parametrize("index", range(len(ef.RESIZE_CASES)), ids=_ids("resize"))
def test_resize_bilinear_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in ef.KINDS:
        t = ef.build("resize", index, kind)
        c, B = t["case"], t["case"]["B"]
        what = f"resize_bilinear_to_nhwc {ef.case_id(c)} {kind}"
        x = _dev(t["x"])
        y = K.resize_bilinear_to_nhwc(x, *c["dst"])
        guard.check()
        _check("resize_bilinear_to_nhwc", t["exact"], y, t["ref"], t["bound"], what)
        assert _same_bits(y, K.resize_bilinear_to_nhwc(x, *c["dst"])), what + ": second call differs"
        for i in range(B):
            assert _same_bits(K.resize_bilinear_to_nhwc(x[i:i + 1], *c["dst"])[0], y[i]), what + f": sample {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(ef.CONV_CASES)), ids=_ids("conv"))
def test_stem_conv_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in ef.KINDS:
        t = ef.build("conv", index, kind)
        c, B = t["case"], t["case"]["B"]
        what = f"conv3x3_small {ef.case_id(c)} {kind}"
        key = "conv3x3 stem (tiled)" if c["tiled"] else "conv3x3_small"
        x, w = _dev(t["x"]), _dev(t["w"])
        y = K.conv3x3_small(x, w)
        guard.check()
        _check(key, t["exact"], y, t["ref"], t["bound"], what)
        assert _same_bits(y, K.conv3x3_small(x, w)), what + ": second call differs"
        if c["Cout"] % 64 == 0:
            y2, st = K.conv3x3_small(x, w, want_stats=True)
            if c["tiled"]:          # one fp64 slot pair per (sample, channel, tile)
                ws = guard.insides(torch.float64)[-1]
                assert ws.numel() == 2 * B * 64 * (c["grid"][0] // 16) * (c["grid"][1] // 16) and unwritten(ws) == 0, what + ": the fp64 slots"
            guard.check()
            assert _same_bits(y2, y), what + ": y depends on want_stats"
            _check_stats(key + " statistics", st, ef.stats_ref(y.cpu()), what + " statistics", output=True)
        for i in range(B if B > 1 else 0):
            assert _same_bits(K.conv3x3_small(x[i:i + 1], w)[0], y[i]), what + f": sample {i} depends on the batch"
        guard.check()


def _nothing_was_written(guard):
    """every tensor a refused wrapper had allocated still holds what empty() put there, and its neighbours their sentinel"""
    for buf in guard.insides(torch.float32) + guard.insides(torch.float64):
        assert unwritten(buf) == buf.numel(), "a refused call wrote to a tensor"
    guard.check()


def test_geometry_outside_the_kernels_sets_is_refused_before_any_launch(guard):
    from e4s_amd import kernels as K
    from e4s_amd.lib import call, fptr, ptr, stream
    z = lambda *sh: torch.zeros(*sh, device=DEV)                                                     # noqa: E731
    one = lambda *sh: torch.ones(*sh, device=DEV)                                                    # noqa: E731
    slots = torch.zeros(12288 * 2, device=DEV, dtype=torch.float64)
    refused = [
        lambda: K.instnorm_stats(z(1, 4, 4, 96)),                                                       # C % 64 (the one-launch kernel's range)
        lambda: K.instnorm_stats(z(1, 2, 2, 96), want_pooled=True),                                     # C % 64 (the split path's)
        lambda: K.instnorm_apply(z(1, 4, 4, 6), one(1, 6, 2)),                                          # C % 4
        lambda: K.instnorm_apply(z(1, 4, 4, 6), one(1, 6, 2), want_stats=True),
        lambda: K.instnorm_apply(z(1, 4, 4, 64), one(1, 64, 2), rs=0),                                  # rs < 1
        lambda: K.instnorm_apply(z(1, 4, 4, 64), one(1, 64, 2), rs=0, want_stats=True),
        lambda: K.instnorm_apply(z(1, 4, 4, 64), one(1, 64, 2), rs=-1),
        lambda: K.conv3x3_small(z(1, 5, 5, 3), z(6, 3, 3, 3)),                                          # Cout % 4
        lambda: K.conv3x3_small(z(1, 5, 5, 32), z(64, 32, 3, 3)),                                       # 72 KB of weights
        lambda: K.se_gate(z(1, 12288), z(4, 12288), z(12288, 4)),                                       # (C + Cr) 4 = 49168 B > 48 KB
        lambda: call("e4s_instnorm_finalize_se_f32", ptr(slots), fptr(guard.empty(1, 12288, 2, device=DEV)), fptr(z(4, 12288)),
                     fptr(z(12288, 4)), fptr(guard.empty(1, 12288, device=DEV)), 1, 16, 12288, 4, 1, ef.EPS, stream()),
    ]
    for call_ in refused:
        with pytest.raises(RuntimeError):
            call_()
        torch.cuda.synchronize()
        _nothing_was_written(guard)
    # the largest the gate takes is taken
    assert K.se_gate(z(1, 12284), z(4, 12284), z(12284, 4)).shape == (1, 12284)
    guard.check()


def test_instnorm_apply_refuses_operands_that_do_not_fit_x(guard):
    """The kernels index res as [B, H rs, W rs, C] and the tables by (b, c) without looking: none of these calls may reach them."""
    from e4s_amd import kernels as K
    z = lambda *sh: torch.zeros(*sh, device=DEV)                                                     # noqa: E731
    one = lambda *sh: torch.ones(*sh, device=DEV)                                                    # noqa: E731
    x, st = z(2, 8, 8, 64), one(2, 64, 2)
    mismatched = [
        dict(res=z(2, 15, 15, 64), rs=2),                      # the residual of an odd map: 15^2 -> 8^2 at stride 2
        dict(res=z(2, 16, 16, 64), rs=1),
        dict(res=z(2, 8, 8, 64), rs=2),
        dict(res=z(2, 8, 8, 128)),
        dict(res=z(1, 8, 8, 64)),
        dict(res=z(2, 8, 8, 64), res_stats=one(1, 64, 2)),
        dict(res=z(2, 8, 8, 64), res_stats=one(2, 64)),
        dict(gate=one(1, 64)),
        dict(gate=one(2, 32)),
        dict(slope=one(32)),
        dict(slope=one(2, 64)),
    ]
    for kw in mismatched:
        for want_stats in (False, True):
            with pytest.raises(ValueError):
                K.instnorm_apply(x, st, want_stats=want_stats, **kw)
            assert not guard.bufs, "a refused call had already allocated its output"
    for bad in (one(2, 64), one(1, 64, 2), one(2, 32, 2)):
        with pytest.raises(ValueError):
            K.instnorm_apply(x, bad)
        assert not guard.bufs
    # operands that fit are taken, in whatever shape holds the right elements (a PReLU weight [C], a gate [B, C, 1, 1])
    y = K.instnorm_apply(x, st, gate=one(2, 64, 1, 1), res=z(2, 16, 16, 64), rs=2, slope=one(64))
    guard.check()
    assert y.shape == x.shape and unwritten(y) == 0
