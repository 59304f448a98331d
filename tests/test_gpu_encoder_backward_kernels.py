"""The streaming kernels of the encoder backward (csrc/encoder_bwd.hip: instnorm_bwd, instnorm_bwd_sums, prelu, prelu_bwd, strided_scatter,
strided_place, pixel_unshuffle2, region_mean_bwd) and the unmasked torgb_bwd_w, each on its own against the fp64 yardsticks of
tests/enc_bwd_cases.py (checked on the CPU by tests/test_enc_bwd_cases_host.py; the bounds are derived in that module's docstring).

Per case, with dyadic data every output EQUALS the reference (no tolerance: a dropped, doubled or mis-filed pixel fails), except the two
quotients by a number that is no power of two, which keep the bound; with random data |got - ref| <= the derived bound elementwise.  The
copies (scatters, pixel_unshuffle2) are torch.equal with both kinds.  A second call reproduces every output bit for bit, sample i of a
batch-3 call equals the batch-1 call on that sample, positions an accumulating kernel must not touch keep their bits, no element of an
output is left unwritten, and the elements on either side of every tensor a wrapper allocates (fp32 outputs and partials, the fp64
workspace, the int32 counts) keep their sentinel.  Geometry a kernel does not take is refused before any launch."""
import pytest
import torch

import enc_bwd_cases as ec
from guarded_alloc import DEV, _GuardedTorch, unwritten

pytestmark = pytest.mark.gpu
U = ec.U
_WORST = {}                 # kernel output -> largest observed error / bound


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
        print(f"\n[enc-bwd] largest error / bound of {k}: {_WORST[k]:.3f}", end="")
    print()


def _dev(t):
    return None if t is None else t.to(DEV)


def _ids(name):
    return [ec.case_id(c) for c in ec.CASES[name]]


def _bits(t):
    return t.contiguous().view(torch.int32)


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
        assert torch.equal(got.cpu(), ref.float()), f"{what}: not equal to the fp64 reference on dyadic data"
        return
    err = _ratio(key, got, ref, bound)
    ok = err <= bound
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements outside the bound, worst error {float(err[~ok].max()):.3e}"


@pytest.mark.parametrize("index", range(len(ec.IN_CASES)), ids=_ids("in"))
def test_instnorm_bwd_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in ec.KINDS:
        t = ec.build("in", index, kind)
        c, B = t["case"], t["case"]["B"]
        what = f"instnorm_bwd {ec.case_id(c)} {kind}"
        dy, x, gate = _dev(t["dy"]), _dev(t["x"]), _dev(t["gate"])
        if kind == "random":          # the fp32 statistics of the forward; the reference takes exactly these
            stats = K.instnorm_stats(x)[0]
            guard.check()
            want = ec.host_stats(t["x"])
            assert torch.allclose(stats.cpu(), want, rtol=1e-4, atol=1e-5), what + ": instnorm_stats is far from the statistics of x"
            ref = ec.in_ref(t["dy"], t["x"], stats.cpu(), t["gate"], t["acc"])
        else:
            stats, ref = _dev(t["stats"]), t["ref"]

        def run(sl=slice(None)):
            acc = None if t["acc"] is None else guard.place(t["acc"][sl])          # random values beforehand, sentinels around them
            dx, sums = K.instnorm_bwd(dy[sl], x[sl], stats[sl], None if gate is None else gate[sl], dx_acc=acc)
            assert acc is None or dx.data_ptr() == acc.data_ptr()
            return dx, sums

        dx, sums = run()
        ws = guard.insides(torch.float64)[-1]
        assert unwritten(ws) == 0, what + ": a slot of the fp64 workspace was never written (an empty split writes zeros)"
        guard.check()
        _check("instnorm_bwd sums[0]", t["exact"], sums[..., 0], ref["sums"][..., 0], ref["sums_bound"][..., 0], what + " sum dy")
        _check("instnorm_bwd sums[1]", t["exact"], sums[..., 1], ref["sums"][..., 1], ref["sums_bound"][..., 1], what + " sum dy xhat")
        _check("instnorm_bwd dx", t["exact_dx"], dx, ref["dx"], ref["dx_bound"], what + " dx")
        if not t["exact_dx"]:
            _ratio("instnorm_bwd dx (12 u form, not asserted)", dx, ref["dx"], ref["dx_bound12"])
        only = K.instnorm_bwd_sums(dy, x, stats)
        guard.check()
        assert torch.equal(only, sums), what + ": instnorm_bwd_sums differs from the sums of instnorm_bwd"
        dx2, sums2 = run()
        assert torch.equal(_bits(dx), _bits(dx2)) and torch.equal(_bits(sums), _bits(sums2)), what + ": second call differs"
        # the split count of these cases does not depend on B (test_case_lists_reach_every_split_path): the same additions in the same order
        for i in range(B if B > 1 else 0):
            dxi, sumsi = run(slice(i, i + 1))
            assert torch.equal(_bits(dxi[0]), _bits(dx[i])) and torch.equal(_bits(sumsi[0]), _bits(sums[i])), what + f": sample {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(ec.PRELU_CASES)), ids=_ids("prelu"))
def test_prelu_and_prelu_bwd_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in ec.KINDS:
        t = ec.build("prelu", index, kind)
        c, ref = t["case"], t["ref"]
        what = f"prelu {ec.case_id(c)} {kind}"
        dy, u, slope = _dev(t["dy"]), _dev(t["u"]), _dev(t["slope"])
        y = K.prelu(u, slope)
        guard.check()
        _check("prelu y", t["exact"], y, ref["y"], ref["y_bound"], what + " y")
        assert torch.equal(y.cpu()[t["u"] > 0], t["u"][t["u"] > 0]), what + ": a positive input is not copied"
        if not c["bwd"]:
            continue
        du, dslope = K.prelu_bwd(dy, u, slope)
        guard.check()
        _check("prelu_bwd du", t["exact"], du, ref["du"], ref["du_bound"], what + " du")
        _check("prelu_bwd dslope", t["exact"], dslope, ref["dslope"], (ref["n"].double() + 4) * U * ref["dslope_abs"], what + " dslope")
        assert float(dslope[0]) == 0.0 and int(ref["n"][0]) == 0, what + ": dslope of the all-positive channel is not exactly 0"
        assert int(ref["n"][1]) == u.numel() // c["C"]
        du2, dslope2 = K.prelu_bwd(dy, u, slope)
        assert torch.equal(_bits(du), _bits(du2)) and torch.equal(_bits(dslope), _bits(dslope2)), what + ": second call differs"
        guard.check()


@pytest.mark.parametrize("index", range(len(ec.SCATTER_CASES)), ids=_ids("scatter"))
def test_strided_scatter_is_exact_in_both_modes(index, guard):
    from e4s_amd import kernels as K
    for kind in ec.KINDS:
        t = ec.build("scatter", index, kind)
        c, s, B, hit = t["case"], t["case"]["s"], t["case"]["B"], t["hit"]
        what = f"strided_scatter {ec.case_id(c)} {kind}"
        src = _dev(t["src"])
        out = K.strided_scatter(src, s)
        guard.check()
        assert unwritten(out) == 0 and torch.equal(out.cpu(), t["zero"]), what + ": zero-insert mode"
        acc = guard.place(t["prior"])
        assert K.strided_scatter(src, s, out=acc).data_ptr() == acc.data_ptr()
        guard.check()
        got = acc.cpu()
        assert torch.equal(got[:, hit], t["accum"][:, hit]), what + ": a hit position is not prior + src"
        assert torch.equal(_bits(got[:, ~hit]), _bits(t["prior"][:, ~hit])), what + ": a position between the hits was rewritten"
        for i in range(B if B > 1 else 0):
            assert torch.equal(K.strided_scatter(src[i:i + 1], s)[0], out[i]), what + f": sample {i} depends on the batch"
            acci = guard.place(t["prior"][i:i + 1])
            K.strided_scatter(src[i:i + 1], s, out=acci)
            assert torch.equal(_bits(acci[0]), _bits(acc[i])), what + f": sample {i} depends on the batch (accumulate)"
        guard.check()


@pytest.mark.parametrize("index", range(len(ec.PLACE_CASES)), ids=_ids("place"))
def test_strided_place_is_exact(index, guard):
    from e4s_amd import kernels as K
    for kind in ec.KINDS:
        t = ec.build("place", index, kind)
        c, B = t["case"], t["case"]["B"]
        what = f"strided_place {ec.case_id(c)} {kind}"
        src = _dev(t["src"])
        out = K.strided_place(src, c["s"], c["oy"], c["ox"], t["out_hw"])
        guard.check()
        assert unwritten(out) == 0 and torch.equal(out.cpu(), t["ref"]), what
        for i in range(B if B > 1 else 0):
            assert torch.equal(K.strided_place(src[i:i + 1], c["s"], c["oy"], c["ox"], t["out_hw"])[0], out[i]), what + f": sample {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(ec.UNSHUFFLE_CASES)), ids=_ids("unshuffle"))
def test_pixel_unshuffle2_is_exact(index, guard):
    from e4s_amd import kernels as K
    for kind in ec.KINDS:
        t = ec.build("unshuffle", index, kind)
        c, B = t["case"], t["case"]["B"]
        what = f"pixel_unshuffle2 {ec.case_id(c)} {kind}"
        x = _dev(t["x"])
        out = K.pixel_unshuffle2(x)
        guard.check()
        assert unwritten(out) == 0 and torch.equal(out.cpu(), t["ref"]), what
        for i in range(B if B > 1 else 0):
            assert torch.equal(K.pixel_unshuffle2(x[i:i + 1])[0], out[i]), what + f": sample {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(ec.REGION_CASES)), ids=_ids("region"))
def test_region_mean_bwd_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in ec.KINDS:
        t = ec.build("region", index, kind)
        c, ref, R, B = t["case"], t["ref"], t["case"]["R"], t["case"]["B"]
        (H, W), C = c["grid"], c["C"]
        what = f"region_mean_bwd {ec.case_id(c)} {kind}"
        dcodes, labels = _dev(t["dcodes"]), _dev(t["labels"])          # NaN in every row and column the kernel has no business reading

        def run(sl=slice(None)):
            acc = None if t["acc"] is None else guard.place(t["acc"][sl])
            dfeat = K.region_mean_bwd(dcodes[sl], labels[sl], R, (labels[sl].shape[0], H, W, C), c["off"], dfeat_acc=acc)
            assert acc is None or dfeat.data_ptr() == acc.data_ptr()
            return dfeat, guard.insides(torch.int32)[-1].clone()

        dfeat, counts = run()
        guard.check()
        assert unwritten(counts) == 0 and torch.equal(counts.cpu().long(), ref["counts"].flatten()), what + ": the counts table"
        assert bool(torch.isfinite(dfeat).all()), what + ": NaN or Inf in dfeat (an absent region's row or a column outside the window was read)"
        _check("region_mean_bwd dfeat", t["exact"], dfeat, ref["dfeat"], ref["bound"], what)
        outside = ~ref["valid"]
        if bool(outside.any()):        # a label >= R belongs to no region: 0, or the bits that were there
            before = torch.zeros(B, H, W, C) if t["acc"] is None else t["acc"]
            assert torch.equal(_bits(dfeat.cpu()[outside]), _bits(before[outside])), what + ": a pixel of no region was written"
        dfeat2, counts2 = run()
        assert torch.equal(_bits(dfeat), _bits(dfeat2)) and torch.equal(counts, counts2), what + ": second call differs"
        for i in range(B if B > 1 else 0):
            dfi, cnti = run(slice(i, i + 1))
            assert torch.equal(_bits(dfi[0]), _bits(dfeat[i])) and torch.equal(cnti, counts[i * R:(i + 1) * R]), what + f": sample {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(ec.TORGBW_CASES)), ids=_ids("torgbw"))
def test_unmasked_torgb_bwd_w_vs_f64(index, guard):
    from e4s_amd import kernels as K, lib
    for kind in ec.KINDS:
        t = ec.build("torgbw", index, kind)
        c, ref, B = t["case"], t["ref"], t["case"]["B"]
        (H, W), C = c["grid"], c["C"]
        what = f"torgb_bwd_w {ec.case_id(c)} {kind}"
        drgb, x = _dev(t["drgb"]), _dev(t["x"])
        dws = K.torgb_bwd_w(drgb, x)
        guard.check()
        _check("torgb_bwd_w dws", t["exact"], dws, ref["dws"], (H * W + 4) * U * ref["dws_abs"], what)
        assert torch.equal(_bits(dws), _bits(K.torgb_bwd_w(drgb, x))), what + ": second call differs"
        nsplit = lib.load().e4s_seg_reduce_nsplit
        if B > 1 and nsplit(B, H, W, C) == nsplit(1, H, W, C):          # the same splits: the same additions in the same order
            for i in range(B):
                assert torch.equal(_bits(K.torgb_bwd_w(drgb[i:i + 1], x[i:i + 1])[0]), _bits(dws[i])), what + f": sample {i} depends on the batch"
        guard.check()


def _nothing_was_written(guard):
    """every tensor a refused wrapper had allocated still holds what empty() put there, and its neighbours their sentinel"""
    for buf in guard.insides(torch.float32) + guard.insides(torch.float64) + guard.insides(torch.int32):
        assert unwritten(buf) == buf.numel(), "a refused call wrote to a tensor"
    guard.check()


def test_geometry_outside_the_kernels_sets_is_refused_before_any_launch(guard):
    from e4s_amd import kernels as K
    z = lambda *sh: torch.zeros(*sh, device=DEV)                                                     # noqa: E731
    stats = torch.ones(1, 96, 2, device=DEV)
    labels = torch.zeros(1, 4, 4, dtype=torch.uint8, device=DEV)
    refused = [
        lambda: K.instnorm_bwd(z(1, 4, 4, 96), z(1, 4, 4, 96), stats),                                  # C % 64
        lambda: K.instnorm_bwd(z(1, 4, 4, 32), z(1, 4, 4, 32), stats[:, :32].contiguous(), dx_acc=guard.empty(1, 4, 4, 32, device=DEV)),
        lambda: K.instnorm_bwd_sums(z(1, 4, 4, 96), z(1, 4, 4, 96), stats),
        lambda: K.prelu_bwd(z(1, 4, 4, 96), z(1, 4, 4, 96), z(96)),                                     # C % 64
        lambda: K.prelu(z(1, 4, 4, 6), z(6)),                                                           # C % 4
        lambda: K.strided_scatter(z(1, 4, 4, 6), 2),
        lambda: K.strided_scatter(z(1, 4, 4, 6), 2, out=guard.empty(1, 8, 8, 6, device=DEV)),
        lambda: K.strided_place(z(1, 4, 4, 6), 2, 1, 1, (8, 8)),
        lambda: K.pixel_unshuffle2(z(1, 4, 4, 6)),
        lambda: K.region_mean_bwd(z(1, 3, 8), labels, 3, (1, 4, 4, 6), 0),
        lambda: K.strided_place(z(1, 5, 7, 4), 2, 1, 1, (9, 14)),                                       # one row short of (10, 14)
        lambda: K.strided_place(z(1, 5, 7, 4), 2, 1, 1, (10, 13)),                                      # one column short
        lambda: K.strided_place(z(1, 5, 7, 4), 2, 0, 0, (8, 13)),                                       # one row short of (9, 13)
        lambda: K.region_mean_bwd(z(1, 17, 64), labels, 17, (1, 4, 4, 64), 0),                          # R = 17
        lambda: K.region_mean_bwd(z(1, 17, 64), labels, 17, (1, 4, 4, 64), 0, dfeat_acc=guard.empty(1, 4, 4, 64, device=DEV)),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(RuntimeError):
            call()
        torch.cuda.synchronize()
        _nothing_was_written(guard)
    # the minimum itself is taken
    assert K.strided_place(z(1, 5, 7, 4), 2, 1, 1, (10, 14)).shape == (1, 10, 14, 4)
    guard.check()
