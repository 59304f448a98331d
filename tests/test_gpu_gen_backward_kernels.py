"""The streaming kernels of the generator backward (act_bwd_demod, demod_grad, torgb_bwd, region_scale, col2im_region, scale_dot), each
on its own against the fp64 yardsticks of tests/gen_bwd_cases.py (checked on the CPU by tests/test_gen_bwd_cases_host.py).

Per case, with dyadic data every output EQUALS the reference (no tolerance: a dropped, doubled or mis-filed pixel fails); with random data
|got - ref| <= (N + 4) 2^-24 S_abs elementwise, N the number of terms of that output (capped at H W) and S_abs the sum of their absolute
values -- the bound of an fp32 sum of N terms in any order plus the roundings inside one term, derived and not measured.  Rows of regions
absent from a sample are exactly 0.0, a second call reproduces every summed output bit for bit, sample i of a batch-3 call equals the
batch-1 call on that sample, and the floats on either side of every tensor a wrapper allocates keep their sentinel."""
import pytest
import torch

import gen_bwd_cases as gc
from guarded_alloc import PAD, SENTINEL, _GuardedTorch  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
_WORST = {}                 # kernel output -> largest observed error / bound on random data


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
        print(f"\n[gen-bwd] largest error / bound of {k}: {_WORST[k]:.3f}", end="")
    print()


def _dev(t):
    return None if t is None else t.to(DEV)


def _exact(got, ref, what):
    assert torch.equal(got.cpu(), ref.float()), f"{what}: not equal to the fp64 reference on dyadic data"


def _within(key, got, ref, sabs, n, what):
    """|got - ref| <= (n + 4) 2^-24 S_abs elementwise; n an int or one count per leading row."""
    if torch.is_tensor(n):
        n = n.double().reshape(-1, *([1] * (ref.dim() - 1)))
    err, bound = (got.cpu().double() - ref).abs(), (n + 4) * U * sabs
    live = bound > 0
    if bool(live.any()):
        _WORST[key] = max(_WORST.get(key, 0.0), float((err[live] / bound[live]).max()))
    ok = err <= bound
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements outside the bound, worst error {float(err[~ok].max()):.3e}"


def _check(key, kind, got, ref, sabs, n, what):
    if kind == "dyadic":
        _exact(got, ref, what)
    else:
        _within(key, got, ref, sabs, n, what)


def _empty_rows_are_zero(got, n, what):
    rows = got.cpu().reshape(n.numel(), -1)[n == 0]
    assert bool((rows == 0.0).all()), f"{what}: the row of an empty region is not exactly 0.0"


def _absent_is_live(c, n):
    """the "absent" pattern really leaves its two regions without a pixel (so _empty_rows_are_zero has rows to look at)"""
    if c.get("pattern") == "absent":
        first, last = gc.absent_regions(c["R"])
        assert int(n[first]) == 0 and int(n[(c["B"] - 1) * c["R"] + last]) == 0


def _ids(name):
    return [gc.case_id(c) for c in gc.CASES[name]]


def _nsplit(fn, c):
    from e4s_amd import lib
    (h, w), f = c["grid"], getattr(lib.load(), fn)
    return f(c["B"], h, w, c["C"]), f(1, h, w, c["C"])


@pytest.mark.parametrize("index", range(len(gc.ACT_CASES)), ids=_ids("act"))
def test_act_bwd_demod_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in gc.KINDS:
        t = gc.build("act", index, kind)
        c, ref, R, B = t["case"], t["ref"], t["case"]["R"], t["case"]["B"]
        what = f"act_bwd_demod {gc.case_id(c)} {kind}"
        dy, y, noise, bias, labels = (_dev(t[k]) for k in ("dy", "y", "noise", "bias", "labels"))
        nw = torch.tensor([t["noise_w"]], device=DEV)
        hw = c["grid"][0] * c["grid"][1]
        run = lambda sl=slice(None): K.act_bwd_demod(dy[sl], y[sl], noise if noise is None or noise.shape[0] == 1 else noise[sl], nw, bias,   # noqa: E731
                                                     t["alpha"], t["gain"], None if labels is None else labels[sl], R)
        gz, dd = run()
        guard.check()
        _absent_is_live(c, ref["n"])
        _check("act_bwd_demod gz", kind, gz, ref["gz"], ref["gz"].abs(), 0, what + " gz")
        _check("act_bwd_demod dd", kind, dd, ref["dd"], ref["dd_abs"], ref["n"].clamp(max=hw), what + " dd")
        _empty_rows_are_zero(dd, ref["n"], what)
        assert torch.equal(gz, K.fused_bias_act(dy, None, y, 3, 1, t["alpha"], t["gain"])), what + ": gz != fused_bias_act"
        gz2, dd2 = run()
        assert torch.equal(dd, dd2) and torch.equal(gz, gz2), what + ": second call differs"
        if B > 1:
            # gz is elementwise: always batch-invariant.  dd only where the batch-1 launch cuts the pixels into the same number of splits
            # (the order of its additions is a function of nsplit).
            nb, n1 = _nsplit("e4s_act_bwd_demod_nsplit", c)
            for i in range(B):
                gzi, ddi = run(slice(i, i + 1))
                assert torch.equal(gzi[0], gz[i]), what + f": gz of sample {i} depends on the batch"
                if nb == n1:
                    assert torch.equal(ddi, dd[i * R:(i + 1) * R]), what + f": dd of sample {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(gc.DEMOD_CASES)), ids=_ids("demod"))
def test_demod_grad_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in gc.KINDS:
        t = gc.build("demod", index, kind)
        c, ref, R, B = t["case"], t["ref"], t["case"]["R"], t["case"]["B"]
        what = f"demod_grad {gc.case_id(c)} {kind}"
        gz, y, noise, bias, labels = (_dev(t[k]) for k in ("gz", "y", "noise", "bias", "labels"))
        nw = torch.tensor([t["noise_w"]], device=DEV)
        hw = c["grid"][0] * c["grid"][1]
        run = lambda sl=slice(None): K.demod_grad(gz[sl], y[sl], noise if noise is None or noise.shape[0] == 1 else noise[sl], nw, bias,   # noqa: E731
                                                  t["alpha"], t["gain"], None if labels is None else labels[sl], R)
        dd = run()
        guard.check()
        _absent_is_live(c, ref["n"])
        _check("demod_grad dd", kind, dd, ref["dd"], ref["dd_abs"], ref["n"].clamp(max=hw), what)
        _empty_rows_are_zero(dd, ref["n"], what)
        assert torch.equal(dd, run()), what + ": second call differs"
        if B > 1:
            nb, n1 = _nsplit("e4s_seg_reduce_nsplit", c)
            if nb == n1:              # the same splits for both batch sizes: the same additions in the same order
                for i in range(B):
                    assert torch.equal(run(slice(i, i + 1)), dd[i * R:(i + 1) * R]), what + f": dd of sample {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(gc.TORGB_CASES)), ids=_ids("torgb"))
def test_torgb_bwd_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in gc.KINDS:
        t = gc.build("torgb", index, kind)
        c, ref, R, B = t["case"], t["ref"], t["case"]["R"], t["case"]["B"]
        what = f"torgb_bwd {gc.case_id(c)} {kind}"
        drgb, x, ws, labels = (_dev(t[k]) for k in ("drgb", "x", "ws", "labels"))
        hw = c["grid"][0] * c["grid"][1]

        def run(sl=slice(None), gs=slice(None)):
            acc = None if t["acc"] is None else guard.place(t["acc"][sl])          # random values beforehand, SENTINEL around them
            dx, dws = K.torgb_bwd(drgb[sl], x[sl], ws[gs], None if labels is None else labels[sl], R, dx_acc=acc)
            assert acc is None or dx.data_ptr() == acc.data_ptr()
            return dx, dws

        dx, dws = run()
        guard.check()
        _absent_is_live(c, ref["n"])
        _check("torgb_bwd dx", kind, dx, ref["dx"], ref["dx_abs"], 3, what + " dx")
        _check("torgb_bwd dws", kind, dws, ref["dws"], ref["dws_abs"], ref["n"].clamp(max=hw), what + " dws")
        _empty_rows_are_zero(dws, ref["n"], what)
        dx2, dws2 = run()
        assert torch.equal(dws, dws2) and torch.equal(dx, dx2), what + ": second call differs"
        if B > 1:
            nb, n1 = _nsplit("e4s_seg_reduce_nsplit", c)
            for i in range(B):
                dxi, dwsi = run(slice(i, i + 1), slice(i * R, (i + 1) * R))
                assert torch.equal(dxi[0], dx[i]), what + f": dx of sample {i} depends on the batch"
                if nb == n1:          # dws is a sum over splits: batch-invariant only where the splits are the same
                    assert torch.equal(dwsi, dws[i * R:(i + 1) * R]), what + f": dws of sample {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(gc.DGRAD_CASES)), ids=_ids("dgrad"))
def test_region_scale_is_the_fp32_product_in_both_layouts(index, guard):
    from e4s_amd import kernels as K
    for kind in gc.KINDS:
        t = gc.build("dgrad", index, kind)
        c, R, B, ncls = t["case"], t["case"]["R"], t["case"]["B"], t["case"]["ncls"]
        what = f"region_scale {gc.case_id(c)} {kind}"
        gz, d, labels = (_dev(t[k]) for k in ("gz", "d", "labels"))
        want = t["gz"] * gc._pix(t["d"], t["reg"], R)                  # one fp32 product per element
        if ncls == 4:
            want = gc.phase_major(want)                                # (oy, ox) -> [(oy & 1) 2 + (ox & 1), b, oy >> 1, ox >> 1]
        u = K.region_scale(gz, d, labels, R, ncls)
        guard.check()
        assert u.shape == want.shape and torch.equal(u.cpu(), want), what + ": not the fp32 product"
        if kind == "dyadic":
            _exact(u, gc.phase_major(t["ref"]["u"]) if ncls == 4 else t["ref"]["u"], what)
        for i in range(B if B > 1 else 0):
            ui = K.region_scale(gz[i:i + 1], d[i * R:(i + 1) * R], labels[i:i + 1], R, ncls)
            assert torch.equal(ui[:, 0] if ncls == 4 else ui[0], u[:, i] if ncls == 4 else u[i]), what + f": sample {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(gc.DGRAD_CASES)), ids=_ids("dgrad"))
def test_col2im_region_vs_f64_autograd(index, guard):
    """dx and ds from scatter products G computed in fp64 on the host and rounded to fp32 once: the two streaming passes alone, without
    the matrix-core contraction."""
    from e4s_amd import kernels as K
    for kind in gc.KINDS:
        t = gc.build("dgrad", index, kind)
        c, ref, R, B, ncls = t["case"], t["ref"], t["case"]["R"], t["case"]["B"], t["case"]["ncls"]
        what = f"col2im_region {gc.case_id(c)} {kind}"
        G, x, s, labels = (_dev(t[k]) for k in ("G", "x", "s", "labels"))
        hw = c["grid"][0] * c["grid"][1]
        n_rows = ref["n_ds"] // 9
        dx, ds = K.col2im_region(G, x, s, labels, R, ncls)
        guard.check()
        _absent_is_live(c, n_rows)
        _check("col2im_region dx", kind, dx, ref["dx"], ref["dx_abs"], ref["n_dx"], what + " dx")
        _check("col2im_region ds", kind, ds, ref["ds"], ref["ds_abs"], ref["n_ds"].clamp(max=hw), what + " ds")
        _empty_rows_are_zero(ds, n_rows, what)
        dx2, ds2 = K.col2im_region(G, x, s, labels, R, ncls)
        assert torch.equal(ds, ds2) and torch.equal(dx, dx2), what + ": second call differs"
        if B > 1:
            nb, n1 = _nsplit("e4s_col2im_region_nsplit", c)
            for i in range(B):
                dxi, dsi = K.col2im_region(G[:, i:i + 1].contiguous(), x[i:i + 1], s[i * R:(i + 1) * R], labels[i:i + 1], R, ncls)
                assert torch.equal(dxi[0], dx[i]), what + f": dx of sample {i} depends on the batch"
                if nb == n1:          # ds is a sum over splits: batch-invariant only where the splits are the same
                    assert torch.equal(dsi, ds[i * R:(i + 1) * R]), what + f": ds of sample {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("index", range(len(gc.SCALE_DOT_CASES)), ids=_ids("scale_dot"))
def test_scale_dot_vs_f64(index, guard):
    from e4s_amd import kernels as K
    for kind in gc.KINDS:
        t = gc.build("scale_dot", index, kind)
        c, ref, B = t["case"], t["ref"], t["case"]["B"]
        what = f"scale_dot {gc.case_id(c)} {kind}"
        x, s = _dev(t["x"]), _dev(t["s"])
        hw = c["grid"][0] * c["grid"][1]
        u = guard.place(t["u"])                                        # updated in place: SENTINEL around it
        out, ds = K.scale_dot(u, x, s)
        guard.check()
        assert out.data_ptr() == u.data_ptr()
        assert torch.equal(u.cpu(), t["u"] * t["s"].reshape(B, 1, 1, -1)), what + ": u is not the fp32 product u * s[b]"
        _check("scale_dot ds", kind, ds, ref["ds"], ref["ds_abs"], hw, what + " ds")
        if kind == "dyadic":
            _exact(u, ref["u"], what + " u")
        assert torch.equal(ds, K.scale_dot(guard.place(t["u"]), x, s)[1]), what + ": second call differs"
        for i in range(B if B > 1 else 0):
            ui, _ = K.scale_dot(guard.place(t["u"][i:i + 1]), x[i:i + 1], s[i:i + 1])
            assert torch.equal(ui[0], u[i]), what + f": u of sample {i} depends on the batch"
        guard.check()


def test_channel_counts_outside_the_sets_are_refused_before_any_launch():
    from e4s_amd import kernels as K
    z = torch.zeros(1, 4, 4, 12, device=DEV)
    labels = torch.zeros(1, 4, 4, dtype=torch.uint8, device=DEV)
    nw = torch.zeros(1, device=DEV)
    assert K.act_bwd_demod(z, z, None, nw, None, 0.2, 1.0, labels, 2) is None
    z192 = torch.zeros(1, 4, 4, 192, device=DEV)
    assert K.act_bwd_demod(z192, z192, None, nw, None, 0.2, 1.0, labels, 2) is None
    assert not K.col2im_region_ok(12)
    with pytest.raises(RuntimeError, match="unsupported channel count"):
        K.col2im_region(torch.zeros(1, 1, 4, 4, 9 * 12, device=DEV), z, torch.zeros(2, 12, device=DEV), labels, 2, 1)
