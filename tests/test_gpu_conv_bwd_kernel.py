"""The exact-fp32 dgrad kernel (conv_bwd_kernel of csrc/conv_bwd.hip through e4s_conv_bwd_mfma_f32 and K.conv_bwd) on its own against
the fp64 autograd yardstick of tests/conv_bwd_cases.py (checked on the CPU by tests/test_conv_bwd_cases_host.py), and three small
kernels next to it: e4s_reduce_parts_f32, K.pack_taps_bwd and K.shift_scale.

Per case of conv_bwd: e4s_conv_bwd_ws_floats answers exactly the size that the restated split rule gives (which confirms the restated
gsplit without reading internal state); with dyadic data dx and ds EQUAL the reference (no tolerance: a dropped, doubled or mis-filed
term fails); with random data |got - ref| <= (N + 3) 2^-24 S_abs elementwise, N = min(9 ncls Cy, Cy + 9 ncls) for dx and
min(9 Cy pixels(region), Cy + 128 + 9 ncls + parts) for ds, S_abs the fp64 sum of the absolute values of the terms -- the bound of a
nested fp32 sum (channels, then tile rows, tap groups and parts), each level in any order, plus the three roundings inside a term (gz d,
the product with W, s T or x T), derived in the case module's docstring and not measured.  ds rows of regions absent from a sample are exactly 0.0, a second call reproduces dx and ds bit for
bit, sample i of a batch-3 call equals the batch-1 call on that sample where both batch sizes split alike, no element of dx, ds or the
used part of the workspace is left unwritten, the floats on either side of every tensor the wrapper allocates keep their sentinel, and
want_ds=False gives the same dx bits.  Every refusal of the entry point is checked by return value, before any launch."""
import ctypes

import pytest
import torch

import conv_bwd_cases as cc
from guarded_alloc import _GuardedTorch, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
INVALID = 1                 # hipErrorInvalidValue
_IDS = [cc.case_id(c) for c in cc.CASES]
_WORST = {}                 # output -> largest observed error / bound on random data


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
        print(f"\n[conv-bwd] largest error / bound of {k}: {_WORST[k]:.3f}", end="")
    print()


def _dev(t):
    return None if t is None else t.to(DEV)


def _check(key, kind, got, ref, sabs, n, c, what):
    if kind == "dyadic":
        assert torch.equal(got.cpu(), ref.float()), f"{what}: not equal to the fp64 reference on dyadic data"
        return
    err, bound = (got.cpu().double() - ref).abs(), cc.bound(sabs, n, c)
    live = bound > 0
    if bool(live.any()):
        _WORST[key] = max(_WORST.get(key, 0.0), float((err[live] / bound[live]).max()))
    ok = err <= bound
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements outside the bound, worst error {float(err[~ok].max()):.3e}"


def _params(c, B, want_ds):
    """what e4s_conv_bwd_ws_floats looks at: the shape fields and whether ds, s and labels are set"""
    from e4s_amd.lib import ConvBwdParams
    (H, W), os_ = c["grid"], 2 if c["ncls"] == 4 else 1
    p = ConvBwdParams()
    p.B, p.Hx, p.Wx, p.Cx, p.Hy, p.Wy, p.Cy, p.ncls = B, H, W, c["Cx"], H * os_, W * os_, c["Cy"], c["ncls"]
    p.R = c["R"] if c["pattern"] is not None else 1
    one = ctypes.c_void_p(16)                      # only compared with null, never read
    p.ds = one if want_ds else None
    p.labels = one if c["pattern"] is not None else None
    return p


def _run(K, guard, t, sl=slice(None), want_ds=True):
    """one guarded K.conv_bwd on samples `sl`; -> (dx, ds, workspace or None)"""
    c, R = t["case"], t["R"]
    B = c["B"]
    idx = list(range(B))[sl]
    rows = slice(idx[0] * R, (idx[-1] + 1) * R)
    cut = lambda v: None if v is None else v[sl]                                              # noqa: E731
    tab = lambda v: None if v is None else v[rows]                                            # noqa: E731
    dx, ds = K.conv_bwd(cut(t["gz_d"]), t["wt_d"], cut(t["x_d"]), tab(t["s_d"]), tab(t["d_d"]), cut(t["labels_d"]), R, c["ncls"],
                        want_ds=want_ds)
    made = guard.insides(torch.float32)
    produces = want_ds and t["s"] is not None
    ws = made[1 + int(produces)] if len(made) > 1 + int(produces) else None
    what = f"conv_bwd {cc.case_id(c)} B{len(idx)}"
    torch.cuda.synchronize()
    assert unwritten(dx) == 0, what + ": elements of dx left unwritten"
    assert (ds is None) == (not produces)
    if produces:
        assert unwritten(ds) == 0, what + ": elements of ds left unwritten"
    want = cc.ws_floats(c, produces, len(idx))
    assert (0 if ws is None else ws.numel()) == want
    for a, b in cc.ws_used(c, produces, len(idx)):
        assert unwritten(ws[a:b]) == 0, what + f": workspace floats [{a}, {b}) not all written"
    guard.check()
    return dx, ds


@pytest.mark.parametrize("index", range(len(cc.CASES)), ids=_IDS)
def test_conv_bwd_vs_f64_autograd(index, guard):
    from e4s_amd import kernels as K
    from e4s_amd import lib
    L = lib.load()
    c = cc.CASES[index]
    for B in {1, c["B"]}:
        for want_ds in (True, False):
            assert L.e4s_conv_bwd_ws_floats(ctypes.byref(_params(c, B, want_ds))) == cc.ws_floats(c, want_ds, B), (B, want_ds)
    for kind in cc.KINDS:
        t = dict(cc.build(index, kind))
        what = f"conv_bwd {cc.case_id(c)} {kind}"
        R, B = t["R"], c["B"]
        for k in ("gz", "x", "s", "d", "labels"):
            t[k + "_d"] = _dev(t[k])
        t["wt_d"] = _dev(t["wt"])
        dx, ds = _run(K, guard, t)
        _check("dx", kind, dx, t["dx"], t["dx_abs"], t["n_dx"], cc.C_DX, what + " dx")
        if ds is not None:
            _check("ds", kind, ds, t["ds"], t["ds_abs"], t["n_ds"], cc.C_DS, what + " ds")
            empty = ds.cpu()[t["count"] == 0]
            assert bool((empty == 0.0).all()), what + ": the ds row of an absent region is not exactly 0.0"
            if c["pattern"] == "absent":
                assert empty.shape[0] >= 2
        dx2, ds2 = _run(K, guard, t)
        assert torch.equal(dx, dx2) and (ds is None or torch.equal(ds, ds2)), what + ": second call differs"
        if ds is not None:
            dx3, none = _run(K, guard, t, want_ds=False)
            assert none is None and torch.equal(dx, dx3), what + ": dx depends on want_ds"
        if B == 3 and cc.geometry(c, 1)["gsplit"] == cc.geometry(c, 3)["gsplit"]:
            for i in range(B):
                dxi, dsi = _run(K, guard, t, slice(i, i + 1))
                assert torch.equal(dxi[0], dx[i]), what + f": dx of sample {i} depends on the batch"
                assert ds is None or torch.equal(dsi, ds[i * R:(i + 1) * R]), what + f": ds of sample {i} depends on the batch"


def test_conv_bwd_refusals_by_return_value_before_any_launch(guard):
    """Every refused input returns hipErrorInvalidValue and leaves dx, ds and the workspace as they were (NaN): nothing was launched."""
    from e4s_amd import lib
    from e4s_amd.lib import ConvBwdParams, fptr, ptr, stream
    L = lib.load()
    B, H, W, Cx, Cy, R = 1, 8, 16, 64, 32, 3
    z = lambda *shape: torch.zeros(*shape, device=DEV)                                        # noqa: E731
    # buffers large enough for every variant below (Cx, Cy up to 64; the polyphase output grid)
    gz, wt, x, s, d = z(B, 2 * H, 2 * W, 64), z(4, 9, 64, 64), z(B, H, W, 64), z(B * 17, 64), z(B * 17, 64)
    labels = torch.zeros(B, 5, 7, dtype=torch.uint8, device=DEV)

    def attempt(masked=True, null_ws=False, null_x=False, with_ds=True, **over):
        dx, ds, ws = guard.empty(B, H, W, 64, device=DEV), guard.empty(B * 17, 64, device=DEV), guard.empty(1 << 20, device=DEV)
        p = ConvBwdParams()
        p.gz, p.wt, p.dx, p.s, p.d = fptr(gz), fptr(wt), fptr(dx), fptr(s), fptr(d)
        p.x, p.ds, p.ds_ws = None if null_x else fptr(x), fptr(ds) if with_ds else None, None if null_ws else fptr(ws)
        p.labels, p.Hm, p.Wm, p.R = (ptr(labels), 5, 7, R) if masked else (None, 0, 0, 1)
        p.B, p.Hx, p.Wx, p.Cx, p.Hy, p.Wy, p.Cy, p.ncls = B, H, W, Cx, H, W, Cy, 1
        for k, v in over.items():
            setattr(p, k, v)
        rc = L.e4s_conv_bwd_mfma_f32(ctypes.byref(p), stream())
        torch.cuda.synchronize()
        for buf in (dx, ds, ws):
            assert unwritten(buf) == buf.numel(), f"{over}: something was written although the call was refused"
        guard.check()
        return rc

    assert attempt(Cx=48) == INVALID
    assert attempt(Cy=48) == INVALID
    assert attempt(ncls=2) == INVALID
    assert attempt(ncls=2, Hy=2 * H, Wy=2 * W) == INVALID
    assert attempt(R=0) == INVALID
    assert attempt(R=17) == INVALID
    assert attempt(Hy=H + 1) == INVALID
    assert attempt(Wy=W - 1) == INVALID
    assert attempt(ncls=4) == INVALID                                    # Hy, Wy not doubled
    assert attempt(ncls=4, Hy=2 * H, Wy=W) == INVALID
    assert attempt(null_x=True) == INVALID                               # ds without x
    assert attempt(null_ws=True) == INVALID                              # ds needs its parts
    assert attempt(null_ws=True, with_ds=False, masked=False) == INVALID   # one tile: gsplit = 9 needs the dx parts


def test_reduce_parts_is_the_in_order_fp32_sum(guard):
    from e4s_amd import lib
    from e4s_amd.lib import c_p, stream
    L = lib.load()

    def run(parts, scale, offset=0):
        nparts, n = parts.shape
        ws = guard.empty(L.e4s_reduce_parts_ws_floats(nparts, n), device=DEV)
        assert ws.numel() == cc.reduce_ws_floats(nparts, n)
        ws[:nparts * n] = parts.reshape(-1).to(DEV)
        buf = guard.empty(n + 4, device=DEV)
        out = buf[offset:offset + n]
        assert L.e4s_reduce_parts_f32(c_p(ws.data_ptr()), c_p(out.data_ptr()), nparts, n, scale, stream()) == 0
        torch.cuda.synchronize()
        assert unwritten(buf) == 4, "reduce_parts wrote next to its output or left an element unwritten"
        assert torch.equal(ws[:nparts * n].cpu(), parts.reshape(-1)), "reduce_parts changed its parts"
        lvl = ws[nparts * n:]
        assert unwritten(lvl) == (0 if nparts > cc.RCHUNK else lvl.numel())
        guard.check()
        return out.cpu()

    for nparts in cc.REDUCE_NPARTS:
        for n in cc.REDUCE_N:
            for scale in cc.REDUCE_SCALES:
                what = f"reduce_parts nparts {nparts} n {n} scale {scale}"
                parts = cc.reduce_parts_data(nparts, n, "random")
                want = torch.from_numpy(cc.reduce_parts_ref(parts.numpy(), scale))
                assert torch.equal(run(parts, scale), want), what + ": not the in-order fp32 sum"
                dy = cc.reduce_parts_data(nparts, n, "dyadic")
                assert torch.equal(run(dy, scale).double(), dy.double().sum(0) * scale), what + ": dyadic parts do not give the fp64 sum"
    # out one float off a 16-byte boundary: the vector path is declined, the result is the same
    for nparts in (9, 130):
        parts = cc.reduce_parts_data(nparts, 1000, "random")
        want = torch.from_numpy(cc.reduce_parts_ref(parts.numpy(), 0.5))
        assert torch.equal(run(parts, 0.5, offset=1), want)
    # more than 16384 parts would need a third level: refused by return value, nothing written
    ws, out = guard.empty(64, device=DEV), guard.empty(4, device=DEV)
    assert L.e4s_reduce_parts_f32(c_p(ws.data_ptr()), c_p(out.data_ptr()), 16385, 4, 1.0, stream()) == INVALID
    torch.cuda.synchronize()
    assert unwritten(ws) == 64 and unwritten(out) == 4
    guard.check()


@pytest.mark.parametrize("shape", cc.PACK_SHAPES, ids=lambda s: "ncls%d-Cout%d-Cin%d" % s)
def test_pack_taps_bwd_is_the_flipped_transposed_forward_pack(shape, guard):
    from e4s_amd import kernels as K
    ncls, cout, cin = shape
    W = cc.operand((ncls, 9, cout, cin), "random", torch.Generator().manual_seed(cout * 100 + cin))
    wt = K.pack_taps_bwd(W.to(DEV))
    guard.check()
    assert wt.shape == (ncls, 9, cin, cout) and torch.equal(wt.cpu(), cc.pack_bwd_ref(W))
    into = guard.empty(ncls, 9, cin, cout, device=DEV)
    assert K.pack_taps_bwd(W.to(DEV), out=into).data_ptr() == into.data_ptr() and torch.equal(into.cpu(), cc.pack_bwd_ref(W))
    guard.check()


def test_shift_scale_is_one_fp32_product_and_zero_outside(guard):
    from e4s_amd import kernels as K
    from e4s_amd import lib
    from e4s_amd.lib import fptr, stream
    g = torch.Generator().manual_seed(17)
    B, _, _, C = cc.SHIFT_X
    x = cc.operand(cc.SHIFT_X, "random", g)
    tab_r, tab_b = cc.operand((B * cc.SHIFT_R, C), "random", g), cc.operand((B, C), "random", g)
    labels = cc.make_labels("noise", B, *cc.SHIFT_MAP, cc.SHIFT_R, seed=4)
    for c in cc.SHIFT_CASES:
        lab, tab = (labels, tab_r) if c["labels"] else (None, tab_b)
        got = K.shift_scale(x.to(DEV), tab.to(DEV), _dev(lab), cc.SHIFT_R, c["anchors"], c["istride"], c["dy"], c["dx"], c["os"], c["py"],
                            c["px"])
        guard.check()
        want = cc.shift_scale_ref(x, tab, lab, cc.SHIFT_R, c["anchors"], c["istride"], c["dy"], c["dx"], c["os"], c["py"], c["px"])
        assert torch.equal(got.cpu(), want), f"shift_scale {c}"
        if c["dy"] or c["dx"]:
            assert bool((want == 0).all(-1).any()), f"shift_scale {c}: the case has no anchor outside the image"
    # C % 4 != 0 is refused before any launch
    x6, t6, out = torch.zeros(1, 4, 4, 6, device=DEV), torch.zeros(1, 6, device=DEV), guard.empty(1, 4, 4, 6, device=DEV)
    rc = lib.load().e4s_shift_scale_f32(fptr(x6), fptr(t6), None, 0, 0, 1, fptr(out), 1, 4, 4, 4, 4, 6, 1, 0, 0, 1, 0, 0, stream())
    torch.cuda.synchronize()
    assert rc == INVALID and unwritten(out) == out.numel()
    guard.check()
    with pytest.raises(RuntimeError, match="e4s_shift_scale_f32"):
        K.shift_scale(x6, t6, None, 1, (4, 4))
