"""The small kernels around the convs of the Discriminator, GPEN and the generator forward (csrc/ops.hip, csrc/gpen.hip, the tail of
csrc/torgb.hip, the single-launch rowdot and weight_sqsum of csrc/style.hip, colsum of csrc/optim.hip, the row plan of csrc/plan.hip), each
on its own against the fp64 yardsticks of tests/glue_cases.py (checked on the CPU by tests/test_glue_cases_host.py; the bounds are
derived in that module's docstring).

Per case, on dyadic data the output EQUALS the reference wherever the chain holds no root, quotient or non-dyadic scale, otherwise
|got - ref| <= the derived bound elementwise.  A second call reproduces every summed output bit for bit; sample i of a batch equals the
batch-1 call where the kernel has a batch; no element of an output is left unwritten (the `out=` forms start as a sentinel, and the
channels a kernel does not own keep it), and the elements on either side of every tensor a wrapper allocates keep their sentinel.  Geometry
the ABI does not take is refused by its return value before any launch.  The region plan is checked structurally (glue_cases.check_plan)."""
import itertools
import math

import pytest
import torch

import glue_cases as gl
from guarded_alloc import DEV, _GuardedTorch, unwritten

pytestmark = pytest.mark.gpu
U = gl.U
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
        print(f"\n[glue] largest error / bound of {k}: {_WORST[k]:.3f}", end="")
    print()


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(key, exact, got, ref, bound, what):
    """exact: got EQUALS the fp64 reference; else |got - ref| <= bound elementwise (0 where the bound is 0)."""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)}, reference {tuple(ref.shape)}"
    assert unwritten(got) == 0, f"{what}: {unwritten(got)} elements were never written"
    if exact:
        assert torch.equal(got.cpu(), ref.float()), f"{what}: not equal to the fp64 reference"
        return
    err = (got.cpu().double() - ref).abs()
    live = bound > 0
    if bool(live.any()):
        _WORST[key] = max(_WORST.get(key, 0.0), float((err[live] / bound[live]).max()))
    ok = err <= bound
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements outside the bound, worst error {float(err[~ok].max()):.3e}"


# ---- fused_bias_act, channel_sum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(gl.FBA_CASES)), ids=[c["tag"] for c in gl.FBA_CASES])
def test_fused_bias_act_vs_f64(index, guard):
    from e4s_amd import kernels as K
    c = gl.FBA_CASES[index]
    off = c["offset"]

    def view(t):          # a contiguous view that starts `off` floats into its allocation
        buf = torch.empty(t.numel() + off, device=DEV)
        v = buf[off:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
        return v

    for kind in gl.KINDS:
        t = gl.fba_case(index, kind)
        x, xb, ref, bias = view(t["x"]), view(t["xb"]), view(t["ref"]), _dev(t["bias"])
        for (act, grad, has_b), (want, bound) in t["refs"].items():
            what = f"fused_bias_act {c['tag']} code {act}{grad} bias{int(has_b)} {kind}"
            y = K.fused_bias_act(xb if has_b else x, bias if has_b else None, ref if (act, grad) == (3, 1) else None, act, grad, t["alpha"], t["scale"])
            guard.check()
            _check("fused_bias_act", t["exact"], y, want, bound, what)


@pytest.mark.parametrize("step_b", gl.CSUM_STEPS)
def test_channel_sum_vs_f64(step_b, guard):
    from e4s_amd import kernels as K
    for outer, C, kind in itertools.product(gl.CSUM_OUTER, gl.CSUM_C, gl.KINDS):
        t = gl.csum_case(step_b, outer, C, kind)
        x = _dev(t["x"])
        s = K.channel_sum(x)
        guard.check()
        what = f"channel_sum step{step_b} outer{outer} C{C} {kind}"
        _check("channel_sum", t["exact"], s, t["ref"], t["bound"], what)
        assert _same_bits(s, K.channel_sum(x)), what + ": second call differs"
        guard.check()


# ---- upfirdn2d -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(gl.UFD_CASES)), ids=[c["tag"] for c in gl.UFD_CASES])
def test_upfirdn2d_vs_f64(index, guard):
    from e4s_amd import kernels as K
    c = gl.UFD_CASES[index]
    path = gl.upfirdn_path(c)
    assert path == gl.UFD_EXPECT[index] and c["tag"].startswith(path), "the case moved to another kernel"
    (ux, uy), (dx, dy) = c["up"], c["down"]
    for kind in gl.KINDS:
        t = gl.ufd_case(index, kind)
        what = f"upfirdn2d {c['tag']} {kind}"
        x, k = _dev(t["x"]), _dev(t["k"])
        y = K.upfirdn2d_raw(x, k, ux, uy, dx, dy, *c["pad"])
        guard.check()
        _check("upfirdn2d " + path, t["exact"], y, t["ref"], t["bound"], what)
        none = t["taps"] == 0
        if bool(none.any()):
            assert float(y.cpu()[none].abs().max()) == 0, what + ": an output that meets no sample is not 0.0"
        assert _same_bits(y, K.upfirdn2d_raw(x, k, ux, uy, dx, dy, *c["pad"])), what + ": second call differs"
        for i in range(c["major"] if c["major"] > 1 else 0):
            assert _same_bits(K.upfirdn2d_raw(x[i:i + 1], k, ux, uy, dx, dy, *c["pad"])[0], y[i]), what + f": plane {i} depends on the batch"
        guard.check()


# ---- conv1x1_small, noise_half ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", gl.C1_CIN)
def test_conv1x1_small_vs_f64(cin, guard):
    from e4s_amd import kernels as K
    for cout, hw, kind in itertools.product(gl.C1_COUT, gl.C1_HW, gl.KINDS):
        t = gl.c1_case(cin, cout, hw, kind)
        x, w, bias = _dev(t["x"]), _dev(t["w"]), _dev(t["bias"])
        for (has_b, act), (ref, bound) in t["refs"].items():
            what = f"conv1x1_small Cin{cin} Cout{cout} {hw[0]}x{hw[1]} bias{int(has_b)} act{act} {kind}"
            args = (w, bias if has_b else None, t["scale"])
            kw = dict(act=act, alpha=t["alpha"], gain=t["gain"])
            y = K.conv1x1_small(x, *args, **kw)
            guard.check()
            _check("conv1x1_small", t["exact"], y, ref, bound, what)
            assert _same_bits(y, K.conv1x1_small(x, *args, **kw)), what + ": second call differs"
            for i in range(gl.C1_B):
                assert _same_bits(K.conv1x1_small(x[i:i + 1], *args, **kw)[0], y[i]), what + f": sample {i} depends on the batch"
            guard.check()
        # the out= form with a channel stride above Cout: the other channels keep their bits
        ref, bound = t["refs"][(True, 1)]
        wide = guard.empty(gl.C1_B, hw[0], hw[1], cout + 8, device=DEV)
        K.conv1x1_small(x, w, bias, t["scale"], act=1, alpha=t["alpha"], gain=t["gain"], out=wide)
        guard.check()
        _check("conv1x1_small", t["exact"], wide[..., :cout], ref, bound, what + " out=")
        assert unwritten(wide[..., cout:]) == wide[..., cout:].numel(), what + ": a channel the kernel does not own was written"


@pytest.mark.parametrize("C", gl.NH_C)
def test_noise_half_vs_f64(C, guard):
    from e4s_amd import kernels as K
    for kind, (cy, coff) in itertools.product(gl.KINDS, gl.nh_layouts(C)):
        t = gl.nh_case(C, kind)
        what = f"noise_half C{C} Cy{cy} coff{coff} {kind}"
        out = guard.empty(*gl.NH_SHAPE, cy, device=DEV)
        got = K.noise_half(_dev(t["feat"]), torch.tensor([t["nw"]], device=DEV), _dev(t["bias"]), out, coff, alpha=t["alpha"], gain=t["gain"])
        guard.check()
        _check("noise_half", t["exact"], got[..., coff:coff + C], t["ref"], t["bound"], what)
        rest = torch.cat([got[..., :coff], got[..., coff + C:]], -1)
        assert unwritten(rest) == rest.numel(), what + ": a channel the kernel does not own was written"


# ---- pixelnorm, add_scale, minibatch_stddev, const_input -------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", gl.PN_D)
def test_pixelnorm_vs_f64(D, guard):
    from e4s_amd import kernels as K
    for B, kind in itertools.product(gl.PN_B, gl.KINDS):
        t = gl.pn_case(B, D, kind)
        what = f"pixelnorm B{B} D{D} {kind}"
        x = _dev(t["x"])
        y = K.pixelnorm(x)
        guard.check()
        _check("pixelnorm", False, y, t["ref"], t["bound"], what)
        if t["zero_row"] is not None:
            assert float(y[t["zero_row"]].abs().max()) == 0, what + ": an all-zero row is not 0.0"
        assert _same_bits(y, K.pixelnorm(x)), what + ": second call differs"
        for i in range(B if B > 1 else 0):
            assert _same_bits(K.pixelnorm(x[i:i + 1])[0], y[i]), what + f": row {i} depends on the batch"
        guard.check()


@pytest.mark.parametrize("n", gl.AS_N)
def test_add_scale_vs_f64(n, guard):
    from e4s_amd import kernels as K
    for kind in gl.KINDS:
        t = gl.as_case(n, kind)
        a, b = _dev(t["a"]), _dev(t["b"])
        y1 = K.add_scale(a, b, 1.0)
        guard.check()
        assert unwritten(y1) == 0 and _same_bits(y1.cpu(), t["a"] + t["b"]), f"add_scale n{n} {kind}: scale 1 is not the fp32 sum bit for bit"
        _check("add_scale", True, y1, t["ref1"], None, f"add_scale n{n} scale 1 {kind}")
        y = K.add_scale(a, b, gl.AS_SCALE)
        guard.check()
        _check("add_scale", False, y, t["ref"], t["bound"], f"add_scale n{n} {kind}")


@pytest.mark.parametrize("B, group", gl.MS_GROUPS, ids=[f"B{b}-group{g}" for b, g in gl.MS_GROUPS])
def test_minibatch_stddev_vs_f64(B, group, guard):
    from e4s_amd import kernels as K
    for hw, C, kind, identical in itertools.product(gl.MS_HW, gl.MS_C, gl.KINDS, (False, True)):
        t = gl.ms_case(B, group, hw, C, kind, identical)
        x = _dev(t["x"])
        for cy in gl.ms_widths(C):
            what = f"minibatch_stddev B{B} group{group} {hw[0]}x{hw[1]} C{C} Cy{cy} {kind}{' identical' if identical else ''}"
            y = K.minibatch_stddev(x, cy, group)
            guard.check()
            assert unwritten(y) == 0, what + ": an element was never written"
            assert _same_bits(y[..., :C], x), what + ": channels [0, C) are not x bit for bit"
            assert float(y[..., C + 1:].abs().max() if cy > C + 1 else 0) == 0, what + ": a channel above C is not 0.0"
            stat = y[..., C].cpu()
            assert bool((stat == stat[:, :1, :1]).all()), what + ": the statistic varies over the pixels of a sample"
            if identical and gl.ms_identical_exact(group, kind):
                assert bool((stat == gl.ROOT_EPS8).all()), what + ": identical members do not give sqrtf(1e-8f)"
            _check("minibatch_stddev", False, stat[:, 0, 0], t["stat"], t["bound"], what)
            assert _same_bits(y, K.minibatch_stddev(x, cy, group)), what + ": second call differs"
            guard.check()


@pytest.mark.parametrize("C", gl.CI_C)
def test_const_input_is_the_expanded_permutation(C, guard):
    from e4s_amd import kernels as K
    for B, (h, w) in itertools.product(gl.CI_B, gl.CI_GRIDS):
        inp = gl.operand((1, C, h, w), "random", gl._gen("ci", f"{C}-{h}-{w}", "random"))
        y = K.const_input(_dev(inp), B)
        guard.check()
        assert unwritten(y) == 0 and torch.equal(y.cpu(), inp.permute(0, 2, 3, 1).expand(B, h, w, C)), f"const_input B{B} C{C} {h}x{w}"


# ---- mask_mul_add, noise_bias_act_nhwc -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", gl.MM_GRIDS, ids=[f"{g[0]}x{g[1]}" for g in gl.MM_GRIDS])
def test_mask_mul_add_vs_f64(grid, guard):
    from e4s_amd import kernels as K
    for rel, cl, kind in itertools.product(("larger", "equal", "smaller"), (True, False), gl.KINDS):
        t = gl.mm_case(grid, rel, cl, kind)
        y, mask = _dev(t["y"]), _dev(t["mask"])
        for r, (v, vb, acc, accb) in t["refs"].items():
            what = f"mask_mul_add {grid[0]}x{grid[1]} mask {rel} {'nhwc' if cl else 'nchw'} r{r} {kind}"
            out = K.mask_mul_add(y, mask, r, None, cl)
            guard.check()
            _check("mask_mul_add", t["exact"], out, v, vb, what)
            got = K.mask_mul_add(y, mask, r, guard.place(t["acc"]), cl)
            guard.check()
            _check("mask_mul_add (accumulate)", t["exact"], got, acc, accb, what + " accumulate")
            for i in range(gl.MM_B):
                assert _same_bits(K.mask_mul_add(y[i:i + 1], mask[i:i + 1], r, None, cl)[0], out[i]), what + f": sample {i} depends on the batch"
            guard.check()


@pytest.mark.parametrize("C", gl.NB_C)
def test_noise_bias_act_nhwc_vs_f64(C, guard):
    from e4s_amd import kernels as K
    for kind in gl.KINDS:
        t = gl.nb_case(C, kind)
        x, bias, nw = _dev(t["x"]), _dev(t["bias"]), torch.tensor([t["nw"]], device=DEV)
        for mode, (ref, bound) in t["refs"].items():
            what = f"noise_bias_act_nhwc C{C} noise {mode} {kind}"
            noise = None if mode == "none" else _dev(t["noise"][:1] if mode == "shared" else t["noise"])
            y = K.noise_bias_act_nhwc(x, noise, nw, bias, t["alpha"], t["gain"])
            guard.check()
            _check("noise_bias_act_nhwc", t["exact"], y, ref, bound, what)
            for i in range(gl.NB_SHAPE[0]):
                ni = None if noise is None else (noise if mode == "shared" else noise[i:i + 1])
                assert _same_bits(K.noise_bias_act_nhwc(x[i:i + 1], ni, nw, bias, t["alpha"], t["gain"])[0], y[i]), what + f": sample {i}"
            guard.check()


# ---- rowdot (single launch), weight_sqsum ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kdim", gl.RD_K)
def test_rowdot_single_launch_vs_f64(Kdim, guard):
    from e4s_amd import kernels as K
    for G, O, kind in itertools.product(gl.RD_G, gl.RD_O, gl.KINDS):
        t = gl.rd_case(G, O, Kdim, kind)
        what = f"rowdot G{G} O{O} K{Kdim} {kind}"
        style, M, bias, wsq = _dev(t["style"]), _dev(t["M"]), _dev(t["bias"]), _dev(t["wsq"])
        s = K.modulate_vec(style, M, bias)
        guard.check()
        _check("rowdot mode 0", t["exact0"], s, *t["mode0"], what + " modulate_vec")
        d = K.demod_coefs(style, wsq, t["conv_scale"])
        guard.check()
        _check("rowdot mode 1", False, d, *t["mode1"], what + " demod_coefs")
        assert _same_bits(s, K.modulate_vec(style, M, bias)) and _same_bits(d, K.demod_coefs(style, wsq, t["conv_scale"])), what + ": second call differs"
        for i in range(G if G > 1 else 0):
            assert _same_bits(K.modulate_vec(style[i:i + 1], M, bias)[0], s[i]), what + f": row {i} depends on the batch"
            assert _same_bits(K.demod_coefs(style[i:i + 1], wsq, t["conv_scale"])[0], d[i]), what + f": row {i} depends on the batch"
        guard.check()
    if Kdim in (256, 260):          # the strided latent input of `modulate`
        for O, kind in itertools.product((3, 5), gl.KINDS):
            t = gl.rd_latent_case(Kdim, O, kind)
            latent, M, bias = _dev(t["latent"]), _dev(t["M"]), _dev(t["bias"])
            for (layer, masked), (ref, bound) in t["refs"].items():
                s = K.modulate(latent, layer, masked, M, bias)
                guard.check()
                _check("rowdot mode 0", t["exact0"], s, ref, bound, f"modulate K{Kdim} O{O} layer {layer} masked{int(masked)} {kind}")


@pytest.mark.parametrize("shape", gl.WS_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in gl.WS_SHAPES])
def test_weight_sqsum_vs_f64(shape, guard):
    from e4s_amd import kernels as K
    for taps, kind in itertools.product(gl.WS_TAPS, gl.KINDS):
        t = gl.ws_case(shape, taps, kind)
        what = f"weight_sqsum {shape} taps{taps} {kind}"
        w = _dev(t["w"])
        s = K.weight_sqsum(w)
        guard.check()
        _check("weight_sqsum", t["exact"], s, t["ref"], t["bound"], what)
        out = guard.empty(*shape, device=DEV)
        assert K.weight_sqsum(w, out=out) is out
        guard.check()
        assert unwritten(out) == 0 and _same_bits(out, s), what + ": the out= form differs"


# ---- colsum ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(gl.COLSUM_CASES)), ids=[f"{c['tag']}-rows{c['rows']}-C{c['C']}" for c in gl.COLSUM_CASES])
def test_colsum_vs_f64(index, guard):
    from e4s_amd import kernels as K, lib
    c = gl.COLSUM_CASES[index]
    path, rpb, parts, levels = gl.colsum_levels(c["rows"], c["C"])
    for kind in gl.KINDS:
        t = gl.colsum_case(index, kind)
        what = f"colsum {c['tag']} rows{c['rows']} C{c['C']} {kind}"
        x = _dev(t["x"])
        s = K.colsum(x)
        if path == "colsum":
            ws = guard.insides(torch.float32)[-1]
            assert ws.numel() == lib.load().e4s_colsum_ws_floats(c["rows"], c["C"]) == (parts + -(-parts // gl.RCHUNK)) * c["C"], what + ": workspace size"
            used = (parts + (-(-parts // gl.RCHUNK) if levels == 2 else 0)) * c["C"]
            assert unwritten(ws[:used]) == 0, what + ": a used slot of the workspace was never written"
        guard.check()
        _check("colsum", t["exact"], s, t["ref"], t["bound"], what)
        assert _same_bits(s, K.colsum(x)), what + ": second call differs"
        guard.check()


# ---- region_plan -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(gl.PLAN_CASES)), ids=[gl.case_id(c) for c in gl.PLAN_CASES])
def test_region_plan_is_a_plan_of_the_label_map(index, guard):
    from e4s_amd import kernels as K
    c = gl.PLAN_CASES[index]
    ha, wa = c["anchors"]
    for pattern in gl.gc.PATTERNS:
        lab = gl.plan_labels(c, pattern)
        pl = K.region_plan(_dev(lab), c["R"], ha, wa, c["nphase"])
        guard.check()
        assert pl.rows.numel() == c["B"] * ha * wa * c["nphase"] + c["B"] * c["R"] * c["nphase"] * gl.BM
        gl.check_plan(pl.rows.cpu().numpy(), pl.tiles.cpu().numpy(), pl.meta.cpu().numpy(), lab, c["B"], c["R"], ha, wa, c["nphase"])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_geometry_outside_the_kernels_sets_is_refused_before_any_launch(guard):
    """Every call returns an error code and leaves its (guarded) outputs as they were: no such kernel ever runs."""
    from e4s_amd import lib
    from e4s_amd.lib import fptr, ptr, stream
    L = lib.load()
    src, lab = torch.zeros(1 << 14, device=DEV), torch.zeros(1 << 10, device=DEV, dtype=torch.uint8)
    out = lambda: fptr(guard.empty(1 << 12, device=DEV))                                               # noqa: E731
    outi = lambda n=1 << 12: ptr(guard.empty(n, device=DEV, dtype=torch.int32))                        # noqa: E731
    x, st = fptr(src), stream()
    s = 1 / math.sqrt(3)
    cap = 1 * 4 * 4 * 1 + 1 * 3 * 1 * gl.BM          # rows_cap of a 4 x 4 anchor grid, one sample, 3 regions, one phase

    def plan(nphase, rows_cap):
        return lambda: L.e4s_region_plan(ptr(lab), 1, 3, 4, 4, 4, 4, nphase, gl.BM, outi(), outi(), outi(), outi(), rows_cap, (rows_cap + gl.BM - 1) // gl.BM, st)

    refused = [
        lambda: L.e4s_channel_sum_f32(x, out(), 100, 7, 3, st),                                          # n no multiple of step_b size_b
        lambda: L.e4s_channel_sum_f32(x, out(), 21, 0, 3, st),
        lambda: L.e4s_fused_bias_act_f32(x, None, None, out(), 64, 1, 1, 3, 1, 0.2, 1.0, st),            # code 31 without ref
        lambda: L.e4s_conv1x1_small_f32(x, x, None, out(), 1, 16, 0, 8, 8, s, 0, 0.2, 1.0, st),          # Cin = 0
        lambda: L.e4s_conv1x1_small_f32(x, x, None, out(), 1, 16, 5, 8, 8, s, 0, 0.2, 1.0, st),          # Cin = 5
        lambda: L.e4s_conv1x1_small_f32(x, x, None, out(), 1, 16, 3, 6, 8, s, 0, 0.2, 1.0, st),          # Cout = 6
        lambda: L.e4s_conv1x1_small_f32(x, x, None, out(), 1, 16, 3, 8, 10, s, 0, 0.2, 1.0, st),         # a channel stride that is no multiple of 4
        lambda: L.e4s_conv1x1_small_f32(x, x, None, out(), 1, 16, 3, 8, 4, s, 0, 0.2, 1.0, st),          # a channel stride below Cout
        lambda: L.e4s_noise_half_f32(x, x, x, out(), 16, 6, 16, 0, 0.2, 1.0, st),                        # C = 6
        lambda: L.e4s_noise_half_f32(x, x, x, out(), 16, 4, 16, 2, 0.2, 1.0, st),                        # coff = 2
        lambda: L.e4s_noise_half_f32(x, x, x, out(), 16, 4, 10, 4, 0.2, 1.0, st),                        # channel stride = 10
        lambda: L.e4s_add_scale_f32(x, x, out(), 1.0, 6, st),                                            # n = 6
        lambda: L.e4s_minibatch_stddev_f32(x, out(), 6, 4, 4, 5, 4, st),                                 # B % group != 0
        lambda: L.e4s_minibatch_stddev_f32(x, out(), 4, 4, 4, 4, 4, st),                                 # Cy <= C
        lambda: L.e4s_rowdot_f32(x, 6, x, None, out(), 2, 2, 6, 0, 1.0, st),                             # K = 6
        lambda: L.e4s_colsum_f32(x, out(), out(), 100, 6, st),                                           # C = 6
        plan(2, cap * 2),                                                                                # nphase = 2
        plan(1, cap - 1),                                                                                # rows_cap one short
    ]
    for n, call_ in enumerate(refused):
        assert call_() != 0, f"refusal {n}: the call was accepted"
        torch.cuda.synchronize()
        for dt in (torch.float32, torch.int32):
            for buf in guard.insides(dt):
                assert unwritten(buf) == buf.numel(), f"refusal {n}: a refused call wrote to a tensor"
        guard.check()
    # the neighbours of the refused geometry are taken
    assert L.e4s_conv1x1_small_f32(x, x, None, out(), 1, 16, 3, 8, 12, s, 0, 0.2, 1.0, st) == 0
    assert L.e4s_conv1x1_small_f32(x, x, None, out(), 1, 16, 3, 8, 0, s, 0, 0.2, 1.0, st) == 0          # stride 0: dense
    assert L.e4s_noise_half_f32(x, x, x, out(), 16, 4, 12, 4, 0.2, 1.0, st) == 0
    assert L.e4s_channel_sum_f32(x, out(), 105, 7, 3, st) == 0
    assert plan(1, cap)() == 0
    guard.check()
