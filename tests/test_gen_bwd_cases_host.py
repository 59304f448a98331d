"""The yardsticks of tests/test_gpu_gen_backward_kernels.py checked on the CPU, before any kernel is involved (tests/gen_bwd_cases.py)."""
import numpy as np
import pytest
import torch

import gen_bwd_cases as gc


def _closed_form(gz, d, x, s, Wt, reg, R, ncls, region_of_input_pixel=False):
    """dx and ds as the header of csrc/dgrad_scatter.hip states them, in fp64 numpy:
         G_ph[m, t, ci] = sum_co u[m_ph, co] W[ph][t][co][ci],   u = gz d[r]
         dx[h, ci]      = sum_ph sum_t s[r_ph(m_t), ci] G_ph[m_t, t, ci],   m_t = h - (t - 1)
         ds[rho, ci]    = sum_ph sum_{m: r_ph(m) = rho} sum_t x[m + t - 1, ci] G_ph[m, t, ci]
    region_of_input_pixel: the deliberate mistake of taking s at the region of h (ncls 1 only)."""
    gz, d, x, s, Wt, reg = (np.asarray(a.double() if a.is_floating_point() else a) for a in (gz, d, x, s, Wt, reg))
    B, H, W, C = x.shape
    os_ = 2 if ncls == 4 else 1
    bi = np.arange(B)[:, None, None]
    u = gz * d.reshape(B, R, -1)[bi, reg]
    dx, ds = np.zeros_like(x), np.zeros((B, R, C))
    for ph in range(ncls):
        r_ph, u_ph = reg[:, (ph >> 1)::os_, (ph & 1)::os_], u[:, (ph >> 1)::os_, (ph & 1)::os_]
        for t in range(9):
            ty, tx = t // 3 - 1, t % 3 - 1
            G = np.einsum("bhwo,oc->bhwc", u_ph, Wt[ph, t])
            ys, xs = slice(max(0, -ty), min(H, H - ty)), slice(max(0, -tx), min(W, W - tx))              # source rows m with m + t - 1 inside
            yd, xd = slice(ys.start + ty, ys.stop + ty), slice(xs.start + tx, xs.stop + tx)              # h = m + t - 1
            r_for_dx = r_ph[:, yd, xd] if region_of_input_pixel else r_ph[:, ys, xs]
            dx[:, yd, xd] += s.reshape(B, R, C)[bi, r_for_dx] * G[:, ys, xs]
            xG = np.zeros_like(G)
            xG[:, ys, xs] = x[:, yd, xd] * G[:, ys, xs]
            np.add.at(ds, (np.broadcast_to(bi, r_ph.shape), r_ph), xG)
    return dx, ds.reshape(B * R, C)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("ncls", [1, 4])
def test_autograd_reference_equals_the_documented_scatter_algebra(ncls):
    """fp64 autograd through the forward (region of the OUTPUT pixel) == the closed-form dx and ds of the kernel file's header, to 1e-12
    relative; the same algebra with the region of the INPUT pixel is far away, so the check can tell the two apart."""
    B, H, W, C, Cy, R = 2, 6, 7, 8, 4, 5
    os_ = 2 if ncls == 4 else 1
    g = torch.Generator().manual_seed(11 + ncls)
    labels = gc.make_labels("noise", B, 5, 9, R, seed=ncls)
    reg = gc.region_map(labels, H * os_, W * os_)
    gz, d = gc.operand((B, H * os_, W * os_, Cy), "random", g), gc.operand((B * R, Cy), "random", g)
    x, s, Wt = gc.operand((B, H, W, C), "random", g), gc.operand((B * R, C), "random", g), gc.operand((ncls, 9, Cy, C), "random", g)
    ref = gc.dgrad_ref(gz, d, x, s, Wt, reg, R, ncls)
    dx, ds = _closed_form(gz, d, x, s, Wt, reg, R, ncls)
    assert _rel(dx, ref["dx"]) < 1e-12 and _rel(ds, ref["ds"]) < 1e-12, (_rel(dx, ref["dx"]), _rel(ds, ref["ds"]))
    # the scatter products the GPU test hands to col2im_region carry the same gradients
    xg, sg = x.double().requires_grad_(True), s.double().requires_grad_(True)
    dx2, ds2 = torch.autograd.grad(gc.scatter_form(xg, gc._pix(sg, reg, R), ref["G"], ncls), (xg, sg))
    assert _rel(dx2, ref["dx"]) < 1e-12 and _rel(ds2, ref["ds"]) < 1e-12
    if ncls == 1:
        bad, _ = _closed_form(gz, d, x, s, Wt, reg, R, ncls, region_of_input_pixel=True)
        assert _rel(bad, ref["dx"]) > 1e-3


def test_elementwise_references_against_a_pixel_loop():
    """act_ref and torgb_ref against a plain per-pixel loop over the interpolated regions (one small case)."""
    B, H, W, C, R = 2, 3, 5, 4, 3
    g = torch.Generator().manual_seed(5)
    labels = gc.make_labels("noise", B, 7, 4, R, seed=2)
    reg = gc.region_map(labels, H, W)
    dy, y, noise, bias = (gc.operand(sh, "random", g) for sh in ((B, H, W, C), (B, H, W, C), (B, 1, H, W), (C,)))
    drgb, ws = gc.operand((B, 3, H, W), "random", g), gc.operand((B * R, 3, C), "random", g)
    a, gain, nw = float(np.float32(0.2)), float(np.float32(2 ** 0.5)), float(np.float32(0.3))
    dd, dws, dxr = np.zeros((B * R, C)), np.zeros((B * R, 3, C)), np.zeros((B, H, W, C))
    for b in range(B):
        for i in range(H):
            for j in range(W):
                r = int(reg[b, i, j])
                for c in range(C):
                    yv, xv = float(y[b, i, j, c]), float(dy[b, i, j, c])
                    sl = gain if yv > 0 else gain * a
                    dd[b * R + r, c] += xv * sl * (yv / sl - nw * float(noise[b, 0, i, j]) - float(bias[c]))
                    for ch in range(3):
                        dws[b * R + r, ch, c] += float(drgb[b, ch, i, j]) * float(y[b, i, j, c])
                        dxr[b, i, j, c] += float(drgb[b, ch, i, j]) * float(ws[b * R + r, ch, c])
    ref = gc.act_ref(dy, y, noise, 0.3, bias, 0.2, 2 ** 0.5, reg, R)
    assert _rel(ref["dd"], dd) < 1e-12
    tr = gc.torgb_ref(drgb, y, ws, reg, R)
    assert _rel(tr["dws"], dws) < 1e-12 and _rel(tr["dx"], dxr) < 1e-12
    assert (np.asarray(tr["dws_abs"]) >= np.abs(dws) - 1e-12).all() and (np.asarray(ref["dd_abs"]) >= np.abs(dd) - 1e-12).all()


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_dyadic_cases_are_exact_in_fp32(name):
    """For every dyadic case of the GPU test: S_abs 2^k < 2^24 with 2^-k the quantum of the terms (every partial sum, in any order, is then
    an fp32 number), and the reference survives the round trip through fp32."""
    for i, c in enumerate(gc.CASES[name]):
        t = gc.build(name, i, "dyadic")
        ref = t["ref"]
        for out, sabs, k in gc.SUMMED[name]:
            scaled = ref[out] * 2.0 ** k
            assert torch.equal(scaled, scaled.round()), (gc.case_id(c), out)
            assert float(ref[sabs].max()) * 2.0 ** k < 2 ** 24, (gc.case_id(c), out, float(ref[sabs].max()) * 2.0 ** k)
            assert (ref[sabs] >= ref[out].abs()).all()
        for key, v in ref.items():
            if torch.is_tensor(v) and v.is_floating_point() and not key.endswith("_abs"):
                assert torch.equal(v.float().double(), v), (gc.case_id(c), key)


@pytest.mark.parametrize("pattern", gc.PATTERNS)
def test_label_generators_stay_below_R_and_keep_their_promises(pattern):
    for R in (1, 3, 5, 12, 16):
        for B in (1, 3):
            if pattern == "absent" and R < 3:
                with pytest.raises(ValueError):
                    gc.make_labels(pattern, B, 9, 10, R, seed=R)
                continue
            for hm, wm in ((3, 4), (10, 9), (64, 64)):
                lab = gc.make_labels(pattern, B, hm, wm, R, seed=R + B)
                assert lab.dtype == torch.uint8 and lab.shape == (B, hm, wm) and int(lab.max()) < R
                if pattern == "one":
                    assert int(lab.min()) == int(lab.max())
                if pattern == "absent":
                    first, last = gc.absent_regions(R)
                    assert not (lab[0] == first).any() and not (lab[-1] == last).any()
                    for H, W in ((5, 7), (13, 37)):               # and so they stay after the resize to any grid
                        reg = gc.region_map(lab, H, W)
                        assert not (reg[0] == first).any() and not (reg[-1] == last).any()


def test_every_case_list_meets_every_value_with_every_pattern():
    for name in ("act", "demod", "torgb", "dgrad"):
        cases = [c for c in gc.CASES[name] if c["pattern"] is not None]
        for pattern in gc.PATTERNS:
            mine = [c for c in cases if c["pattern"] == pattern]
            assert {c["grid"] for c in mine} == {(5, 7), (16, 24), (13, 37), (33, 50)}
            assert {c["rel"] for c in mine} == {"larger", "equal", "smaller"}
            assert {c["B"] for c in mine} == {1, 3}
            assert {c["R"] for c in mine} >= ({5, 12, 16} | ({3} if pattern == "absent" else {1}))
            assert len({c["C"] for c in mine}) == 4
