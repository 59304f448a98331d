"""Face editing on the device (e4s_amd/edit.py, csrc/edit.hip) and per-channel noise in the epilogues of the split-bf16 conv family.

Per-channel noise [Bn,C,H,W] is what the reference's editor always generates with (face_edit.py:49-52, 96-97).  Layers are held to
the CPU oracle with the bound and error model of test_styled_conv_bf16x3_vs_oracle (1e-4 of the output scale), the whole generator to
the images the real reference produced (tests/golden/make_edit_golden.py), bound 1e-3.  Every per-channel run under "bf16x3" must
differ from the exact-fp32 run: before these epilogues could read the layout both ran the exact kernels.

Masked launches with per-channel noise never take the one-wave-per-SIMD kernel (path 2): with the noise reads in its epilogue it
spilled, so e4s_plan_masked keeps them on the 8-wave rows kernel; test_masked_paths pins that routing."""
import numpy as np
import pytest
import torch

import edit_cases as ec
from e4s_amd import synth
from oracle import e4s_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 2


def maxabs(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _styled_sd(cin, cout, up, seed):
    spec = [("conv.weight", (1, cout, cin, 3, 3), "randn"), ("conv.modulation.weight", (cin, 512), "randn"),
            ("conv.modulation.bias", (cin,), "modbias"), ("noise.weight", (1,), "noisew"), ("activate.bias", (cout,), "bias")]
    sd = {k: synth.synth_tensor(k, s, kind, seed) for k, s, kind in spec}
    if up:
        sd["conv.blur.kernel"] = orc.make_blur_kernel() * 4
    return sd


def _layer(case, monkeypatch):
    from e4s_amd import stylegan2 as S
    cin, cout, res, up, cells, masked, poly = case
    if poly:
        monkeypatch.setattr(S, "UPCONV_BF16X3_EXACT", False)
    sd = _styled_sd(cin, cout, up, 12)
    m = S.StyledConv(cin, cout, 3, 512, upsample=up, mask_op=masked)
    m.load_state_dict(sd)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, cin, res, res, generator=g)
    style = torch.randn(B, 12, 512, generator=g) if masked else torch.randn(B, 512, generator=g)
    mask = synth.onehot(synth.synth_labels_blocks(B, 512, cells, seed=7)) if masked else None
    return sd, m.to(DEV), x, style, mask, g


def _run(m, x, style, mask, noise):
    return m(x.to(DEV), style.to(DEV), mask.to(DEV) if mask is not None else None, noise=noise.to(DEV))


# ---- 1, 2: layers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bn", [1, B])
@pytest.mark.parametrize("case", ec.STYLED, ids=ec.styled_id)
def test_styled_conv_per_channel_noise_vs_oracle(case, bn, monkeypatch):
    from e4s_amd import kernels as K
    cin, cout, res, up, cells, masked, poly = case
    sd, m, x, style, mask, g = _layer(case, monkeypatch)
    out_res = 2 * res if up else res
    noise = torch.randn(bn, cout, out_res, out_res, generator=g)
    want = orc.styled_conv(sd, "", x, style, mask, noise, up, masked)
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    got = _run(m, x, style, mask, noise)
    got_cl = _run(m, x, style, mask, noise.contiguous(memory_format=torch.channels_last))       # the editor's storage: a view
    monkeypatch.setattr(K, "PRECISION", "f32")
    got32 = _run(m, x, style, mask, noise)
    scale = float(want.abs().max())
    print(ec.styled_id(case), "Bn", bn, "vs oracle", maxabs(got, want), "vs f32", maxabs(got, got32), "scale", scale)
    assert torch.equal(got, got_cl)
    assert 0.0 < maxabs(got, got32)                                  # the split-bf16 kernel really ran
    assert maxabs(got, want) < 1e-4 * scale, (maxabs(got, want), scale)


@pytest.mark.parametrize("bn", [1, B])
@pytest.mark.parametrize("case", ec.STYLED, ids=ec.styled_id)
def test_per_channel_copies_of_one_map_give_the_per_pixel_bits(case, bn, monkeypatch):
    """noise_w * noise is rounded on its own in both layouts, so [Bn,C,H,W] copies of a [Bn,1,H,W] map change no bit."""
    from e4s_amd import kernels as K
    cin, cout, res, up, cells, masked, poly = case
    _, m, x, style, mask, g = _layer(case, monkeypatch)
    out_res = 2 * res if up else res
    one = torch.randn(bn, 1, out_res, out_res, generator=g)
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    y1 = _run(m, x, style, mask, one)
    yc = _run(m, x, style, mask, one.expand(bn, cout, out_res, out_res).contiguous())
    assert torch.equal(y1, yc), maxabs(y1, yc)


@pytest.mark.parametrize("bn", [1, B])
def test_c32_fused_torgb_partial_keeps_its_bits(bn, monkeypatch):
    """32 -> 32 at 64^2 with rgb_ws: the output and the ToRGB partial equal the per-pixel run's."""
    from e4s_amd import kernels as K
    case = (32, 32, 64, False, 8, False, False)
    _, m, x, style, _, g = _layer(case, monkeypatch)
    one = torch.randn(bn, 1, 64, 64, generator=g)
    ws = torch.randn(B, 3, 32, generator=g).to(DEV)
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    xn = K.nchw_to_nhwc(x.to(DEV))
    s = K.modulate_vec(style.to(DEV), m.conv.modulation.weight, m.conv.modulation.bias)
    y1, p1 = m.run_nhwc(xn, s, one.to(DEV), rgb_ws=ws)
    yc, pc = m.run_nhwc(xn, s, one.expand(bn, 32, 64, 64).contiguous().to(DEV), rgb_ws=ws)
    assert torch.equal(y1, yc) and torch.equal(p1, pc)
    assert float(p1.abs().max()) > 0


def test_masked_paths(monkeypatch):
    """Which kernel a masked launch with per-channel noise takes: the packed small-map tiles (3) at 4^2, the 8-wave rows kernel (1)
    elsewhere -- also where the same launch with per-pixel noise takes the one-wave kernel (2).  Copies of one map give the per-pixel
    bits where both layouts run the same kernel; at 128^2 they run two kernels that add the products in different orders (measured
    2.9e-6 apart), each within 1e-4 of the output scale of the exact result (test_styled_conv_bf16x3_vs_oracle's model), so within
    2e-4 of it of each other."""
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    seen = {}
    for case in [(512, 512, 4, False, 64, True, False), (512, 512, 16, False, 16, True, False), (256, 256, 128, False, 16, True, False)]:
        cin, cout, res = case[:3]
        _, m, x, style, mask, g = _layer(case, monkeypatch)
        one = torch.randn(1, 1, res, res, generator=g)
        monkeypatch.setattr(K, "LAST_REGION_PATH", 0)
        y1 = _run(m, x, style, mask, one)
        p1 = K.LAST_REGION_PATH
        yc = _run(m, x, style, mask, one.expand(1, cout, res, res).contiguous())
        seen[res] = (p1, K.LAST_REGION_PATH)
        if seen[res][0] == seen[res][1]:
            assert torch.equal(y1, yc), (case, maxabs(y1, yc))
        else:
            print(case, "one-wave kernel (per-pixel) vs 8-wave kernel (per-channel):", maxabs(y1, yc))
            assert maxabs(y1, yc) < 2e-4 * float(y1.abs().max())
    print("paths (per-pixel, per-channel) by resolution:", seen)
    assert seen[4] == (3, 3) and seen[16] == (1, 1)
    assert seen[128] == ((2 if K.REGION_1W else 1), 1)


# ---- 3: the fallback ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ec.STYLED[0], ec.STYLED[4], ec.STYLED[7], ec.STYLED[9], ec.STYLED[11]], ids=ec.styled_id)
def test_fallback_runs_the_exact_kernels(case, monkeypatch):
    """PC_NOISE_SPLIT = False: per-channel noise under "bf16x3" gives the bits of "f32" (the dispatch before this feature)."""
    from e4s_amd import kernels as K
    from e4s_amd import stylegan2 as S
    cin, cout, res, up, cells, masked, poly = case
    _, m, x, style, mask, g = _layer(case, monkeypatch)
    out_res = 2 * res if up else res
    noise = torch.randn(1, cout, out_res, out_res, generator=g)
    monkeypatch.setattr(S, "PC_NOISE_SPLIT", False)
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    got = _run(m, x, style, mask, noise)
    monkeypatch.setattr(K, "PRECISION", "f32")
    assert torch.equal(got, _run(m, x, style, mask, noise))


# ---- 4: the generator against the reference ---------------------------------------------------------------------------------------
_NETS = {}


def _net(size):
    if size not in _NETS:
        from e4s_amd.networks import Net3
        from e4s_amd.options import make_opts
        net = Net3(make_opts(out_size=size))
        net.load_state_dict(synth.synth_state_dict(size, 13), strict=True)
        net.latent_avg = synth.synth_latent_avg(size).to(DEV)
        _NETS[size] = net.to(DEV).eval()
    return _NETS[size]


@pytest.fixture(scope="module")
def setup(golden):
    """Per output size: the fixture, the texture vectors it was made from, the label map and the noise list -- drawn once."""
    from e4s_amd import edit
    cache = {}

    def get(size):
        if size not in cache:
            rec = ec.golden("edit.pt" if size == 256 else "edit1024.pt")
            base = golden(f"net{size}.pt")
            lab = synth.synth_labels_blocks(1, 512, 64, seed=3) if size == 256 else synth.synth_labels_face(1, 512, seed=3)
            cache[size] = dict(rec=rec, src=base["driven_sv"].to(DEV), ref=base["target_sv"].to(DEV),
                               labels=lab[:, 0].to(torch.uint8).to(DEV), noise=edit.make_noise(size, DEV, seed=rec["noise_seed"]))
        return cache[size]
    return get


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "auto"])
@pytest.mark.parametrize("size", [256, 1024])
def test_generator_with_per_channel_noise_vs_reference(size, precision, setup, monkeypatch):
    from e4s_amd import edit
    from e4s_amd import kernels as K
    s = setup(size)
    rec = s["rec"]
    monkeypatch.setattr(K, "PRECISION", precision)
    calls = {"torgb_finish": 0, "transpose": 0}
    real_finish, real_tr = K.torgb_finish, K.nchw_to_nhwc

    def finish(*a, **k):
        calls["torgb_finish"] += 1
        return real_finish(*a, **k)

    def transpose(t):
        calls["transpose"] += t.numel() > 3 * 4 * 4 * 512                 # (the 4^2 constant input is not a noise map)
        return real_tr(t)
    monkeypatch.setattr(K, "torgb_finish", finish)
    monkeypatch.setattr(K, "nchw_to_nhwc", transpose)
    ed = edit.FaceEditor(_net(size))
    alphas = torch.tensor(rec["alphas"])                                  # the three edits of the fixture as ONE batch
    img = ed.texture_edit(s["src"], s["ref"], s["labels"], rec["regions"], alphas, s["noise"], as_float=True).cpu()
    assert tuple(img.shape) == (3, 3, size, size)
    assert calls["transpose"] == 0                                        # channels-last maps are views
    if size == 256:
        errs = [maxabs(img[1:2], rec["img"]), maxabs(img[[0, 2]][:, :, ::4, ::4], rec["img_stride4"])]
    else:
        c0 = size // 2 - 64
        errs = [maxabs(img[:, :, ::8, ::8], rec["img_stride8"]), maxabs(img[1:, :, c0:c0 + 128, c0:c0 + 128], rec["img_crop"])]
        if precision == "auto":
            assert calls["torgb_finish"] >= 1                             # the 32 -> 32 conv at 1024^2 took conv_c32 with the fused ToRGB
    print(size, precision, "max |image - reference|", errs)
    assert max(errs) < 1e-3, errs
    u8 = ed.texture_edit(s["src"], s["ref"], s["labels"], rec["regions"], alphas, s["noise"])
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (3, size, size, 3)


# ---- 5: the mix and the joins -------------------------------------------------------------------------------------------------
def test_texture_mix_equals_the_reference_rows(golden):
    from e4s_amd import edit
    from e4s_amd import kernels as K
    rec = ec.golden("edit.pt")
    base = golden("net256.pt")
    src, ref = base["driven_sv"], base["target_sv"]
    order = [edit.COMP2INDEX[r] for r in rec["regions"]]
    alphas = torch.tensor(rec["alphas"])
    sel, a0, a1 = edit.mix_coefficients(rec["regions"], alphas, 3)
    out = K.texture_mix(src.to(DEV), ref.to(DEV), sel.to(DEV), a0.to(DEV), a1.to(DEV)).cpu()      # [1,R,C] operands, three alphas
    for k in range(3):
        assert torch.equal(out[k, order], rec["mixed_rows"][k])
    assert torch.equal(out, ec.mix_ref(src, ref, sel, a0, a1))
    ed_out = edit.FaceEditor(_net(256)).mix(src.to(DEV), ref.to(DEV), rec["regions"], alphas.to(DEV)).cpu()
    assert torch.equal(ed_out, out)


@pytest.mark.parametrize("c", [1280, 1281, 6])
def test_texture_mix_edges(c):
    """Bn = 1 sources against B references, per-sample coefficients, unselected rows copied bit for bit (-0.0, a NaN payload), a row
    length that is no multiple of 4 (the scalar kernel)."""
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(3)
    b, r = 3, 12
    src, ref = torch.randn(1, r, c, generator=g), torch.randn(b, r, c, generator=g)
    src[0, 0, :3] = torch.tensor([-0.0, 0.0, float("inf")])
    src[0, 0, 3:5] = torch.from_numpy(np.array([0x7FC01234, 0xFFC00001], dtype=np.uint32).view(np.float32))
    sel = (torch.rand(b, r, generator=g) < 0.5).to(torch.uint8)
    sel[:, 0] = 0
    a1 = torch.rand(b, r, generator=g)
    a0 = (1.0 - a1.double()).float()
    out = K.texture_mix(src.to(DEV), ref.to(DEV), sel.to(DEV), a0.to(DEV), a1.to(DEV)).cpu()
    want = ec.mix_ref(src, ref, sel, a0, a1)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))                 # bit patterns: -0.0 and NaN payloads too
    assert torch.equal(out[:, 0].view(torch.int32), src[0, 0].view(torch.int32).expand(b, -1))
    out2 = K.texture_mix(ref.to(DEV), src.to(DEV), sel.to(DEV), a0.to(DEV), a1.to(DEV)).cpu()   # B sources, one reference
    assert torch.equal(out2.view(torch.int32), ec.mix_ref(ref, src, sel, a0, a1).view(torch.int32))
    with pytest.raises(ValueError):
        K.texture_mix(src.to(DEV), ref.to(DEV)[:2], sel.to(DEV), a0.to(DEV), a1.to(DEV))
    with pytest.raises(RuntimeError):
        K.texture_mix(src, ref.to(DEV), sel.to(DEV), a0.to(DEV), a1.to(DEV))


def test_mask_joins_equal_the_reference():
    from e4s_amd import edit
    j = ec.golden("edit.pt")["joins"]
    labels, colored = j["labels"].to(DEV), j["colored"].to(DEV)
    assert torch.equal(edit.label_map_to_colored_mask(labels).cpu(), j["colored"])
    assert torch.equal(edit.colored_mask_to_label_map(j["colored_in"].to(DEV)).cpu(), j["labels_back"])
    back = edit.colored_mask_to_label_map(colored)
    brushed = edit.edit_mask(back, j["brush"].to(DEV), "hair")
    assert torch.equal(brushed.cpu(), j["brushed"])
    assert torch.equal(edit.label_map_to_colored_mask(brushed).cpu(), j["brushed_colored"])
    rgb_brush = j["brush"][..., :3].contiguous().to(DEV)                               # an RGB brush; in place
    assert edit.edit_mask(back, rgb_brush, "hair", out=back) is back
    assert torch.equal(back.cpu(), j["brushed"])


@pytest.mark.parametrize("n,lead", [(4093, 1), (7, 0), (4096, 2), (1, 3)])
def test_mask_joins_on_unaligned_and_odd_sized_maps(n, lead):
    """Pointers that are no multiple of 4 and sizes that are no multiple of 4 pixels take the byte-wise paths; batched shapes."""
    from e4s_amd import kernels as K
    g = np.random.RandomState(n)
    lab = g.randint(0, 24, size=n + lead).astype(np.uint8)
    lab[::17] = 255
    rgb = ec.labels_to_color_ref(lab)
    rgb[::5] = g.randint(0, 256, size=rgb[::5].shape)
    brush = (g.randint(0, 256, size=(n + lead, 4)) * (g.rand(n + lead, 1) < 0.3)).astype(np.uint8)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    d_lab, d_rgb, d_br = t(lab)[lead:], t(rgb.reshape(-1))[3 * lead:].view(n, 3), t(brush.reshape(-1))[4 * lead:].view(n, 4)
    assert np.array_equal(K.labels_to_color(d_lab).cpu().numpy(), ec.labels_to_color_ref(lab[lead:]))
    assert np.array_equal(K.color_to_labels(d_rgb).cpu().numpy(), ec.color_to_labels_ref(rgb[lead:]))
    assert np.array_equal(K.mask_brush(d_lab, d_br, 9).cpu().numpy(), ec.brush_ref(lab[lead:], brush[lead:], 9))
    br3 = t(brush[:, :3].reshape(-1))[3 * lead:].view(n, 3)
    assert np.array_equal(K.mask_brush(d_lab, br3, 200).cpu().numpy(), ec.brush_ref(lab[lead:], brush[lead:, :3], 200))
    with pytest.raises(ValueError):
        K.mask_brush(d_lab, d_rgb[: n - 1] if n > 1 else d_rgb.view(-1), 3)
    with pytest.raises(RuntimeError):
        K.labels_to_color(d_lab.cpu())


# ---- 6: the captured edit -------------------------------------------------------------------------------------------------------
def test_graphed_edit_replays_the_eager_edit(setup):
    from e4s_amd import edit
    s = setup(256)
    net = _net(256)
    ed = edit.FaceEditor(net)
    src, ref = s["src"].expand(B, -1, -1).contiguous(), torch.flip(s["ref"], [1]).expand(B, -1, -1).contiguous()
    ref[1] = s["ref"][0]
    labels = torch.cat([s["labels"], torch.flip(s["labels"], [2])])
    g = edit.GraphedFaceEdit(net, B, s["noise"])
    g.load(src_sv=src, ref_sv=ref, labels=labels, regions=["hair", "skin"], alpha=0.3)
    out = g.replay().clone()
    graph = g.graph
    want = ed.texture_edit(src, ref, labels, ["hair", "skin"], 0.3, s["noise"])
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, 256, 256, 3)
    assert torch.equal(out, want)
    assert torch.equal(g.image, ed.texture_edit(src, ref, labels, ["hair", "skin"], 0.3, s["noise"], as_float=True))
    # a slider move, other regions, per-sample alphas: writes into sel / a0 / a1, the same graph
    alphas = torch.tensor([0.8, 0.1])
    g.set_mix(["lip", "nose", "eyes"], alphas)
    assert torch.equal(g.replay(), ed.texture_edit(src, ref, labels, ["lip", "nose", "eyes"], alphas, s["noise"]))
    g.a1[:, 1] = 0.5                                                       # ... or written on the device
    g.a0[:, 1] = 0.5
    g.sel[:, 3] = 0
    sel, a0, a1 = g.sel.clone(), g.a0.clone(), g.a1.clone()
    from e4s_amd import kernels as K
    mixed = K.texture_mix(src, ref, sel, a0, a1)
    assert torch.equal(g.replay(), ed.generate(mixed, labels, s["noise"]))
    # an edited label map (shape editing is sel = 0 and new labels)
    brush = torch.zeros(B, 512, 512, 4, dtype=torch.uint8, device=DEV)
    brush[:, 100:300, 150:400, 0] = 255
    edit.edit_mask(g.labels, brush, "hair", out=g.labels)
    g.sel.zero_()
    assert not torch.equal(g.labels, labels)
    assert torch.equal(g.replay(), ed.shape_edit(src, g.labels.clone(), s["noise"]))
    # alpha = 0 is plain generation from the source's vectors
    g.load(labels=labels, regions=["hair", "skin", "lip"], alpha=0.0)
    assert torch.equal(g.replay(), ed.generate(src, labels, s["noise"]))
    assert g.graph is graph                                                # never re-captured
    g.validate()                                                           # every mask so far was one-hot
    g.mask[:, :2, :8, :8] = 0.5                                            # a soft mask of the caller's own
    g.replay(from_labels=False)
    with pytest.raises(RuntimeError, match="one-hot"):
        g.validate()
    g.replay()
    g.validate()
