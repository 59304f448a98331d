"""GPU tests of GPEN's ParseNet (e4s_amd/parsenet.py, csrc/parsenet.hip) against the REAL reference's fp64 outputs
(tests/golden/parsenet.pt, tests/golden/make_parsenet_golden.py) and fp64 torch restatements of the reflect-padded conv.

Bounds (those of test_gpu_sr.py): a single layer 1e-5 x scale (f32) and 1e-3 x scale (bf16x3); the whole network 1e-4 x scale and
1e-3 x scale.  Masks: a pixel's mask depends on the sign of (best logit of classes 0 / 14 / 18) - (best logit of the rest); two
logits that each move by at most bound x scale cannot change that sign where the fp64 margin exceeds 2 x bound x scale, so every
such pixel must equal the fixture exactly, and at most 1 % of the pixels may be excluded."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import unz
from e4s_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = [("f32", 1e-5, 1e-4), ("bf16x3", 1e-3, 1e-3)]                 # (PRECISION, single-layer bound, whole-network bound)
SENTINEL = 12345.0
PAIRS = [(64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 128), (128, 64)]     # every (Cin, Cout) of the three nets
PAIRS_S2 = [(64, 128), (128, 128), (128, 256), (256, 256)]                                   # those that run at stride 2

_NETS = {}


def _net(g, ni):
    """The seeded ParseNet `ni` of the fixture on the device (one per session: the weight packs are keyed on the precision)."""
    from e4s_amd.parsenet import ParseNet
    if ni not in _NETS:
        size, osize, mfs, depth = g["nets"][ni]
        net = ParseNet(size, osize, mfs, 64, 19, res_depth=depth, norm_type="bn", relu_type="LeakyReLU", ch_range=[32, 256])
        net.load_state_dict(synth.synth_parsenet_state_dict(net), strict=True)
        _NETS[ni] = net.to(DEV).eval()
    return _NETS[ni]


def _face_parse(g):
    from e4s_amd.parsenet import FaceParse
    if "fp" not in _NETS:
        fp = FaceParse(base_dir=None, device=DEV)
        fp.faceparse = _net(g, 2)
        _NETS["fp"] = fp
    return _NETS["fp"]


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def _conv64(x_nhwc, w, stride=1, up2=False):
    """fp64 restatement: NHWC fp32 values -> [nearest x2] -> F.pad(reflect, 1) -> conv2d(stride), NHWC fp64."""
    x = x_nhwc.double().permute(0, 3, 1, 2)
    if up2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w.double(), None, stride=stride).permute(0, 2, 3, 1)


def _err(got, ref, tol, what):
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max())
    print(f"{what}: err {err:.3e} = {err / scale:.2e} x scale (bound {tol:.0e})")
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    assert err <= tol * scale, (what, err, scale)


def _run(K, x, wt, cout, ho, wo, **kw):
    y = torch.full((x.shape[0], ho, wo, cout), SENTINEL).to(DEV)
    K.pconv(x.to(DEV), wt.shape[1], K.pconv_pack(wt.to(DEV), K.sr_f32()), cout, y, **kw)
    return y.cpu()


@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
@torch.no_grad()
def test_reflect_conv_strides_and_folded_upsampling_at_small_and_multi_tile_shapes(monkeypatch, precision, tol, _):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    wt = _rand(64, 64, 3, 3, seed=1) / (9 * 64) ** 0.5
    cases = [((2, 2, 2), 1, False), ((2, 9, 13), 1, False), ((1, 17, 33), 1, False),          # the last: > 1 tile per axis, overhang
             ((2, 2, 2), 2, False), ((2, 9, 13), 2, False), ((1, 18, 34), 2, False), ((1, 17, 33), 2, False),
             ((2, 5, 1), 1, True), ((1, 9, 13), 1, True)]
    for (b, h, w), stride, up2 in cases:
        x = _rand(b, h, w, 64, seed=h * w + stride)
        ref = _conv64(x, wt, stride, up2)
        g = 2 if up2 else 1
        assert tuple(ref.shape[1:3]) == ((g * h + 2 - 3) // stride + 1, (g * w + 2 - 3) // stride + 1)
        got = _run(K, x, wt, 64, ref.shape[1], ref.shape[2], stride=stride, up2=up2)
        _err(got, ref, tol, f"{precision} {(b, h, w)} stride {stride} up2 {up2}")


@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
@torch.no_grad()
def test_every_channel_pair_of_the_net(monkeypatch, precision, tol, _):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    for stride, pairs in ((1, PAIRS), (2, PAIRS_S2)):
        for cin, cout in pairs:
            x = _rand(2, 9, 13, cin, seed=cin + cout)
            wt = _rand(cout, cin, 3, 3, seed=cin * 3 + cout) / (9 * cin) ** 0.5
            ref = _conv64(x, wt, stride)
            _err(_run(K, x, wt, cout, ref.shape[1], ref.shape[2], stride=stride), ref, tol, f"{precision} {cin}->{cout} stride {stride}")


@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
@torch.no_grad()
def test_epilogues_and_untouched_channel_padding(monkeypatch, precision, tol, _):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    b, h, w, cin, cout = 2, 9, 13, 64, 128
    x = _rand(b, h, w, cin + 8, seed=1)
    x[..., cin:] = SENTINEL                                               # channels past Cin are never read
    wt = _rand(cout, cin, 3, 3, seed=2) / (9 * cin) ** 0.5
    scale, bias = 1 + 0.3 * _rand(cout, seed=3), _rand(cout, seed=4)
    r0, r1 = torch.full((b, h, w, cout + 8), SENTINEL), torch.full((b, h, w, cout + 4), SENTINEL)
    r0[..., :cout], r1[..., :cout] = _rand(b, h, w, cout, seed=5), _rand(b, h, w, cout, seed=6)
    conv = _conv64(x[..., :cin], wt)
    aff = conv * scale.double() + bias.double()
    act = F.leaky_relu(aff, 0.2)
    pack = K.pconv_pack(wt.to(DEV), K.sr_f32())
    xd, r0d, r1d = x.to(DEV), r0.to(DEV), r1.to(DEV)
    variants = [("plain", {}, conv), ("bias", dict(bias=bias), conv + bias.double()), ("scale", dict(scale=scale), conv * scale.double()),
                ("scale+bias", dict(scale=scale, bias=bias), aff), ("lrelu", dict(scale=scale, bias=bias, lrelu=True), act),
                ("lrelu+r0", dict(scale=scale, bias=bias, lrelu=True, r0=r0d), act + r0[..., :cout].double()),
                ("r0+r1", dict(bias=bias, r0=r0d, r1=r1d), conv + bias.double() + r0[..., :cout].double() + r1[..., :cout].double())]
    for name, kw, ref in variants:
        kw = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        y = torch.full((b, h, w, cout + 4), SENTINEL).to(DEV)
        K.pconv(xd, cin, pack, cout, y, **kw)
        got = y.cpu()
        _err(got[..., :cout], ref, tol, f"{precision} {name}")
        assert torch.equal(got[..., cout:], torch.full((b, h, w, 4), SENTINEL))      # the output's channel padding is not touched
    assert torch.equal(r0d.cpu(), r0) and torch.equal(r1d.cpu(), r1) and torch.equal(xd.cpu(), x)
    # in place over the residual it reads (a block may write identity + res over the identity)
    K.pconv(xd, cin, pack, cout, r1d, bias=bias.to(DEV), r0=r1d)
    _err(r1d.cpu()[..., :cout], conv + bias.double() + r1[..., :cout].double(), tol, f"{precision} in place")
    assert torch.equal(r1d.cpu()[..., cout:], r1[..., cout:])
    # refused: the output over the input, up2 at stride 2, a map too small to reflect, channel counts off the 32-grid
    with pytest.raises(RuntimeError):
        K.pconv(xd, cin, pack, cin, xd)
    with pytest.raises(RuntimeError):
        K.pconv(xd, cin, pack, cout, torch.empty(b, h, w, cout, device=DEV), stride=2, up2=True)
    with pytest.raises(RuntimeError):
        K.pconv(torch.zeros(1, 1, 5, cin, device=DEV), cin, pack, cout, torch.empty(1, 1, 5, cout, device=DEV))
    with pytest.raises(RuntimeError):
        K.pconv_pack(torch.zeros(48, 64, 3, 3, device=DEV), True)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("stride,up2", [(1, False), (2, False), (1, True)])
@torch.no_grad()
def test_the_batch_and_the_tile_position_do_not_change_a_samples_bits(monkeypatch, precision, stride, up2):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    x = _rand(3, 17, 33, 64, seed=9)
    wt = _rand(64, 64, 3, 3, seed=10) / 24.0
    ho, wo = K.pconv_out_size(17, stride, up2), K.pconv_out_size(33, stride, up2)
    batch = _run(K, x, wt, 64, ho, wo, stride=stride, up2=up2)
    for i in range(3):
        assert torch.equal(_run(K, x[i:i + 1], wt, 64, ho, wo, stride=stride, up2=up2)[0], batch[i])
    # a periodic image: interior outputs one period apart lie in different tiles / tile rows and must carry the same bits
    if not up2:
        xp = _rand(1, 4, 4, 64, seed=11).repeat(1, 12, 12, 1)              # 48 x 48, period 4
        yp = _run(K, xp, wt, 64, K.pconv_out_size(48, stride), K.pconv_out_size(48, stride), stride=stride)
        per = 4 // stride
        inner = yp[0, per:-per, per:-per]
        assert torch.equal(inner[per:], inner[:-per]) and torch.equal(inner[:, per:], inner[:, :-per])


@torch.no_grad()
def test_head_reads_uint8_pixels_normalised_as_the_reference_does():
    from e4s_amd import kernels as K
    b, h, w = 2, 6, 10
    img = synth.synth_sr_input_u8(b, h, w, seed=3)
    wt, bias = _rand(64, 3, 3, 3, seed=4) / 27 ** 0.5, _rand(64, seed=5)
    wp = wt.permute(2, 3, 1, 0).reshape(27, 64).contiguous()
    x32 = (img.permute(0, 3, 1, 2).double() / 255.0 * 2 - 1).float()      # face_parsing.py:59-63
    ref = F.conv2d(F.pad(x32.double(), (1, 1, 1, 1), mode="reflect"), wt.double(), bias.double()).permute(0, 2, 3, 1)
    y = K.parsenet_head(img.to(DEV), wp.to(DEV), bias.to(DEV), torch.empty(b, h, w, 64, device=DEV))
    _err(y.cpu(), ref, 1e-5, "head uint8")
    yf = K.parsenet_head(x32.to(DEV), wp.to(DEV), bias.to(DEV), torch.empty(b, h, w, 64, device=DEV))
    assert torch.equal(yf, y)                                              # the same fp32 pixels, given as floats
    yb = K.parsenet_head(img.flip(-1).contiguous().to(DEV), wp.to(DEV), bias.to(DEV), torch.empty(b, h, w, 64, device=DEV), flip=True)
    assert torch.equal(yb, y)                                              # BGR pixels with flip = RGB pixels without


@torch.no_grad()
def test_tail_logits_first_maximum_and_colour_map():
    from e4s_amd import kernels as K
    from e4s_amd.parsenet import MASK_COLORMAP
    b, h, w = 2, 6, 10
    x = _rand(b, h, w, 64, seed=6)
    wt, bias = _rand(19, 64, 3, 3, seed=7) / 24.0, _rand(19, seed=8)
    lut = torch.tensor(MASK_COLORMAP, dtype=torch.uint8)

    def tail(wt, bias):
        wp = F.pad(wt.permute(2, 3, 1, 0).reshape(9, 64, 19), (0, 1)).contiguous()
        m, lab, lg = K.parsenet_tail(x.to(DEV), 64, wp.to(DEV), bias.to(DEV), mask=True, labels=True, logits=True)
        return m.cpu(), lab.cpu(), lg.cpu()

    m, lab, lg = tail(wt, bias)
    ref = F.conv2d(F.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect"), wt.double(), bias.double())
    _err(lg, ref, 1e-5, "tail logits")
    assert torch.equal(lab.long(), lg.argmax(1)) and torch.equal(m, lut[lab.long()])
    assert len(set(lab.flatten().tolist())) > 4                           # a real contest between classes
    only_mask = K.parsenet_tail(x.to(DEV), 64, F.pad(wt.permute(2, 3, 1, 0).reshape(9, 64, 19), (0, 1)).contiguous().to(DEV),
                                bias.to(DEV))
    assert only_mask[1] is None and only_mask[2] is None and torch.equal(only_mask[0].cpu(), m)
    # ties resolve to the first index: classes 3 and 7 (then 14 and 18) get the same weights and a bias above every other class
    for first, second, colour in ((3, 7, 255), (14, 18, 0)):
        wt2, bias2 = wt.clone(), bias.clone()
        wt2[second] = wt2[first]
        bias2[first] = bias2[second] = 1000.0
        m2, lab2, lg2 = tail(wt2, bias2)
        assert torch.equal(lg2[:, first], lg2[:, second])
        assert torch.equal(lab2, torch.full_like(lab2, first)) and torch.equal(m2, torch.full_like(m2, colour))
    m0, lab0, _ = tail(torch.zeros_like(wt), torch.zeros_like(bias))       # all logits equal: class 0, background
    assert int(lab0.max()) == 0 and int(m0.max()) == 0


@pytest.mark.parametrize("precision,_,tol", PRECISIONS)
@pytest.mark.parametrize("case", [0, 1, 2])
@torch.no_grad()
def test_whole_net_matches_the_reference_fp64_logits_and_masks(golden, monkeypatch, precision, _, tol, case):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    g = golden("parsenet.pt")
    ni, b, seed = g["cases"][case]
    size = g["nets"][ni][0]
    net = _net(g, ni)
    img = synth.synth_sr_input_u8(b, size, size, seed).to(DEV)
    rows, cols = torch.tensor(g[f"rows.{case}"]), torch.tensor(g[f"cols.{case}"])
    scale = g[f"scale.{case}"]
    if case == 2:                                                         # locate a failure: three places inside the full net
        taps = {}
        net.features_nhwc(img, taps=taps)
        for name in ("enc0", "trunk", "dec0"):
            rc = torch.tensor(g[f"mid_rc.{name}"])
            got = taps[name].cpu().permute(0, 3, 1, 2)[:, :, rc][:, :, :, rc].double()
            err, sc = float((got - g[f"mid.{name}"].double()).abs().max()), g[f"mid.{name}.scale"]
            print(f"{precision} {name}: err {err:.3e} = {err / sc:.2e} x scale")
            assert err <= tol * sc, (name, err, sc)
    mask, logits = net.masks_u8(img, logits=True)
    assert tuple(logits.shape) == (b, 19, size, size) and logits.dtype == torch.float32
    assert tuple(mask.shape) == (b, size, size) and mask.dtype == torch.uint8
    got = logits.cpu()[:, :, rows][:, :, :, cols].double()
    err = float((got - g[f"logits.{case}"].double()).abs().max())
    print(f"{precision} case {case}: err {err:.3e} = {err / scale:.2e} x scale (bound {tol:.0e}; reference fp32 {g[f'e32.{case}'] / scale:.2e})")
    assert err <= tol * scale, (err, scale)
    x32 = (img.cpu().permute(0, 3, 1, 2).double() / 255.0 * 2 - 1).float().to(DEV)
    assert torch.equal(net(x32), logits)                                  # forward(x) of the module is the same computation
    # masks: exact wherever the recorded fp64 margin (rounded down to the fixture's unit) exceeds 2 x bound x scale
    want, margin = unz(g[f"mask.{case}"]), unz(g[f"margin.{case}"]).double() * g["margin_unit"] * scale
    sure = margin > 2 * tol * scale
    excluded = 1.0 - float(sure.double().mean())
    m = mask.cpu()
    print(f"{precision} case {case}: mask equal on {float((m == want).double().mean()):.5f}, excluded {excluded:.4f}")
    assert excluded <= 0.01
    assert torch.equal(m[sure], want[sure])
    assert set(m.flatten().tolist()) == {0, 255}
    if case == 0:
        assert torch.equal(net.masks_u8(img.flip(-1).contiguous(), bgr=True), mask)


@torch.no_grad()
def test_batch_equals_single_calls_and_a_second_call_bitwise(golden):
    g = golden("parsenet.pt")
    net = _net(g, 0)
    imgs = synth.synth_sr_input_u8(3, 32, 32, seed=51).to(DEV)
    mask, logits = net.masks_u8(imgs, logits=True)
    mask, logits = mask.clone(), logits.clone()
    for i in range(3):
        mi, li = net.masks_u8(imgs[i:i + 1], logits=True)
        assert torch.equal(li[0], logits[i]) and torch.equal(mi[0], mask[i])
    again = net.masks_u8(imgs, logits=True)
    assert torch.equal(again[0], mask) and torch.equal(again[1], logits)


@torch.no_grad()
def test_face_parse_process_masks_and_graph_capture(golden):
    g = golden("parsenet.pt")
    fp = _face_parse(g)
    a, b = synth.synth_sr_input_u8(1, 512, 512, seed=52), synth.synth_sr_input_u8(1, 512, 512, seed=53)
    eager_a, eager_b = fp.masks(a.to(DEV)).clone(), fp.masks(b.to(DEV)).clone()
    assert tuple(eager_a.shape) == (1, 512, 512) and not torch.equal(eager_a, eager_b)
    out = fp.process(a[0].numpy())
    assert isinstance(out, list) and len(out) == 1 and out[0].dtype == np.uint8 and out[0].shape == (512, 512)
    assert np.array_equal(out[0], eager_a[0].cpu().numpy())
    assert torch.equal(fp.masks(a.flip(-1).contiguous().to(DEV), bgr=False), eager_a)
    with pytest.raises(ValueError):
        fp.masks(torch.zeros(1, 256, 256, 3, dtype=torch.uint8, device=DEV))
    static = a.to(DEV).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fp.masks(static)                                                  # warm-up: every pack and buffer exists before capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = fp.masks(static)
    for src, ref in ((b, eager_b), (a, eager_a)):
        static.copy_(src.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(res, ref)
