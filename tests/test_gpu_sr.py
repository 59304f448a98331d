"""GPU tests of the Real-ESRNet x4 super-resolution (e4s_amd/sr.py, csrc/rrdb.hip) against the REAL reference's fp64 outputs
(tests/golden/sr.pt, tests/golden/make_sr_golden.py) and fp64 torch restatements of the dense-block conv.

Bounds: a single conv / one dense block / one RRDB 1e-5 x scale (f32) and 1e-3 x scale (bf16x3), the bounds of
test_gpu_face_parser.test_basic_block_residual_epilogue; the whole network 1e-4 x scale (f32) and 1e-3 x scale (bf16x3), the
parser's whole-network bounds (the reference's own fp32 forward lies ~1e-6 x scale from its fp64 forward: sr.pt e32.*)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from e4s_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = [("f32", 1e-5, 1e-4), ("bf16x3", 1e-3, 1e-3)]                 # (PRECISION, single-layer bound, whole-network bound)
SENTINEL = 12345.0

_NETS = {}


def _net():
    """The seeded RRDBNet on the device (one per session: the weight packs are keyed on the precision)."""
    from e4s_amd.sr import RRDBNet
    if "net" not in _NETS:
        net = RRDBNet(3, 3, scale=4, num_feat=32, num_block=23, num_grow_ch=32)
        net.load_state_dict(synth.synth_rrdb_state_dict(net), strict=True)
        _NETS["net"] = net.to(DEV).eval()
    return _NETS["net"]


def _sr():
    from e4s_amd.sr import RealESRNet
    sr = RealESRNet(device=DEV)
    sr.srmodel = _net()
    return sr


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def _conv64(x_nhwc, w, b, up2=False):
    """fp64 reference: NHWC fp32 values -> NHWC fp64 conv (nearest x2 first with up2)."""
    x = x_nhwc.double().permute(0, 3, 1, 2)
    if up2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, w.double(), b.double(), padding=1).permute(0, 2, 3, 1)


def _err(got, ref, tol, what):
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max())
    print(f"{what}: err {err:.3e} = {err / scale:.2e} x scale (bound {tol:.0e})")
    assert err <= tol * scale, (what, err, scale)


@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
@pytest.mark.parametrize("shape", [(2, 9, 13), (1, 33, 50)])
@torch.no_grad()
def test_dense_conv_reads_a_channel_prefix_and_writes_a_channel_slice(monkeypatch, precision, tol, _, shape):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    b, h, w = shape
    for cin in (32, 64, 96, 128, 160):
        buf = _rand(b, h, w, 160, seed=cin)
        buf[..., cin:] = SENTINEL
        wt, bias = _rand(32, cin, 3, 3, seed=cin + 1) / (9 * cin) ** 0.5, _rand(32, seed=cin + 2)
        ref = F.leaky_relu(_conv64(buf[..., :cin], wt, bias), 0.2)
        dbuf = buf.to(DEV)
        pack = K.rrdb_pack(wt.to(DEV), K.sr_f32())
        if cin < 160:
            out, coff = dbuf, cin
            before = buf
        else:
            before = torch.full((b, h, w, 96), SENTINEL)
            out, coff = before.to(DEV), 32
        K.rrdb_conv(dbuf, cin, pack, bias.to(DEV), out, coff, epilogue=0)
        got = out.cpu()
        _err(got[..., coff:coff + 32], ref, tol, f"{precision} cin {cin} {shape}")
        keep = torch.ones(got.shape[-1], dtype=torch.bool)
        keep[coff:coff + 32] = False
        assert torch.equal(got[..., keep], before[..., keep])            # nothing outside the slice is touched
        if cin == 160:
            assert torch.equal(dbuf.cpu(), buf)


@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
@torch.no_grad()
def test_dense_conv_epilogues_and_folded_nearest_upsampling(monkeypatch, precision, tol, _):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    b, h, w = 2, 9, 13
    x = _rand(b, h, w, 160, seed=1)
    wt, bias = _rand(32, 160, 3, 3, seed=2) / (9 * 160) ** 0.5, _rand(32, seed=3)
    pack = K.rrdb_pack(wt.to(DEV), K.sr_f32())
    conv = _conv64(x, wt, bias)
    outer = _rand(b, h, w, 64, seed=4)
    # (b) x5 * 0.2 + x, r0 = the input buffer's own first 32 channels
    y = torch.full((b, h, w, 32), SENTINEL).to(DEV)
    K.rrdb_conv(x.to(DEV), 160, pack, bias.to(DEV), y, 0, epilogue=1, r0=x.to(DEV), s0=0.2)
    _err(y.cpu(), conv * 0.2 + x[..., :32].double(), tol, f"{precision} epilogue b")
    # (c) (x5 * 0.2 + x) * 0.2 + outer, written over the slice of `outer` it reads
    o = outer.to(DEV)
    K.rrdb_conv(x.to(DEV), 160, pack, bias.to(DEV), o, 32, epilogue=2, r0=x.to(DEV), s0=0.2, r1=o, r1_coff=32, s1=0.2)
    _err(o.cpu()[..., 32:], (conv * 0.2 + x[..., :32].double()) * 0.2 + outer[..., 32:].double(), tol, f"{precision} epilogue c")
    assert torch.equal(o.cpu()[..., :32], outer[..., :32])
    # (b) with s0 = 1: feat + conv_body(...)
    w32 = _rand(32, 32, 3, 3, seed=5) / (9 * 32) ** 0.5
    pack32 = K.rrdb_pack(w32.to(DEV), K.sr_f32())
    feat = _rand(b, h, w, 32, seed=6)
    y = torch.empty(b, h, w, 32, device=DEV)
    K.rrdb_conv(x.to(DEV), 32, pack32, bias.to(DEV), y, 0, epilogue=1, r0=feat.to(DEV), s0=1.0)
    _err(y.cpu(), _conv64(x[..., :32], w32, bias) + feat.double(), tol, f"{precision} skip")
    # up2: F.interpolate(nearest, 2) then the conv, on odd sizes and more than one tile
    for hh, ww in ((9, 13), (5, 1)):
        xs = _rand(b, hh, ww, 160, seed=7)
        xs[..., 32:] = SENTINEL
        y = torch.empty(b, 2 * hh, 2 * ww, 32, device=DEV)
        K.rrdb_conv(xs.to(DEV), 32, pack32, bias.to(DEV), y, 0, epilogue=0, up2=True)
        _err(y.cpu(), F.leaky_relu(_conv64(xs[..., :32], w32, bias, up2=True), 0.2), tol, f"{precision} up2 {hh}x{ww}")
    # refused: conv5 / an up-conv into the buffer it reads, an output slice inside the channels read
    xd = x.to(DEV)
    with pytest.raises(RuntimeError):
        K.rrdb_conv(xd, 160, pack, bias.to(DEV), xd, 128, epilogue=0)
    with pytest.raises(RuntimeError):
        K.rrdb_conv(xd, 64, pack, bias.to(DEV), xd, 32, epilogue=0)
    assert torch.equal(xd.cpu(), x)


@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
@torch.no_grad()
def test_one_dense_block_and_one_rrdb_match_the_reference_intermediates(golden, monkeypatch, precision, tol, _):
    from e4s_amd import kernels as K
    from e4s_amd.sr import _packed_small, dense_block, rrdb
    monkeypatch.setattr(K, "PRECISION", precision)
    g = golden("sr.pt")
    b, h, w, seed = g["cases"][1]
    net = _net()
    img = synth.synth_sr_input_u8(b, h, w, seed).to(DEV)
    rows, cols = torch.tensor(g["mid_rows"]), torch.tensor(g["mid_cols"])
    ws = net.workspace(b, h, w, img.device)
    wp, bias = _packed_small(net.conv_first)

    def sampled(t):
        return t[..., :32].cpu().permute(0, 3, 1, 2)[:, :, rows][:, :, :, cols].double()

    def check(got, name):
        err = float((got - g[f"mid.{name}"].double()).abs().max())
        scale = g[f"mid.{name}.scale"]
        print(f"{precision} {name}: err {err:.3e} = {err / scale:.2e} x scale")
        assert err <= tol * scale, (name, err, scale)

    K.rrdb_head(img, wp, bias, ws["a"], ws["feat"])
    dense_block(net.body[0].rdb1, ws["a"], ws["b"])
    check(sampled(ws["b"]), "rdb1")
    K.rrdb_head(img, wp, bias, ws["a"], ws["feat"])
    rrdb(net.body[0], ws["a"], ws["b"], ws["c"])
    check(sampled(ws["a"]), "rrdb")


@pytest.mark.parametrize("precision,_,tol", PRECISIONS)
@pytest.mark.parametrize("case", [0, 1, 2])
@torch.no_grad()
def test_whole_net_matches_the_reference_fp64_forward_float_and_uint8(golden, monkeypatch, precision, _, tol, case):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    g = golden("sr.pt")
    b, h, w, seed = g["cases"][case]
    net, sr = _net(), _sr()
    img = synth.synth_sr_input_u8(b, h, w, seed).to(DEV)
    ref, scale = g[f"y.{case}"].double(), g[f"scale.{case}"]
    full = h * w <= 64 * 64
    s = torch.tensor(g["sample_out"])

    def sampled(t):                                                      # NCHW on the host -> the recorded positions
        return t if full else t[:, :, s][:, :, :, s]

    if case == 1:                                                        # locate a failure: the trunk before the upsampling tail
        net.features_nhwc(img)
        rows, cols = torch.tensor(g["mid_rows"]), torch.tensor(g["mid_cols"])
        trunk = net.workspace(b, h, w, img.device)["b"][..., :32].cpu().permute(0, 3, 1, 2)[:, :, rows][:, :, :, cols].double()
        terr = float((trunk - g["mid.trunk"].double()).abs().max())
        print(f"{precision} trunk: err {terr:.3e} = {terr / g['mid.trunk.scale']:.2e} x scale")
        assert terr <= tol * g["mid.trunk.scale"]
    y = net(img.permute(0, 3, 1, 2).float().div(255).contiguous())
    assert tuple(y.shape) == (b, 3, 4 * h, 4 * w) and y.dtype == torch.float32
    got = sampled(y.cpu()).double()
    err = float((got - ref).abs().max())
    print(f"{precision} {b}x{h}x{w}: err {err:.3e} = {err / scale:.2e} x scale (bound {tol:.0e}; reference fp32 {g[f'e32.{case}'] / scale:.2e})")
    assert err <= tol * scale, (err, scale)
    # uint8: real_esrnet.py:53-55 on the fp64 output
    out = sr.upscale(img)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (b, 4 * h, 4 * w, 3)
    u8 = sampled(out.cpu().permute(0, 3, 1, 2)).to(torch.int32)
    levels = 255.0 * ref.clamp(0, 1)
    want = torch.round(levels).to(torch.int32)                           # half to even, as numpy.round
    assert int((u8 - want).abs().max()) <= 1
    # exact wherever the fp64 value is further from a rounding boundary k + 0.5 than the float bound allows an output to move
    # (+ the fixture's fp32 storage rounding of the fp64 value)
    margin = 255.0 * (tol + 2.0 ** -23) * scale
    sure = ((levels - torch.floor(levels)) - 0.5).abs() > margin
    share = float(sure.double().mean())
    print(f"{precision} {b}x{h}x{w}: uint8 exact on {float((u8 == want).double().mean()):.4f}, required on {share:.3f} (margin {margin:.3f} levels)")
    assert share >= 0.40
    assert torch.equal(u8[sure], want[sure])
    if case == 0:
        flipped = sr.upscale(img.flip(-1).contiguous(), bgr=True)
        assert torch.equal(flipped.flip(-1), out)


@torch.no_grad()
def test_tail_rounds_half_to_even_like_numpy_and_flips_channels():
    from e4s_amd import kernels as K
    k = np.arange(-2, 258, dtype=np.float32)
    half = (k + np.float32(0.5)) / np.float32(255)
    v = np.concatenate([half, np.nextafter(half, np.float32(9)), np.nextafter(half, np.float32(-9)), k / np.float32(255),
                        np.array([0.5, 1.5, 2.5, 253.5, 254.5], dtype=np.float32) / np.float32(255)]).astype(np.float32)
    n = v.size
    x = torch.zeros(1, 1, n, 32)
    x[0, 0, :, 0] = torch.from_numpy(v)
    wp = torch.zeros(9, 3, 32)
    wp[4, :, 0] = torch.tensor([1.0, 0.5, 0.25])                          # centre tap: channel o = v * 2^-o exactly
    bias = torch.zeros(3)
    u8 = K.rrdb_tail(x.to(DEV), wp.to(DEV), bias.to(DEV), u8=True).cpu().numpy()[0, 0]
    for o, f in enumerate((1.0, 0.5, 0.25)):
        val = (v * np.float32(f)).astype(np.float32)
        ref = (np.clip(val, 0, 1) * 255.0).round().astype(np.uint8)       # real_esrnet.py:53-55
        assert np.array_equal(u8[:, o], ref), o
    fl = K.rrdb_tail(x.to(DEV), wp.to(DEV), bias.to(DEV), u8=True, flip=True).cpu().numpy()[0, 0]
    assert np.array_equal(fl[:, ::-1], u8)
    yf = K.rrdb_tail(x.to(DEV), wp.to(DEV), bias.to(DEV), nchw=True).cpu()
    assert torch.equal(yf[0, 0, 0], torch.from_numpy(v)) and tuple(yf.shape) == (1, 3, 1, n)
    assert torch.equal(K.rrdb_tail(x.to(DEV), wp.to(DEV), bias.to(DEV), nchw=False).cpu().permute(0, 3, 1, 2), yf)


@torch.no_grad()
def test_batch_equals_single_calls_and_a_second_call_bitwise():
    sr = _sr()
    imgs = synth.synth_sr_input_u8(3, 17, 23, seed=31).to(DEV)
    batch = sr.upscale(imgs)
    single = torch.cat([sr.upscale(imgs[i:i + 1]) for i in range(3)])
    assert torch.equal(batch, single)
    assert torch.equal(sr.upscale(imgs), batch)
    x = imgs.permute(0, 3, 1, 2).float().div(255).contiguous()
    y = sr.srmodel(x)
    assert torch.equal(torch.cat([sr.srmodel(x[i:i + 1]) for i in range(3)]), y)


@torch.no_grad()
def test_graph_capture_of_upscale_replays_bitwise():
    sr = _sr()
    a, b = synth.synth_sr_input_u8(2, 24, 40, seed=32).to(DEV), synth.synth_sr_input_u8(2, 24, 40, seed=33).to(DEV)
    eager_a, eager_b = sr.upscale(a), sr.upscale(b)
    static = a.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sr.upscale(static)                                               # warm-up: every pack and buffer exists before capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sr.upscale(static)
    for src, ref in ((b, eager_b), (a, eager_a)):
        static.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)


@torch.no_grad()
def test_process_is_upscale_on_the_same_pixels():
    sr = _sr()
    img = synth.synth_sr_input_u8(1, 20, 28, seed=34)
    got = sr.process(img[0].numpy())
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (80, 112, 3)
    assert np.array_equal(got, sr.upscale(img.to(DEV), bgr=True)[0].cpu().numpy())
    with pytest.raises(RuntimeError):
        sr.upscale(img)                                                  # a CPU tensor: no CPU path
