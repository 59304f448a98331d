"""GPU tests of the BiSeNet face parser (e4s_amd/face_parser.py, csrc/parser.hip) against the REAL reference's outputs
(tests/golden/face_parser.pt, tests/golden/make_face_parser_golden.py) and fp64 torch restatements of each new kernel."""
import pytest
import torch
import torch.nn.functional as F

from e4s_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _unz(z):
    """(zlib bytes, shape) of a uint8 fixture -> uint8 tensor."""
    import zlib
    import numpy as np
    return torch.from_numpy(np.frombuffer(zlib.decompress(z[0]), dtype=np.uint8).reshape(z[1]).copy())


def _net():
    from e4s_amd.face_parser import BiSeNet
    net = BiSeNet(19)
    net.load_state_dict(synth.synth_module_state_dict(net, tag="bisenet."), strict=True)
    return net.to(DEV).eval()


def _parser():
    from e4s_amd.face_parser import FaceParser
    fp = FaceParser(None, device="cpu")
    fp.seg.load_state_dict(synth.synth_module_state_dict(fp.seg, tag="bisenet."), strict=True)
    return fp.to(DEV)


def _full_image(g):
    """The fixture's 1024^2 uint8 NHWC image, rebuilt from its seed (make_face_parser_golden.full_image)."""
    x = synth.synth_image(1, 1024, seed=g["full_seed"], tag="bisenet.full")
    return ((x + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _images(b, size, seed):
    x = synth.synth_image(b, size, seed=seed, tag="bisenet.batch")
    return ((x + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("precision,tol", [("f32", 1e-4), ("bf16x3", 1e-3)])
@torch.no_grad()
def test_bisenet_forward_matches_the_reference_heads(golden, monkeypatch, precision, tol):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    g = golden("face_parser.pt")
    x = synth.synth_image(2, 128, seed=g["small_seed"], tag="bisenet.small")
    heads = _net()(x.to(DEV))
    idx = torch.tensor(g["sample128"])
    for got, ref in zip(heads, g["small.logits"]):
        assert tuple(got.shape) == (2, 19, 128, 128)
        got = got.cpu()[:, :, idx][:, :, :, idx].double()
        scale = float(ref.abs().max())
        err = float((got - ref.double()).abs().max())
        assert err <= tol * scale, (precision, err, scale)


@torch.no_grad()
def test_parse_full_size_matches_the_reference_labels(golden):
    from e4s_amd import kernels as K
    g = golden("face_parser.pt")
    fp = _parser()
    img = _full_image(g).to(DEV)
    pre = fp.preprocess(img)
    assert tuple(pre.shape) == (1, 512, 512, 3)
    s = torch.tensor(g["sample512"])
    pre_s = pre.cpu().permute(0, 3, 1, 2)[:, :, s][:, :, :, s]
    assert float((pre_s - g["full.pre"]).abs().max()) <= 1e-5
    low = fp.seg.main_logits_nhwc(pre)[..., :19].permute(0, 3, 1, 2).cpu().double()
    scale = g["full.scale"]
    tol = 1e-4 if K.PRECISION == "f32" else 1e-3
    assert float((low - g["full.logits64"].double()).abs().max()) <= tol * scale
    confident = _unz(g["full.margin_u8"]) > 10                    # fp64 margin > 1e-3 x scale (units of 1e-4 x scale)
    for seg12, key in ((False, "full.labels19"), (True, "full.labels12")):
        lab = fp.parse(img, seg12=seg12)
        assert lab.dtype == torch.uint8 and tuple(lab.shape) == (1, 512, 512)
        lab, ref = lab[0].cpu(), _unz(g[key])
        assert torch.equal(lab[confident], ref[confident]), key
        assert float((lab == ref).double().mean()) >= 0.999, key


@torch.no_grad()
def test_parse_onehot_is_labelmap2onehot_and_feeds_net3_identically():
    from e4s_amd import postproc
    from e4s_amd.networks import Net3
    from e4s_amd.options import make_opts
    fp = _parser()
    img = _images(1, 1024, seed=3).to(DEV)
    lab, oh = fp.parse(img, seg12=True, onehot=True)
    ref = postproc.labelMap2OneHot(lab[:, None], 12)
    assert oh.dtype == torch.float32 and tuple(oh.shape) == (1, 12, 512, 512)
    assert torch.equal(oh, ref)
    lab19, oh19 = fp.parse(img, seg12=False, onehot=True)
    assert torch.equal(oh19, postproc.labelMap2OneHot(lab19[:, None], 19))
    size = 256
    net = Net3(make_opts(out_size=size))
    net.load_state_dict(synth.synth_state_dict(size, 13), strict=True)
    net.latent_avg = synth.synth_latent_avg(size).to(DEV)
    net = net.to(DEV).eval()
    x = synth.synth_image(1, 1024, tag="smoke").to(DEV)
    sv_a, _ = net.get_style_vectors(x, oh)
    sv_b, _ = net.get_style_vectors(x, ref)
    assert torch.equal(sv_a, sv_b)


@torch.no_grad()
def test_batched_parse_equals_single_calls_for_both_input_layouts():
    fp = _parser()
    imgs = _images(3, 1024, seed=5).to(DEV)
    single = torch.cat([fp.parse(imgs[i:i + 1]) for i in range(3)])
    assert torch.equal(fp.parse(imgs), single)
    nchw = imgs.permute(0, 3, 1, 2).float().div(255).contiguous()
    assert torch.equal(fp.parse(nchw), single)
    small = _images(1, 512, seed=6).to(DEV)
    assert tuple(fp.parse(small).shape) == (1, 256, 256)


@torch.no_grad()
def test_graph_capture_of_parse_replays_bitwise():
    fp = _parser()
    a, b = _images(2, 1024, seed=7).to(DEV), _images(2, 1024, seed=8).to(DEV)
    eager_a, eager_b = fp.parse(a, onehot=True), fp.parse(b, onehot=True)
    again = fp.parse(a, onehot=True)
    assert torch.equal(eager_a[0], again[0]) and torch.equal(eager_a[1], again[1])
    static = a.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fp.parse(static, onehot=True)                            # warm-up: every pack and cached tensor exists before capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fp.parse(static, onehot=True)
    for src, ref in ((b, eager_b), (a, eager_a)):
        static.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])


# ---- per-kernel checks against fp64 torch --------------------------------------------------------------------------
def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@torch.no_grad()
def test_maxpool3s2p1_kernel():
    from e4s_amd import kernels as K
    for h, w in ((9, 12), (8, 7)):
        x = _rand(2, h, w, 8, seed=h)
        got = K.maxpool3s2p1(x.float().to(DEV)).cpu().double()
        ref = F.max_pool2d(x.float().double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        assert torch.equal(got, ref)


@torch.no_grad()
def test_gate_add_up2_and_pooled_gate_kernels():
    from e4s_amd import kernels as K
    x, gate = _rand(2, 3, 5, 16, seed=1).float(), torch.sigmoid(_rand(2, 16, seed=2)).float()
    for add in (_rand(2, 16, seed=3).float(), _rand(2, 3, 5, 16, seed=4).float()):
        got = K.gate_add_up2(x.to(DEV), gate.to(DEV), add.to(DEV)).cpu().double()
        a = add.double()[:, None, None] if add.dim() == 2 else add.double()
        ref = (x.double() * gate.double()[:, None, None] + a).repeat_interleave(2, 1).repeat_interleave(2, 2)
        assert float((got - ref).abs().max()) <= 1e-6
    feat = _rand(2, 6, 7, 40, seed=5).float()
    pooled = K.mean_hw(feat.to(DEV)).cpu().double()
    assert float((pooled - feat.double().mean((1, 2))).abs().max()) <= 1e-6
    w, b = _rand(24, 40, seed=6).float() * 0.2, _rand(24, seed=7).float()
    for act, fn in ((0, lambda t: t), (1, torch.relu), (2, torch.sigmoid)):
        got = K.parser_fc(pooled.float().to(DEV), w.to(DEV), b.to(DEV), act=act, offset=0.5).cpu().double()
        ref = fn(pooled.float().double() @ w.double().T + b.double()) + 0.5
        assert float((got - ref).abs().max()) <= 1e-5
    one_plus = K.parser_fc(gate.to(DEV), None, None, act=0, offset=1.0).cpu()
    assert torch.equal(one_plus, gate + 1.0)


@torch.no_grad()
def test_upsample_argmax_head_kernel_including_an_exact_tie():
    from e4s_amd import kernels as K
    from e4s_amd.face_parser import seg19_to_12
    lg = _rand(2, 5, 6, 32, seed=9).float()
    lg[..., 19:] = 100.0                                         # padding channels are never read
    lg[0, :, :, 7] = 50.0                                        # classes 7 and 3 tie exactly on sample 0: the lowest index wins
    lg[0, :, :, 3] = 50.0
    H, W = 33, 41
    lab, oh, nchw = K.parser_head(lg.to(DEV), 19, (H, W), labels=True, nchw=True)
    ref = F.interpolate(lg[..., :19].double().permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=True)
    assert float((nchw.cpu().double() - ref).abs().max()) <= 1e-5
    top2 = torch.topk(ref, 2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 1e-4
    lab = lab.cpu()
    ref_lab = ref.argmax(1).to(torch.uint8)
    assert torch.equal(lab[sure], ref_lab[sure])
    assert bool((lab[0] == 3).all())
    lab12, oh12, none = K.parser_head(lg.to(DEV), 19, (H, W), seg12=True, onehot=True)
    assert none is None
    assert torch.equal(lab12.cpu(), seg19_to_12(lab))
    assert torch.equal(oh12.cpu(), F.one_hot(lab12.cpu().long(), 12).permute(0, 3, 1, 2).float())


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@torch.no_grad()
def test_basic_block_residual_epilogue(monkeypatch, precision):
    """relu(shortcut + bn2(conv2(...))) of a BasicBlock: the fp32 conv's noise epilogue (f32) or e4s_add_relu_f32 after the
    split-bf16 conv (bf16x3), against fp64 torch."""
    from e4s_amd import kernels as K
    from e4s_amd.face_parser import BasicBlock, basic_block
    monkeypatch.setattr(K, "PRECISION", precision)
    for cin, cout, stride in ((64, 64, 1), (64, 128, 2)):
        blk = BasicBlock(cin, cout, stride).eval()
        blk.load_state_dict(synth.synth_module_state_dict(blk, tag=f"blk{cin}.{stride}."), strict=True)
        x = torch.relu(_rand(2, cin, 16, 16, seed=cout)).float()
        b64 = BasicBlock(cin, cout, stride).double().eval()
        b64.load_state_dict(blk.state_dict())
        r = F.relu(b64.bn1(b64.conv1(x.double())))
        r = b64.bn2(b64.conv2(r))
        sc = x.double() if b64.downsample is None else b64.downsample(x.double())
        ref = F.relu(sc + r).permute(0, 2, 3, 1)
        got = basic_block(blk.to(DEV), x.permute(0, 2, 3, 1).contiguous().to(DEV)).cpu().double()
        scale = float(ref.abs().max())
        assert float((got - ref).abs().max()) <= (1e-5 if precision == "f32" else 1e-3) * scale
    a, r = _rand(3, 5, 7, 12, seed=1).float(), _rand(3, 5, 7, 12, seed=2).float()
    got = K.add_relu(a.to(DEV), r.to(DEV)).cpu()
    assert torch.equal(got, torch.relu(a + r))
    wide = torch.zeros(3, 5, 7, 20, device=DEV)
    K.add_relu(a.to(DEV), out=wide, coff=8)
    assert torch.equal(wide[..., 8:].cpu(), torch.relu(a)) and not bool(wide[..., :8].any())
