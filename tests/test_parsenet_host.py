"""Host-side tests of GPEN's ParseNet (e4s_amd/parsenet.py): the module tree against the reference's recorded state_dict
(tests/golden/parsenet.pt), the BatchNorm fold, and what the native net refuses.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from e4s_amd import synth
from e4s_amd.parsenet import MASK_COLORMAP, ConvLayer, FaceParse, NormLayer, ParseNet, ReluLayer, ResidualBlock


def _net(size, osize, mfs, depth):
    return ParseNet(size, osize, mfs, 64, 19, res_depth=depth, norm_type="bn", relu_type="LeakyReLU", ch_range=[32, 256])


def test_state_dict_keys_and_shapes_equal_the_reference(golden):
    g = golden("parsenet.pt")
    for i, (ni, _, _) in enumerate(g["cases"]):
        with torch.device("meta"):
            net = _net(*g["nets"][ni])
        sd = net.state_dict()
        assert list(sd.keys()) == g[f"keys.{i}"]
        assert [tuple(v.shape) for v in sd.values()] == g[f"shapes.{i}"]
    assert g["keys"] == g["keys.2"] and len(g["keys"]) == 238


def test_seeded_state_dict_loads_strict_and_has_nontrivial_bn_statistics():
    net = _net(32, 32, 8, 2)
    sd = synth.synth_parsenet_state_dict(net)
    net.load_state_dict(sd, strict=True)
    bn = net.encoder[1].conv1.norm.norm
    assert float((bn.running_mean).abs().max()) > 0.01 and float((bn.running_var - 1).abs().max()) > 0.01
    assert float((bn.weight.detach() - 1).abs().max()) > 0.01
    again = synth.synth_parsenet_state_dict(_net(32, 32, 8, 2))
    assert all(torch.equal(sd[k], again[k]) for k in sd)


@pytest.mark.parametrize("scale", ["none", "down", "up"])
def test_folded_conv_layer_equals_conv_bn_leakyrelu_in_fp64(scale):
    """ConvLayer.folded() (eval-mode BatchNorm folded into weight and bias) against the unfolded layer -- nearest x2, reflect pad,
    conv, BatchNorm with running statistics, LeakyReLU(0.2) -- all in fp64: the fold is exact up to fp64 rounding."""
    g = torch.Generator().manual_seed(5)
    layer = ConvLayer(8, 16, 3, scale, norm_type="bn", relu_type="LeakyReLU").double().eval()
    bn = layer.norm.norm
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(16, generator=g, dtype=torch.float64))
        bn.bias.copy_(0.3 * torch.randn(16, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(0.5 * torch.randn(16, generator=g, dtype=torch.float64))
        bn.running_var.copy_(0.5 + torch.rand(16, generator=g, dtype=torch.float64))
    assert layer.conv2d.bias is None
    x = torch.randn(2, 8, 7, 9, generator=g, dtype=torch.float64)

    def pre(t):
        if scale == "up":
            t = F.interpolate(t, scale_factor=2, mode="nearest")
        return F.pad(t, (1, 1, 1, 1), mode="reflect")

    with torch.no_grad():
        ref = F.leaky_relu(bn(F.conv2d(pre(x), layer.conv2d.weight, None, stride=layer.stride)), 0.2)
        w, b = layer.folded()
        assert w.dtype == torch.float32                                   # the kernels' operand; compare the fp64 fold itself
        from e4s_amd.face_parser import fold_conv_bn
        w64, b64 = fold_conv_bn(layer.conv2d.weight.detach(), bn)
        got = F.leaky_relu(F.conv2d(pre(x), w64, b64, stride=layer.stride), 0.2)
    assert tuple(got.shape) == tuple(ref.shape)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float((w.double() - w64).abs().max()) <= 2.0 ** -24 * float(w64.abs().max())


def test_layer_without_norm_keeps_its_bias_and_identity_shortcut_has_no_parameters():
    layer = ConvLayer(8, 16, 3, "down")
    w, b = layer.folded()
    assert torch.equal(w, layer.conv2d.weight.detach()) and torch.equal(b, layer.conv2d.bias.detach()) and layer.stride == 2
    block = ResidualBlock(16, 16, relu_type="LeakyReLU", norm_type="bn")
    assert block.shortcut_func is None and not any(k.startswith("shortcut") for k in block.state_dict())
    assert ResidualBlock(16, 32, relu_type="LeakyReLU", norm_type="bn", scale="up").shortcut_func.conv2d.bias is not None


def test_unsupported_variants_raise():
    for norm in ("in", "gn", "pixel", "layer"):
        with pytest.raises(NotImplementedError):
            NormLayer(8, norm_type=norm)
    for relu in ("relu", "prelu", "selu"):
        with pytest.raises(NotImplementedError):
            ReluLayer(8, relu)
    with pytest.raises(NotImplementedError):
        ParseNet(32, 32, 8, 64, 19, res_depth=2)                          # the reference's default relu_type='prelu'
    with pytest.raises(NotImplementedError):
        ConvLayer(8, 8, 1)


def test_face_parse_refuses_missing_weights_other_sizes_and_cpu_tensors(monkeypatch, tmp_path):
    from e4s_amd import criteria
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", False)
    with pytest.raises(FileNotFoundError):
        FaceParse(base_dir=str(tmp_path), device="cpu")
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", True)
    fp = FaceParse(base_dir=str(tmp_path), device="cpu")
    assert fp.size == 512 and fp.MASK_COLORMAP == MASK_COLORMAP and [i for i, v in enumerate(MASK_COLORMAP) if v == 0] == [0, 14, 18]
    with pytest.raises(ValueError):
        fp.masks(torch.zeros(1, 256, 256, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        fp.process(np.zeros((256, 512, 3), dtype=np.uint8))
    with pytest.raises(RuntimeError):
        fp.masks(torch.zeros(1, 512, 512, 3, dtype=torch.uint8))         # no CPU path
    with pytest.raises(NotImplementedError):
        fp.process_tensor(torch.zeros(1, 3, 512, 512))


def test_a_real_checkpoint_layout_loads_strict(tmp_path):
    """weights/ParseNet-latest.pth is a plain state_dict (face_parsing.py:35): one saved with the fixture's keys loads."""
    (tmp_path / "weights").mkdir()
    net = _net(512, 512, 32, 10)
    sd = synth.synth_parsenet_state_dict(net)
    torch.save(sd, str(tmp_path / "weights" / "ParseNet-latest.pth"))
    fp = FaceParse(base_dir=str(tmp_path), device="cpu")
    assert torch.equal(fp.faceparse.out_mask_conv.conv2d.bias, sd["out_mask_conv.conv2d.bias"])
    assert not any(p.requires_grad for p in fp.faceparse.parameters())
