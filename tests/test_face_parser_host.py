"""CPU tests of the BiSeNet face parser's host side (e4s_amd/face_parser.py) against the reference's recorded values
(tests/golden/face_parser.pt, written by tests/golden/make_face_parser_golden.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from e4s_amd import synth


def test_state_dict_keys_and_shapes_match_the_reference(golden):
    from e4s_amd.face_parser import BiSeNet
    g = golden("face_parser.pt")
    sd = BiSeNet(19).state_dict()
    assert list(sd.keys()) == g["keys"]
    assert [tuple(v.shape) for v in sd.values()] == [tuple(s) for s in g["shapes"]]
    # the seeded weights the GPU tests load are keyed on those names
    net = BiSeNet(19)
    net.load_state_dict(synth.synth_module_state_dict(net, tag="bisenet."), strict=True)


def test_seg19_to_12_table_matches_the_reference(golden):
    from e4s_amd.face_parser import SEG19_TO_12, seg19_to_12
    g = golden("face_parser.pt")
    assert torch.equal(torch.tensor(SEG19_TO_12, dtype=torch.uint8), g["seg12_of_arange19"])
    assert np.array_equal(seg19_to_12(np.arange(19)), g["seg12_of_arange19"].numpy())
    assert torch.equal(seg19_to_12(torch.arange(19)), g["seg12_of_arange19"])


def test_bicubic_taps_equal_the_reference_filter(golden):
    from e4s_amd.face_parser import bicubic_taps
    g = golden("face_parser.pt")
    assert torch.equal(bicubic_taps(2), g["taps"])
    assert abs(float(bicubic_taps(2).sum()) - 1.0) < 1e-6


def test_bn_fold_equals_conv_then_batchnorm_in_fp64():
    from e4s_amd.face_parser import ConvBNReLU, fold_conv_bn
    m = ConvBNReLU(16, 24, ks=3).double().eval()
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        m.conv.weight.copy_(torch.randn(m.conv.weight.shape, generator=gen, dtype=torch.float64) * 0.2)
        m.bn.weight.copy_(1 + 0.1 * torch.randn(24, generator=gen, dtype=torch.float64))
        m.bn.bias.copy_(0.1 * torch.randn(24, generator=gen, dtype=torch.float64))
        m.bn.running_mean.copy_(0.1 * torch.randn(24, generator=gen, dtype=torch.float64))
        m.bn.running_var.copy_(0.75 + 0.5 * torch.rand(24, generator=gen, dtype=torch.float64))
        x = torch.randn(2, 16, 9, 11, generator=gen, dtype=torch.float64)
        ref = m.bn(m.conv(x))
        w, b = fold_conv_bn(m.conv.weight, m.bn)
        got = F.conv2d(x, w, b, padding=1)
    assert float((got - ref).abs().max()) < 1e-12


def test_parse_size_is_half_the_input_and_small_inputs_are_refused():
    from e4s_amd.face_parser import parse_size
    assert parse_size(1024, 1024) == (512, 512)
    assert parse_size(512, 512) == (256, 256)
    with pytest.raises(ValueError, match="below 512"):
        parse_size(256, 256)
    with pytest.raises(ValueError, match="below 512"):
        parse_size(511, 1024)


def test_preprocess_refuses_small_inputs_before_any_device_work():
    from e4s_amd.face_parser import FaceParser
    fp = FaceParser(None, device="cpu")
    with pytest.raises(ValueError, match="below 512"):
        fp.preprocess(torch.zeros(1, 256, 256, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="below 512"):
        fp.preprocess(torch.zeros(1, 3, 300, 300))


def test_construction_without_weights_raises_unless_allowed(monkeypatch, tmp_path):
    from e4s_amd import criteria
    from e4s_amd.face_parser import BiSeNet, FaceParser
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", False)
    with pytest.raises(FileNotFoundError, match="FaceParser"):
        FaceParser(str(tmp_path / "79999_iter.pth"), device="cpu")
    with pytest.raises(FileNotFoundError):
        FaceParser(None, device="cpu")
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", True)
    FaceParser(None, device="cpu")
    # a checkpoint that exists loads with strict=True, whatever the switch says
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", False)
    net = BiSeNet(19)
    sd = synth.synth_module_state_dict(net, tag="bisenet.")
    torch.save(sd, tmp_path / "ckpt.pth")
    fp = FaceParser(str(tmp_path / "ckpt.pth"), device="cpu")
    assert torch.equal(fp.seg.state_dict()["conv_out.conv_out.weight"], sd["conv_out.conv_out.weight"])
