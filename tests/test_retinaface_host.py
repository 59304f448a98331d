"""Host-side checks of the RetinaFace-R50 detector (e4s_amd/retinaface.py) against tests/golden/retinaface.pt
(tests/golden/make_retinaface_golden.py): the parameter tree, the BatchNorm fold, the size arithmetic, the prior formula, argument
validation and the FaceRestorer wiring.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from e4s_amd import retinaface as R


@pytest.fixture(scope="module")
def g(golden):
    return golden("retinaface.pt")


def test_state_dict_keys_and_shapes_equal_the_reference(g):
    with torch.device("meta"):
        net = R.RetinaFace(R.cfg_re50)
    sd = net.state_dict()
    assert list(sd.keys()) == g["keys"]
    assert [tuple(v.shape) for v in sd.values()] == [tuple(s) for s in g["shapes"]]
    assert "body.conv1.weight" in sd and "body.layer4.2.bn3.running_var" in sd and "fpn.output1.0.weight" in sd
    assert "ssh1.conv3X3.0.weight" in sd and "ClassHead.0.conv1x1.weight" in sd and not any(k.startswith("body.fc") for k in sd)


def test_bn_fold_equals_conv_then_bn_in_fp64():
    from e4s_amd.face_parser import fold_conv_bn
    gen = torch.Generator().manual_seed(3)
    conv = nn.Conv2d(64, 128, 3, 2, 1, bias=False).double()
    bn = nn.BatchNorm2d(128).double().eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen, dtype=torch.float64))
        bn.weight.copy_(1 + 0.1 * torch.randn(128, generator=gen, dtype=torch.float64))
        bn.bias.copy_(torch.randn(128, generator=gen, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(128, generator=gen, dtype=torch.float64))
        bn.running_var.copy_(0.5 + torch.rand(128, generator=gen, dtype=torch.float64))
        x = torch.randn(2, 64, 9, 11, generator=gen, dtype=torch.float64)
        ref = bn(conv(x))
        w, b = fold_conv_bn(conv.weight, bn)
        got = F.conv2d(x, w, b, stride=2, padding=1)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_output_size_and_shrink_size_arithmetic(g):
    assert R.feature_sizes(*g["frame_A"][:2]) == [(38, 55), (19, 28), (10, 14), (5, 7), (3, 4)]
    assert R.feature_sizes(*g["frame_B"][:2]) == [(32, 48), (16, 24), (8, 12), (4, 6), (2, 3)]
    assert R.feature_sizes(1000, 667)[2:] == [(125, 84), (63, 42), (32, 21)]
    for h, w in (g["frame_A"][:2], g["frame_B"][:2], (1000, 43), (1000, 667)):
        # the conv maps are the grids PriorBox lays its priors on (ceil(size / step))
        assert R.feature_sizes(h, w)[2:] == [(-(-h // s), -(-w // s)) for s in (8, 16, 32)]
    assert R.shrink_size(*g["frame_A"][:2]) == (1.0, 75, 109)
    assert R.shrink_size(1500, 1500) == (1.0, 1500, 1500)
    ss, h, w = R.shrink_size(*g["frame_thin"][:2])
    assert ss == 1000.0 / 1504 and (h, w) == tuple(g["thin.size"]) == (1000, 43)
    assert R.shrink_size(64, 1504)[1:] == (43, 1000)
    from e4s_amd import kernels as K
    for n in (1, 2, 5, 7, 38, 55, 75):
        assert K.rconv_out_size(n, 1, 2) == K.rconv_out_size(n, 3, 2) == -(-n // 2)
        assert K.rconv_out_size(n, 1, 1) == K.rconv_out_size(n, 3, 1) == n


def test_prior_formula_equals_the_reference_priors_to_one_ulp(g):
    for name in ("A", "B"):
        h, w = g["frame_" + name][:2]
        ref = g[name + ".priors"].numpy()
        got = R.prior_boxes(h, w)
        assert got.shape == ref.shape and got.dtype == np.float32
        assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))
    assert R.prior_boxes(75, 109).shape == (374, 4)


def test_argument_validation():
    with pytest.raises(NotImplementedError):
        R.RetinaFaceDetection(None, device="cpu", network="mobilenet0.25")
    with pytest.raises(NotImplementedError):
        R.RetinaFace({"name": "mobilenet0.25"})
    det = R.RetinaFaceDetection(None, device="cpu")                       # conftest allows a net without a checkpoint
    with pytest.raises(NotImplementedError):
        det.detect_tensor(torch.zeros(1, 3, 8, 8))
    for bad in (torch.zeros(8, 8, 3), torch.zeros(3, 8, 8, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8),
                torch.zeros(1, 1, 8, 8, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            det.detect_device(bad)
        with pytest.raises(ValueError):
            det.raw(bad)
    with pytest.raises(RuntimeError):
        det.detect_device(torch.zeros(8, 8, 3, dtype=torch.uint8))       # a CPU frame: no CPU path
    with pytest.raises(ValueError):
        det.detect(np.zeros((8, 8, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        det.detect(np.zeros((3, 8, 8), dtype=np.uint8))


def test_module_prefix_is_removed_as_the_reference_does():
    sd = R.RetinaFaceDetection.remove_prefix({"module.body.conv1.weight": 1, "fpn.output1.0.weight": 2}, "module.")
    assert sd == {"body.conv1.weight": 1, "fpn.output1.0.weight": 2}


def test_face_restorer_without_a_detector_behaves_as_before():
    from e4s_amd.face_paste import FaceRestorer
    fr = FaceRestorer(lambda x: x, parser=None)
    assert fr.detector is None
    frame = torch.zeros(16, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):                                     # given boxes: reaches the old device check, as before
        fr.process(frame, np.zeros((0, 5)), np.zeros((0, 10)))
    with pytest.raises(RuntimeError):
        fr.process(frame)                                                 # the device check still comes first
    with pytest.raises(ValueError):
        fr.process(_FakeCuda(frame))                                      # neither boxes nor a detector
    with pytest.raises(ValueError):
        fr.process(_FakeCuda(frame), np.zeros((0, 5)))                    # boxes without landmarks


class _FakeCuda(torch.Tensor):
    """A CPU frame that claims to be on the device: enough to reach the argument checks that follow the device check."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True
