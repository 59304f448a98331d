"""Host-side checks of the face-vid2vid pose front end (e4s_amd/reenact.py) against the REAL reference's records
(tests/golden/reenact.pt, tests/golden/make_reenact_golden.py): no GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn


@pytest.fixture(scope="module")
def g(golden):
    return golden("reenact.pt")


def test_state_dict_keys_and_shapes_equal_the_reference(g):
    from e4s_amd import reenact
    with torch.device("meta"):
        nets = {"kp": reenact.KPDetector(**g["kp_shipped"]), "he": reenact.HEEstimator(**g["he_shipped"])}
    for name, net in nets.items():
        sd = net.state_dict()
        assert list(sd.keys()) == g[name + ".keys"]
        assert [tuple(v.shape) for v in sd.values()] == g[name + ".shapes"]
    assert not nets["kp"].training and not nets["he"].training
    with torch.device("meta"):
        kj = reenact.KPDetector(**dict(g["kp_shipped"], estimate_jacobian=True, single_jacobian_map=True))
    assert tuple(kj.jacobian.weight.shape) == (9, 32, 3, 3, 3)


def test_jacobian_head_is_identity_at_construction(g):
    from e4s_amd import reenact
    net = reenact.KPDetector(**g["kp_cfg"], estimate_jacobian=True)
    assert float(net.jacobian.weight.abs().max()) == 0.0
    assert net.jacobian.bias.view(15, 3, 3).eq(torch.eye(3)).all()


@pytest.mark.parametrize("dims", [2, 3])
def test_batchnorm_fold_equals_conv_then_bn_in_fp64(dims):
    from e4s_amd.reenact import fold_conv_bn_bias
    gen = torch.Generator().manual_seed(5 + dims)
    conv = (nn.Conv2d if dims == 2 else nn.Conv3d)(6, 5, 3, padding=1).double()
    bn = (nn.BatchNorm2d if dims == 2 else nn.BatchNorm3d)(5).double().eval()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(5, generator=gen, dtype=torch.float64))
        bn.bias.copy_(torch.randn(5, generator=gen, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(5, generator=gen, dtype=torch.float64))
        bn.running_var.copy_(0.5 + torch.rand(5, generator=gen, dtype=torch.float64))
        x = torch.randn(2, 6, *([4, 5, 3][:dims]), generator=gen, dtype=torch.float64)
        ref = bn(conv(x))
        w, b = fold_conv_bn_bias(conv.weight, conv.bias, bn)
        got = (F.conv2d if dims == 2 else F.conv3d)(x, w, b, padding=1)
    assert w.dtype == torch.float64
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_antialias_taps_equal_the_reference_kernel(g):
    from e4s_amd import reenact
    taps, step = reenact.antialias_taps(0.25)
    ref = g["aa.weight"].double()
    assert step == 4 and taps.shape == (13,) and tuple(ref.shape) == (13, 13)
    assert float((torch.from_numpy(np.outer(taps, taps)) - ref).abs().max()) <= 2e-7 * float(ref.max())     # the reference builds it in fp32
    assert abs(taps.sum() - 1) < 1e-15
    mine = reenact.AntiAliasInterpolation2d(3, 0.25).weight
    assert tuple(mine.shape) == (3, 1, 13, 13) and float((mine[1, 0].double() - ref).abs().max()) <= 1e-8


def test_size_arithmetic_for_odd_frames(g):
    from e4s_amd import reenact
    assert reenact.kp_map_sizes(64, 48, 0.25, 3) == [(16, 12), (8, 6), (4, 3), (2, 1)]
    assert reenact.kp_map_sizes(256, 256, 0.25, 5) == [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4), (2, 2)]
    assert reenact.kp_map_sizes(75, 61, 0.25, 2) == [(19, 16), (9, 8), (4, 4)]
    assert reenact.kp_map_sizes(75, 61, 1, 1) == [(75, 61), (37, 30)]
    with pytest.raises(ValueError):
        reenact.kp_map_sizes(16, 16, 0.25, 3)
    assert reenact.he_map_sizes(75, 61) == [(38, 31), (19, 16), (10, 8), (5, 4), (3, 2)]
    assert reenact.he_map_sizes(256, 256)[-1] == (8, 8)
    # against torch's own size arithmetic on an odd frame
    x = torch.zeros(1, 1, 75, 61)
    aa = F.conv2d(F.pad(x, (6, 6, 6, 6)), torch.zeros(1, 1, 13, 13))[:, :, ::4, ::4]
    assert tuple(aa.shape[2:]) == reenact.kp_map_sizes(75, 61, 0.25, 0)[0]
    assert tuple(F.avg_pool2d(aa, 2).shape[2:]) == reenact.kp_map_sizes(75, 61, 0.25, 1)[1]
    c1 = F.conv2d(x, torch.zeros(1, 1, 7, 7), stride=2, padding=3)
    assert [tuple(c1.shape[2:]), tuple(F.max_pool2d(c1, 3, 2, 1).shape[2:])] == reenact.he_map_sizes(75, 61)[:2]


def test_reshape_permutation_against_view():
    from e4s_amd.reenact import reshape_permutation
    gen = torch.Generator().manual_seed(3)
    b, cin, c, depth, h, w = 2, 8, 24, 4, 3, 2
    x = torch.randn(b, cin, h, w, generator=gen, dtype=torch.float64)
    wt, bias = torch.randn(c, cin, 1, 1, generator=gen, dtype=torch.float64), torch.randn(c, generator=gen, dtype=torch.float64)
    ref = F.conv2d(x, wt, bias).view(b, c // depth, depth, h, w)                                  # the reference's volume, NCDHW
    perm = reshape_permutation(c, depth)
    assert sorted(perm.tolist()) == list(range(c))
    nhwc = F.conv2d(x, wt[perm], bias[perm]).permute(0, 2, 3, 1).contiguous()                     # what the permuted 1x1 conv writes
    vol = nhwc.view(b, h, w, depth, c // depth).permute(0, 3, 1, 2, 4)                            # [B,D,h,w,C] through strides
    assert vol.stride(4) == 1 and vol.data_ptr() == nhwc.data_ptr()
    assert torch.equal(vol.permute(0, 4, 1, 2, 3), ref)
    with pytest.raises(ValueError):
        reshape_permutation(10, 4)


def test_keypoint_transformation_equals_the_recorded_cases(g):
    from e4s_amd import reenact
    assert len(g["kt"]) >= 6
    for case in g["kt"]:
        he_in = {k: v.clone() for k, v in case["he"].items()}
        got = reenact.keypoint_transformation(case["kp"], he_in, **case["kwargs"])
        assert float((got["value"] - case["value"]).abs().max()) <= 1e-12, case["name"]
        if case["jacobian"] is None:
            assert got["jacobian"] is None
        else:
            assert float((got["jacobian"] - case["jacobian"]).abs().max()) <= 1e-12, case["name"]
        assert all(torch.equal(he_in[k], case["he"][k]) for k in he_in), "the arguments are left alone"
        reenact.keypoint_transformation(case["kp"], he_in, **case["kwargs"])                     # a second call with the same dict works
    r = g["rot"]
    assert float((reenact.get_rotation_matrix(r["yaw"], r["pitch"], r["roll"]) - r["mat"]).abs().max()) <= 1e-12
    # the kept quirks: pi is 3.14, and the product is pitch . yaw . roll
    m = reenact.get_rotation_matrix(torch.tensor([180.0], dtype=torch.float64), torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))
    assert abs(float(m[0, 0, 0]) - np.cos(3.14)) < 1e-15 and float(m[0, 0, 0]) != -1.0
    deg = reenact.headpose_pred_to_degree(g["he.B.yaw"])
    assert float((deg - g["he.B.degrees"][:, 0]).abs().max()) <= 1e-12


def test_argument_validation(g):
    from e4s_amd import reenact
    with pytest.raises(NotImplementedError):
        reenact.KPDetector(**dict(g["kp_cfg"], image_channel=1))
    with pytest.raises(ValueError):
        reenact.KPDetector(**dict(g["kp_cfg"], reshape_channel=1024))                            # 1024 / 4 is not the first up block's 128
    with pytest.raises(NotImplementedError):
        reenact.HEEstimator(block_expansion=48, feature_channel=32, num_kp=15, image_channel=3, max_features=2048)
    kp = reenact.KPDetector(**g["kp_cfg"], estimate_jacobian=False)
    he = reenact.HEEstimator(block_expansion=64, feature_channel=32, num_kp=15, image_channel=3, max_features=2048)
    for net in (kp, he):
        assert not net.training
        with pytest.raises(RuntimeError):
            net.train()
        assert net.eval() is net
        with pytest.raises(NotImplementedError):
            net(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        reenact.PoseFrontEnd(kp, he, estimate_jacobian=True)                                     # the detector has no jacobian head
    with pytest.raises(TypeError):
        reenact.PoseFrontEnd(nn.Identity(), he, False)
    with pytest.raises(ValueError):
        reenact.PoseFrontEnd(kp, reenact.HEEstimator(64, 32, 10, 3, 2048), False)                # num_kp differs
    with pytest.raises(ValueError):
        reenact.PoseFrontEnd(kp, reenact.HEEstimator(64, 32, 15, 3, 2048, num_bins=60), False)
    fe = reenact.PoseFrontEnd(kp, he, False)
    with pytest.raises(RuntimeError):
        fe.head_pose_device(torch.zeros(8, 8, 3))                                                # a CPU tensor: there is no CPU path
    with pytest.raises(RuntimeError):
        kp.run(torch.zeros(1, 8, 8, 3))
    with pytest.raises(ValueError):
        reenact._frames(torch.zeros(8, 8, 4), "cpu", "t")
    with pytest.raises(ValueError):
        reenact._frames(torch.zeros(8, 8, 3, dtype=torch.int32), "cpu", "t")
    assert tuple(reenact._frames(np.zeros((5, 4, 3), np.float64), "cpu", "t").shape) == (1, 5, 4, 3)
    assert reenact._frames([np.zeros((5, 4, 3), np.uint8)] * 2, "cpu", "t").dtype == torch.uint8


def test_refuses_to_run_without_weights(g, monkeypatch):
    from e4s_amd import criteria, reenact
    kp = reenact.KPDetector(**g["kp_cfg"])
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", False)
    with pytest.raises(RuntimeError, match="no weights"):
        kp._require_weights()
    kp.load_state_dict(kp.state_dict())
    kp._require_weights()


def test_synthetic_state_dict_is_seeded_and_loads(g):
    from e4s_amd import reenact, synth
    kp = reenact.KPDetector(**g["kp_cfg"], estimate_jacobian=True)
    sd = synth.synth_vid2vid_state_dict(kp, seed=g["kp_seed"])
    kp.load_state_dict(sd, strict=True)
    again = synth.synth_vid2vid_state_dict(reenact.KPDetector(**g["kp_cfg"], estimate_jacobian=True), seed=g["kp_seed"])
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert float(sd["jacobian.weight"].abs().max()) > 0
    assert not torch.equal(sd["kp.weight"], synth.synth_vid2vid_state_dict(kp, seed=g["kp_seed"] + 1)["kp.weight"])
