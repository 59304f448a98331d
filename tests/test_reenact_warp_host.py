"""Host checks of face-vid2vid's dense motion and feature warp (e4s_amd/reenact_warp.py): the parameter trees against the reference's
recorded shipped state_dicts (tests/golden/reenact_warp.pt), the checkpoint loader, the host helpers against small fp64 torch
computations, and the refusals.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from e4s_amd import reenact_warp as rw, synth


@pytest.fixture(scope="module")
def g(golden):
    return golden("reenact_warp.pt")


def _reduced(g):
    net = rw.FeatureWarp(**g["gen_cfg"])
    net.load_generator_state_dict(synth.synth_vid2vid_generator_state_dict(net, seed=g["gen_seed"]))
    return net


def test_parameter_trees_equal_the_references_at_the_shipped_sizes(g):
    with torch.device("meta"):
        gen = rw.FeatureWarp(**g["gen_shipped"])
    ref = {k: s for k, s in zip(g["gen.keys"], g["gen.shapes"]) if not k.startswith("decoder.")}
    assert any(k.startswith("decoder.") for k in g["gen.keys"])
    assert {k: tuple(v.shape) for k, v in gen.state_dict().items()} == ref
    assert list(gen.state_dict().keys()) == list(ref.keys())
    dm = {k: tuple(v.shape) for k, v in gen.dense_motion_network.state_dict().items()}
    assert dm == dict(zip(g["dm.keys"], g["dm.shapes"]))
    for key in ("hourglass.encoder.down_blocks.0.conv.weight", "hourglass.decoder.up_blocks.4.norm.running_var", "hourglass.decoder.conv.weight",
                "mask.weight", "compress.weight", "norm.weight", "occlusion.bias"):
        assert key in dm, key
    assert dm["hourglass.encoder.down_blocks.0.conv.weight"] == (64, 80, 3, 3, 3) and dm["mask.weight"] == (16, 112, 7, 7, 7)
    assert dm["occlusion.weight"] == (1, 112 * 16, 7, 7)


def test_load_generator_state_dict_ignores_the_decoder_and_is_strict_elsewhere(g, monkeypatch):
    from e4s_amd import criteria
    net = rw.FeatureWarp(**g["gen_cfg"])
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", False)
    with pytest.raises(RuntimeError, match="no weights were loaded"):
        net._require_weights()
    with pytest.raises(RuntimeError, match="no weights were loaded"):
        net.dense_motion_network._require_weights()
    sd = synth.synth_vid2vid_generator_state_dict(net, seed=3)
    with_decoder = dict(sd)
    with_decoder["decoder.fc.weight"] = torch.zeros(4, 4)
    with_decoder["decoder.G_middle_0.norm_0.mlp_gamma.bias"] = torch.zeros(7)
    net.load_generator_state_dict(with_decoder)
    net._require_weights()
    net.dense_motion_network._require_weights()                              # loaded through its parent
    assert torch.equal(net.third.conv.weight, sd["third.conv.weight"])
    assert torch.equal(net.dense_motion_network.mask.bias, sd["dense_motion_network.mask.bias"])
    missing = {k: v for k, v in with_decoder.items() if k != "fourth.bias"}
    with pytest.raises(RuntimeError, match="fourth.bias"):
        net.load_generator_state_dict(missing)
    extra = dict(with_decoder)
    extra["fifth.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="fifth.weight"):
        net.load_generator_state_dict(extra)
    # the dense motion network's own loader marks it loaded as well
    dm = rw.DenseMotionNetwork(num_kp=15, feature_channel=32, estimate_occlusion_map=True, **g["gen_cfg"]["dense_motion_params"])
    dm.load_state_dict({k[len("dense_motion_network."):]: v for k, v in sd.items() if k.startswith("dense_motion_network.")}, strict=True)
    dm._require_weights()


def test_synthetic_weights_are_chosen_by_key_and_shape(g):
    a, b = rw.FeatureWarp(**g["gen_cfg"]), rw.FeatureWarp(**g["gen_cfg"])
    sa, sb = synth.synth_vid2vid_generator_state_dict(a, seed=5), synth.synth_vid2vid_generator_state_dict(b, seed=5)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    other = synth.synth_vid2vid_generator_state_dict(a, seed=6)
    assert not torch.equal(sa["first.conv.weight"], other["first.conv.weight"])
    assert abs(float(sa["dense_motion_network.occlusion.weight"].mean())) < 1e-6


def test_third_input_permutation_undoes_the_view_of_the_warped_volume():
    c, d, h, w = 8, 4, 3, 5
    gen = torch.Generator().manual_seed(1)
    vol = torch.randn(2, c, d, h, w, generator=gen, dtype=torch.float64)          # the reference's warped volume
    weight = torch.randn(6, c * d, 3, 3, generator=gen, dtype=torch.float64)
    ref = F.conv2d(vol.view(2, c * d, h, w), weight, padding=1)
    perm = rw.third_input_permutation(c, d)
    ours = vol.permute(0, 3, 4, 2, 1).reshape(2, h, w, d * c)                     # what e4s_warp3d_f32 writes: channel d * C + c
    got = F.conv2d(ours.permute(0, 3, 1, 2), weight[:, perm], padding=1)
    assert torch.equal(perm, torch.tensor([ci * d + di for di in range(d) for ci in range(c)]))
    assert float((got - ref).abs().max()) < 1e-12
    # `second`'s output permutation: the NHWC result read as [B,D,h,w,C] is the reference's .view(bs, C, D, h, w)
    from e4s_amd.reenact import reshape_permutation
    x = torch.randn(2, c * d, h, w, generator=gen, dtype=torch.float64)
    p2 = reshape_permutation(c * d, d)
    assert torch.equal(x[:, p2].permute(0, 2, 3, 1).reshape(2, h, w, d, c).permute(0, 4, 3, 1, 2), x.view(2, c, d, h, w))


def test_hourglass_layout_and_map_sizes():
    lay = rw.hourglass_layout(32, 80, 5, 1024)                                   # the shipped dense motion network
    assert [(lv["up"], lv["skip"], lv["stride"], lv["skip_read"]) for lv in lay["levels"]] == \
        [(32, 80, 128, 96), (64, 64, 128, 64), (128, 128, 256, 128), (256, 256, 512, 256), (512, 512, 1024, 512)]
    assert lay["bottom"] == 1024
    with torch.device("meta"):
        hg = rw.Hourglass(32, 80, 5, 1024)
    for i, lv in enumerate(lay["levels"]):
        up = hg.decoder.up_blocks[len(lay["levels"]) - 1 - i]
        assert up.conv.out_channels == lv["up"] and hg.encoder.down_blocks[i].conv.in_channels == lv["skip"]
        assert lv["up"] % 32 == 0 and lv["up"] + lv["skip_read"] <= lv["stride"]          # the padded read stays inside the buffer
        consumer = hg.decoder.conv if i == 0 else hg.decoder.up_blocks[len(lay["levels"]) - i]
        assert (consumer.conv if hasattr(consumer, "conv") else consumer).in_channels == lv["up"] + lv["skip"]
    assert hg.decoder.conv.in_channels == 112 == hg.out_filters
    lay2 = rw.hourglass_layout(32, 80, 2, 128)                                   # the reduced one: max_features caps the widths
    assert [(lv["up"], lv["skip"], lv["stride"]) for lv in lay2["levels"]] == [(32, 80, 128), (64, 64, 128)] and lay2["bottom"] == 128
    assert rw.hourglass_map_sizes(64, 64, 5) == [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4), (2, 2)]
    assert rw.hourglass_map_sizes(16, 12, 2) == [(16, 12), (8, 6), (4, 3)]
    with pytest.raises(ValueError, match="does not halve"):
        rw.hourglass_map_sizes(16, 12, 3)
    assert rw.encoder_map_sizes(256, 256, 2) == [(256, 256), (128, 128), (64, 64)]
    assert rw.encoder_map_sizes(75, 61, 2) == [(75, 61), (37, 30), (18, 15)]     # AvgPool2d(2) floors
    x = torch.zeros(1, 1, 75, 61)
    assert tuple(F.avg_pool2d(F.avg_pool2d(x, 2), 2).shape[2:]) == (18, 15)
    assert rw.pad32(80) == 96 and rw.pad32(112) == 128 and rw.pad32(64) == 64


def test_inverse3x3_matches_torch_inverse():
    gen = torch.Generator().manual_seed(2)
    m = torch.eye(3, dtype=torch.float64) + 0.2 * torch.randn(2, 15, 3, 3, generator=gen, dtype=torch.float64)
    assert float((rw.inverse3x3(m) - torch.inverse(m)).abs().max()) < 1e-12
    assert float((rw.inverse3x3(m) @ m - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12


def test_train_and_forward_are_refused(g):
    net = _reduced(g)
    assert not net.training and not net.dense_motion_network.training
    with pytest.raises(RuntimeError, match="inference only"):
        net.train()
    with pytest.raises(RuntimeError, match="inference only"):
        net.dense_motion_network.train()
    net.eval()
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 3, 64, 48))
    with pytest.raises(RuntimeError, match="device frames only"):
        net.encode_source(torch.zeros(64, 48, 3))                               # there is no CPU path


def test_unsupported_configurations_are_named(g):
    cfg = dict(g["gen_cfg"])
    dmp = dict(cfg["dense_motion_params"])
    with pytest.raises(NotImplementedError, match="compress = 4"):
        rw.FeatureWarp(**{**cfg, "dense_motion_params": {**dmp, "compress": 8}})
    with pytest.raises(NotImplementedError, match="dense_motion_params"):
        rw.FeatureWarp(**{**cfg, "dense_motion_params": None})
    with pytest.raises(NotImplementedError, match="3-channel"):
        rw.FeatureWarp(**{**cfg, "image_channel": 1})
    with pytest.raises(NotImplementedError, match="at most 31 keypoints"):
        rw.DenseMotionNetwork(num_kp=32, feature_channel=32, **dmp)
    with pytest.raises(NotImplementedError, match="32 k"):
        rw.DenseMotionNetwork(num_kp=15, feature_channel=32, **{**dmp, "block_expansion": 24})
    with pytest.raises(NotImplementedError, match="64 j"):
        rw.FeatureWarp(**{**cfg, "block_expansion": 16, "max_features": 128})
    with pytest.raises(ValueError, match="max_features"):
        rw.FeatureWarp(**{**cfg, "reshape_depth": 8})
    with pytest.raises(TypeError):
        rw.ReenactWarp(object(), _reduced(g))
    # keypoint dicts: a list of per-frame dicts or one batched dict; mixed jacobians are an error
    kp = lambda n, jac: {"value": torch.zeros(n, 15, 3), "jacobian": torch.zeros(n, 15, 3, 3) if jac else None}
    sv, sj, dv, dj = rw._kp_batch(kp(1, True), [kp(1, True), kp(1, True)], 15, "t")
    assert tuple(dv.shape) == (2, 15, 3) and tuple(dj.shape) == (2, 15, 3, 3) and tuple(sj.shape) == (1, 15, 3, 3)
    sv, sj, dv, dj = rw._kp_batch(kp(1, False), kp(3, False), 15, "t")
    assert tuple(dv.shape) == (3, 15, 3) and sj is None and dj is None
    with pytest.raises(ValueError, match="some driving"):
        rw._kp_batch(kp(1, True), [kp(1, True), kp(1, False)], 15, "t")
    with pytest.raises(ValueError, match="keypoint values"):
        rw._kp_batch(kp(1, False), {"value": torch.zeros(2, 10, 3), "jacobian": None}, 15, "t")
