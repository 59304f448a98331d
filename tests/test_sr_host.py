"""CPU tests of the Real-ESRNet host side (e4s_amd/sr.py) against the reference's recorded state_dict layout
(tests/golden/sr.pt, written by tests/golden/make_sr_golden.py)."""
import numpy as np
import pytest
import torch

from e4s_amd import synth


def test_state_dict_keys_and_shapes_match_the_reference(golden):
    from e4s_amd.sr import RRDBNet
    g = golden("sr.pt")
    net = RRDBNet(3, 3, scale=4, num_feat=32, num_block=23, num_grow_ch=32)
    sd = net.state_dict()
    assert list(sd.keys()) == g["keys"]
    assert [tuple(v.shape) for v in sd.values()] == [tuple(s) for s in g["shapes"]]
    assert sum(1 for k in sd if k.endswith(".weight")) == 351
    # the seeded weights the GPU tests load are keyed on those names
    net.load_state_dict(synth.synth_rrdb_state_dict(net), strict=True)
    a, b = synth.synth_rrdb_state_dict(net), synth.synth_rrdb_state_dict(RRDBNet())
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_fixture_is_usable_and_the_reference_stays_far_inside_the_bounds(golden):
    g = golden("sr.pt")
    assert [tuple(c[:3]) for c in g["cases"]] == [(1, 5, 7), (2, 40, 48), (1, 256, 256)]
    for i, (b, h, w, _) in enumerate(g["cases"]):
        y = g[f"y.{i}"]
        n = len(g["sample_out"])
        assert tuple(y.shape) == ((b, 3, 4 * h, 4 * w) if h * w <= 64 * 64 else (b, 3, n, n))
        assert g[f"inside.{i}"] >= 0.5
        assert g[f"e32.{i}"] <= 1e-5 * g[f"scale.{i}"]                 # the reference's own fp32 error: 100 x inside the f32 bound
    for name in ("rdb1", "rrdb", "trunk"):
        assert tuple(g[f"mid.{name}"].shape) == (2, 32, len(g["mid_rows"]), len(g["mid_cols"]))


def test_refused_configurations_raise():
    from e4s_amd.sr import RRDBNet, RealESRNet
    for scale in (2, 1):
        with pytest.raises(NotImplementedError):
            RRDBNet(3, 3, scale=scale)
        with pytest.raises(NotImplementedError):
            RealESRNet(scale=scale, device="cpu")
    with pytest.raises(NotImplementedError):
        RRDBNet(3, 3, num_feat=64)
    with pytest.raises(NotImplementedError):
        RRDBNet(3, 3, num_grow_ch=16)
    net = RRDBNet(3, 3, num_block=1)
    with pytest.raises(RuntimeError):                                   # no CPU path
        net(torch.zeros(1, 3, 8, 8))
    sr = RealESRNet(device="cpu")
    sr.srmodel = net
    with pytest.raises(RuntimeError):
        sr.upscale(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        net(torch.zeros(1, 8, 8, 3))
    with pytest.raises(ValueError):
        sr.process(np.zeros((8, 8, 3), dtype=np.float32))


def test_uint8_rule_is_numpy_round_half_even_on_the_half_grid():
    """real_esrnet.py:53-55: clamp(0, 1), * 255.0 in fp32, numpy.round (half to even), astype(uint8)."""
    from e4s_amd.sr import round_half_even_u8
    k = np.arange(-2, 258, dtype=np.float32)
    for v in ((k + np.float32(0.5)) / np.float32(255), k / np.float32(255), np.nextafter((k + np.float32(0.5)) / np.float32(255), np.float32(9)),
              np.nextafter((k + np.float32(0.5)) / np.float32(255), np.float32(-9))):
        v = v.astype(np.float32)
        ref = (np.clip(v, 0, 1) * 255.0).round().astype(np.uint8)
        assert ref.dtype == np.uint8 and (np.clip(v, 0, 1) * 255.0).dtype == np.float32
        assert np.array_equal(round_half_even_u8(v).numpy(), ref)
        assert np.array_equal(round_half_even_u8(torch.from_numpy(v)).numpy(), ref)
    exact = np.array([0.5, 1.5, 2.5, 253.5, 254.5], dtype=np.float32)   # ties that survive the fp32 product exactly
    assert np.array_equal(np.round(exact), [0, 2, 2, 254, 254])
    assert np.array_equal(torch.round(torch.from_numpy(exact)).numpy(), np.round(exact))
