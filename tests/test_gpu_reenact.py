"""GPU tests of the face-vid2vid pose front end (e4s_amd/reenact.py, csrc/vid2vid.hip) against the REAL reference's fp64 records
(tests/golden/reenact.pt, tests/golden/make_reenact_golden.py) and fp64 torch restatements of the single kernels.

Bounds (those of test_gpu_retinaface.py): a single layer 1e-5 x scale (f32) and 1e-3 x scale (bf16x3); a whole network, up to the
logits or the raw head outputs, 1e-4 x scale and 1e-3 x scale; scale = max |fp64 reference|.

What follows a softmax has no free tolerance.  If every logit is within delta of the reference's, every softmax weight changes by a
factor within e^{+-2 delta / T}, so an expectation of values in [-v, v] moves by at most v (e^{2 delta / T} - 1):
    KPDetector value       v = 1 (the coordinate grid), T = 0.1, delta = the logit bound applied
    KPDetector jacobian    v = max |jacobian maps|, plus the maps' own error (the network bound x their scale)
    degrees                v = 3 x 65 (66 bins, x 3), T = 1, delta = the raw-output bound applied
Transformed keypoints R kp + t + exp: an angle error of a degrees is a x 3.14 / 180 radians; each entry of Rx Ry Rz moves by at most
the sum of the three, so |d value| <= 3 max |kp| sum(d angle) + sqrt(3) |d kp| + |d t| + |d exp| (a row of R has 1-norm <= sqrt(3)),
and the same with J for kp for the jacobian, without t and exp.  The final fp32 kernel adds the single-layer 1e-5 x scale."""
import math

import pytest
import torch
import torch.nn.functional as F

from e4s_amd import synth
from guarded_alloc import _GuardedTorch, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = [("f32", 1e-5, 1e-4), ("bf16x3", 1e-3, 1e-3)]                 # (PRECISION, single-layer bound, whole-network bound)
CHANNELS = [(32, 32), (64, 32), (32, 64), (32, 15)]
VOLUMES = [(1, 1, 1), (3, 5, 7), (4, 16, 8), (2, 33, 17)]                  # one voxel; odd; the reduced net's last; more than one tile, ragged
_STATE = {}


@pytest.fixture(scope="module")
def g(golden):
    return golden("reenact.pt")


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def _err(got, ref, tol, what):
    scale = float(ref.abs().max())
    err = float((got.double().cpu() - ref).abs().max())
    print(f"{what}: err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, (what, err, tol * scale)


def _abs_err(got, ref, bound, what):
    err = float((got.double().cpu() - ref).abs().max())
    print(f"{what}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def _conv3d_64(x_ndhwc, w, bias, up2, relu):
    x = x_ndhwc.double().permute(0, 4, 1, 2, 3)
    if up2:
        x = F.interpolate(x, scale_factor=(1, 2, 2))
    y = F.conv3d(x, w.double(), None if bias is None else bias.double(), padding=1)
    return (F.relu(y) if relu else y).permute(0, 2, 3, 4, 1)


def _nets(g):
    from e4s_amd import reenact
    if "he" not in _STATE:
        for jac in (1, 0):
            kp = reenact.KPDetector(**g["kp_cfg"], estimate_jacobian=bool(jac))
            kp.load_state_dict(synth.synth_vid2vid_state_dict(kp, seed=g["kp_seed"]), strict=True)
            _STATE[f"kp{jac}"] = kp.to(DEV)
        he = reenact.HEEstimator(block_expansion=64, feature_channel=32, num_kp=15, image_channel=3, max_features=2048, num_bins=66)
        he.load_state_dict(synth.synth_vid2vid_state_dict(he, seed=g["he_seed"]), strict=True)
        _STATE["he"] = he.to(DEV)
    return _STATE


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
def test_conv3d_matches_fp64_with_guard_bands(precision, tol, _, cin, cout):
    from e4s_amd import kernels as K
    f32 = precision == "f32"
    w, bias = _rand(cout, cin, 3, 3, 3, seed=cin + cout) / math.sqrt(27 * cin), _rand(cout, seed=7)
    wp = K.conv3d_pack(w.to(DEV), f32)
    guard = _GuardedTorch()
    for vi, (d, h, wd) in enumerate(VOLUMES):
        for up2, use_bias, relu in ((False, True, True), (True, False, False), (True, True, True), (False, False, False)):
            b = 2 if d * h * wd < 600 else 1
            x = _rand(b, d, h, wd, cin, seed=100 + vi)
            ho, wo = (2 * h, 2 * wd) if up2 else (h, wd)
            y = guard.empty(b, d, ho, wo, cout, device=DEV)
            K.conv3d(x.to(DEV), wp, cout, y, bias=bias.to(DEV) if use_bias else None, relu=relu, up2=up2, f32=f32)
            guard.check()
            assert unwritten(y) == 0
            _err(y, _conv3d_64(x, w, bias if use_bias else None, up2, relu), tol, f"conv3d {cin}->{cout} {d}x{h}x{wd} up2={up2} bias={use_bias} relu={relu}")
    if cout % 4:                                                            # a wider buffer: the padded channels 15 .. 31 are computed, never stored
        x = _rand(1, 2, 33, 17, cin, seed=9)
        y = guard.empty(1, 2, 33, 17, cout + 1, device=DEV)
        K.conv3d(x.to(DEV), wp, cout, y, bias=bias.to(DEV), f32=f32)
        guard.check()
        assert unwritten(y[..., :cout]) == 0 and unwritten(y[..., cout]) == y[..., cout].numel()
        _err(y[..., :cout], _conv3d_64(x, w, bias, False, False), tol, "conv3d into a wider buffer")


def test_conv3d_reads_a_strided_volume_and_refuses_what_it_cannot_take():
    from e4s_amd import kernels as K
    b, d, h, wd, c = 2, 4, 3, 5, 32
    flat = _rand(b, h, wd, d * c, seed=21)                                  # the 1x1 conv's NHWC output, channels (depth, feature)
    vol = flat.to(DEV).view(b, h, wd, d, c).permute(0, 3, 1, 2, 4)
    w = _rand(32, c, 3, 3, 3, seed=22) / math.sqrt(27 * c)
    y = torch.empty(b, d, 2 * h, 2 * wd, 32, device=DEV)
    K.conv3d(vol, K.conv3d_pack(w.to(DEV), True), 32, y, up2=True, f32=True)
    _err(y, _conv3d_64(flat.view(b, h, wd, d, c).permute(0, 3, 1, 2, 4), w, None, True, False), 1e-5, "conv3d on the strided volume")
    with pytest.raises(RuntimeError):
        K.conv3d_pack(_rand(32, 48, 3, 3, 3).to(DEV), True)                 # Cin is no multiple of 32
    with pytest.raises(RuntimeError):
        K.conv3d(vol, K.conv3d_pack(w.to(DEV), False), 32, y, up2=True, f32=True)      # a pack of the other precision
    with pytest.raises(RuntimeError):
        K.conv3d(vol, K.conv3d_pack(w.to(DEV), True), 32, y, f32=True)      # y has the up-sampled size


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_conv3d_batch_and_position_do_not_change_the_bits(precision):
    from e4s_amd import kernels as K
    f32 = precision == "f32"
    for (cin, cout), up2 in (((64, 32), True), ((32, 15), False)):
        w, bias = _rand(cout, cin, 3, 3, 3, seed=1) / math.sqrt(27 * cin), _rand(cout, seed=2)
        wp = K.conv3d_pack(w.to(DEV), f32)
        a, other = _rand(1, 3, 9, 7, cin, seed=3), _rand(1, 3, 9, 7, cin, seed=4)
        run = lambda x: K.conv3d(x.to(DEV), wp, cout, torch.empty(x.shape[0], 3, *((18, 14) if up2 else (9, 7)), cout, device=DEV),
                                 bias=bias.to(DEV), relu=True, up2=up2, f32=f32)
        alone, three = run(a), run(torch.cat([a, other, a]))
        assert torch.equal(three[0], alone[0]) and torch.equal(three[2], alone[0])
        assert not torch.equal(three[1], alone[0])


def _aa64(frames, weight):
    x = frames.double().permute(0, 3, 1, 2)
    k = weight.shape[-1] // 2
    y = F.conv2d(F.pad(x, (k, k, k, k)), weight.double()[None, None].repeat(3, 1, 1, 1), groups=3)
    return y[:, :, ::4, ::4].permute(0, 2, 3, 1)


@pytest.mark.parametrize("h,w", [(75, 61), (64, 48)])
def test_antialias_downsampling_and_average_pool_match_fp64(g, h, w):
    from e4s_amd import kernels as K, reenact
    taps, step = reenact.antialias_taps(0.25)
    tdev = torch.from_numpy(taps).float().to(DEV)
    frames = synth.synth_vid2vid_frames(2, h, w, seed=5)
    got = K.aa_down(frames.to(DEV), tdev, step)
    assert tuple(got.shape) == (2, -(-h // 4), -(-w // 4), 3)
    _err(got, _aa64(frames, g["aa.weight"]), 1e-5, f"anti-alias {h}x{w}")
    u8 = (frames * 255).round().to(torch.uint8)
    _err(K.aa_down(u8.to(DEV), tdev, step), _aa64(u8.double() / 255, g["aa.weight"]), 1e-5, f"anti-alias uint8 {h}x{w}")
    _err(K.aa_down(u8.to(DEV), torch.ones(1, device=DEV), 1), u8.double() / 255, 1e-7, "uint8 -> float")
    x = _rand(2, h, w, 64, seed=6)
    guard = _GuardedTorch()
    y = K.avgpool2(x.to(DEV), guard.empty(2, h // 2, w // 2, 64, device=DEV))
    guard.check()
    assert unwritten(y) == 0
    _err(y, F.avg_pool2d(x.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), 1e-5, f"avgpool {h}x{w}")


def _grid64(d, h, w):
    ax = lambda n: 2 * (torch.arange(n, dtype=torch.float64) / (n - 1)) - 1
    z, y, x = torch.meshgrid(ax(d), ax(h), ax(w), indexing="ij")
    return torch.stack([x, y, z], -1)


def _softargmax64(logits, temperature, jac):
    b, k = logits.shape[:2]
    heat = torch.softmax(logits.double().view(b, k, -1) / temperature, dim=2)
    value = (heat.unsqueeze(-1) * _grid64(*logits.shape[2:]).view(1, 1, -1, 3)).sum(2)
    if jac is None:
        return value, None
    jm = jac.double().view(b, -1, 9, heat.shape[2])
    return value, (heat.unsqueeze(2) * jm).sum(-1).view(b, k, 3, 3)


@pytest.mark.parametrize("nmaps", [15, 1])
def test_softargmax_head_matches_fp64_and_is_batch_invariant(nmaps):
    from e4s_amd import kernels as K
    logits = 0.3 * _rand(2, 15, 4, 16, 8, seed=31)
    logits[0, 3, 1, 5, 2] += 1.0                                            # a keypoint with a clear peak, one that is nearly flat
    logits[1, 7] *= 0.01
    jac = _rand(2, 9 * nmaps, 4, 16, 8, seed=32)
    ref_v, ref_j = _softargmax64(logits, 0.1, jac)
    v, j = K.softargmax3d(logits.to(DEV), 0.1, jac.to(DEV))
    _err(v, ref_v, 1e-5, f"soft-argmax value ({nmaps} maps)")
    _err(j, ref_j, 1e-5, f"soft-argmax jacobian ({nmaps} maps)")
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    v2, j2 = K.softargmax3d(cl(logits), 0.1, cl(jac), channels_last=True)
    assert torch.equal(v2, v) and torch.equal(j2, j)                        # the layout does not change the order of the sums
    v1, j1 = K.softargmax3d(logits[1:].to(DEV), 0.1, jac[1:].to(DEV))
    assert torch.equal(v1[0], v[1]) and torch.equal(j1[0], j[1])
    v0, none = K.softargmax3d(logits.to(DEV), 0.1)
    assert none is None and torch.equal(v0, v)


@pytest.mark.parametrize("jac", [1, 0])
@pytest.mark.parametrize("precision,_,tol", PRECISIONS)
def test_reduced_kp_detector_on_frame_a(g, monkeypatch, precision, _, tol, jac):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    net = _nets(g)[f"kp{jac}"]
    frame = synth.synth_vid2vid_frames(*g["frame_A"]).to(DEV)
    taps, pre, cs = {}, f"kp{jac}.", g["tap_cstep"]
    with torch.no_grad():
        logits, jmaps = net.logits_ndhwc(frame, taps)
        out = net.run(frame)
    for name in [f"down{i}" for i in range(3)] + [f"up{i}" for i in range(3)]:
        ref, scale = g[f"{pre}tap.{name}"].double(), g[f"{pre}tap.{name}.scale"]
        got = taps[name][0].permute(2, 0, 1) if name.startswith("down") else taps[name][0].permute(3, 0, 1, 2)
        assert tuple(got[::cs].shape) == tuple(ref.shape), name
        _abs_err(got[::cs], ref, tol * scale, f"{precision} {name}")
    ref_logits = g[pre + "logits"]
    _err(logits[0].permute(3, 0, 1, 2), ref_logits, tol, f"{precision} logits")
    delta = tol * float(ref_logits.abs().max())
    grow = math.exp(2 * delta / g["kp_cfg"]["temperature"]) - 1
    assert float(out["value"].abs().max()) <= 1.0
    _abs_err(out["value"], g[pre + "value"], grow, f"{precision} value")
    if jac:
        js = g[pre + "jmaps.scale"]
        assert abs(float(jmaps.abs().max()) - js) <= tol * js
        _abs_err(out["jacobian"], g[pre + "jacobian"], js * grow + tol * js, f"{precision} jacobian")
    else:
        assert jmaps is None and "jacobian" not in out


def _he_bounds(g, tag, tol):
    """delta of each raw output and the derived bound on the degrees, from the bounds applied to the raw outputs"""
    delta = {k: tol * float(g[f"he.{tag}.{k}"].abs().max()) for k in ("yaw", "pitch", "roll", "t", "exp")}
    deg = {k: 3 * 65 * (math.exp(2 * delta[k]) - 1) for k in ("yaw", "pitch", "roll")}
    return delta, deg


@pytest.mark.parametrize("tag", ["C", "B"])
@pytest.mark.parametrize("precision,_,tol", PRECISIONS)
def test_he_estimator_on_the_fixture_frames(g, monkeypatch, precision, _, tol, tag):
    from e4s_amd import kernels as K, reenact
    monkeypatch.setattr(K, "PRECISION", precision)
    st = _nets(g)
    fe = reenact.PoseFrontEnd(st["kp0"], st["he"], False)
    frames = synth.synth_vid2vid_frames(*g[f"frame_{tag}"]).to(DEV)
    raw = st["he"].run(frames)
    for k in ("yaw", "pitch", "roll", "t", "exp"):
        _err(raw[k], g[f"he.{tag}.{k}"], tol, f"{precision} {tag} {k}")
    pose = fe.head_pose_device(frames)
    _, deg = _he_bounds(g, tag, tol)
    for i, k in enumerate(("yaw", "pitch", "roll")):
        assert tuple(pose[k].shape) == (frames.shape[0],)
        _abs_err(pose[k], g[f"he.{tag}.degrees"][:, i], deg[k], f"{precision} {tag} {k} degrees")
    assert torch.equal(pose["t"], raw["t"]) and torch.equal(pose["exp"], raw["exp"])
    u8 = (frames * 255).round().to(torch.uint8)                              # uint8 frames are read as x / 255
    as_float = u8.float() / torch.full_like(u8, 255, dtype=torch.float32)     # an IEEE division (a scalar divisor becomes a reciprocal multiply)
    assert torch.equal(st["he"].run(u8)["t"], st["he"].run(as_float)["t"])


@pytest.mark.parametrize("precision,_,tol", PRECISIONS)
def test_pose_front_end_keypoints_equal_the_composition_of_the_parts(g, monkeypatch, precision, _, tol):
    from e4s_amd import kernels as K, reenact
    monkeypatch.setattr(K, "PRECISION", precision)
    st = _nets(g)
    fe = reenact.PoseFrontEnd(st["kp1"], st["he"], True)
    src = synth.synth_vid2vid_frames(*g["frame_A"])[0]
    drv = synth.synth_vid2vid_frames(*g["frame_B"])
    kp_source, kp_driving = fe.keypoints(src.numpy(), [f.numpy() for f in drv])
    alone, none = fe.keypoints_device(src.to(DEV))
    assert none == [] and torch.equal(alone["value"], kp_source["value"]) and torch.equal(alone["jacobian"], kp_source["jacobian"])
    assert len(kp_driving) == 2 and tuple(kp_source["value"].shape) == (1, 15, 3) and tuple(kp_driving[1]["jacobian"].shape) == (1, 15, 3, 3)
    # the canonical keypoints' own bounds (test_reduced_kp_detector_on_frame_a)
    grow = math.exp(2 * tol * float(g["kp1.logits"].abs().max()) / g["kp_cfg"]["temperature"]) - 1
    js = g["kp1.jmaps.scale"]
    d_kp, d_j = grow, js * grow + tol * js
    kp_max, j_max = float(g["kp1.value"].abs().max()), float(g["kp1.jacobian"].abs().max())

    def check(got, tag, i, what):
        delta, deg = _he_bounds(g, tag, tol)
        d_angle = sum(deg.values()) * 3.14 / 180
        ref_v, ref_j = g[f"he.{tag}.value"][i:i + 1], g[f"he.{tag}.jacobian"][i:i + 1]
        bound_v = 3 * kp_max * d_angle + math.sqrt(3) * d_kp + delta["t"] + delta["exp"] + 1e-5 * float(ref_v.abs().max())
        bound_j = 3 * j_max * d_angle + math.sqrt(3) * d_j + 1e-5 * float(ref_j.abs().max())
        _abs_err(got["value"], ref_v, bound_v, f"{precision} {what} value")
        _abs_err(got["jacobian"], ref_j, bound_j, f"{precision} {what} jacobian")
    check(kp_source, "A", 0, "kp_source")
    for i in range(2):
        check(kp_driving[i], "B", i, f"kp_driving[{i}]")
    # free view: fixed angles replace the estimates of the driving frames only, as in make_animation
    ks, kd = fe.keypoints_device(src.to(DEV), drv.to(DEV), free_view=True, yaw=20.0, pitch=None, roll=-5.0)
    assert torch.equal(ks["value"], kp_source["value"])
    he = {k: g[f"he.B.{k}"] for k in ("yaw", "pitch", "roll", "t", "exp")}
    ref = reenact.keypoint_transformation({"value": g["kp1.value"], "jacobian": g["kp1.jacobian"]}, he, True, True, 20.0, None, -5.0)
    _, deg = _he_bounds(g, "B", tol)
    delta = _he_bounds(g, "B", tol)[0]
    bound = 3 * kp_max * deg["pitch"] * 3.14 / 180 + math.sqrt(3) * d_kp + delta["t"] + delta["exp"] + 1e-5 * float(ref["value"].abs().max())
    _abs_err(torch.cat([k["value"] for k in kd]), ref["value"], bound, f"{precision} free-view value")
    # without the jacobian the dicts carry None
    ks0, kd0 = reenact.PoseFrontEnd(st["kp0"], st["he"], False).keypoints_device(src.to(DEV), drv.to(DEV))
    assert ks0["jacobian"] is None and kd0[0]["jacobian"] is None and torch.equal(ks0["value"], kp_source["value"])
