"""GPU tests of face-vid2vid's SPADE decoder (e4s_amd/spade.py, csrc/spade.hip) against the REAL reference's fp64 records
(tests/golden/spade.pt, tests/golden/make_spade_golden.py) and fp64 torch restatements of the single kernels.

Bounds (those of test_gpu_reenact_warp.py): a single layer 1e-5 x scale (f32) and 1e-3 x scale (bf16x3); the whole network 1e-4 x
scale and 1e-3 x scale, scale = max |fp64 reference| (recorded per tap); the streaming tail is fp32 in either mode: 1e-5 x scale.
    modulating conv   v = n (1 + gamma) + beta with gamma and beta two single layers: first order, tol x (max |n| max |1 + gamma| +
                      max |beta|), every maximum taken from the fp64 restatement (LeakyReLU is 1-Lipschitz)
    prediction        sigmoid is 1/4-Lipschitz: 0.25 x the network bound x max |logit| + 1e-5 (the rule of the occlusion map)"""
import math

import pytest
import torch
import torch.nn.functional as F

from e4s_amd import synth
from guarded_alloc import _GuardedTorch, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = [("f32", 1e-5, 1e-4), ("bf16x3", 1e-3, 1e-3)]                 # (PRECISION, single-layer bound, whole-network bound)
STREAM_TOL = 1e-5
SMALL_GEN = dict(image_channel=3, feature_channel=32, num_kp=15, block_expansion=64, max_features=256, num_down_blocks=2, reshape_channel=32,
                 reshape_depth=8, num_resblocks=1, estimate_occlusion_map=True,
                 dense_motion_params=dict(block_expansion=32, max_features=128, num_blocks=2, reshape_depth=8, compress=4))
_STATE = {}


@pytest.fixture(scope="module")
def g(golden):
    return golden("spade.pt")


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def _abs_err(got, ref, bound, what):
    err = float((got.double().cpu() - ref).abs().max())
    print(f"{what}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def _err(got, ref, tol, what):
    _abs_err(got, ref, tol * float(ref.abs().max()), what)


def _nchw64(t):
    return t.double().permute(0, 3, 1, 2)


# ---- the modulating conv ------------------------------------------------------------------------------------------------------------
def _mod_case(c, xs, hw, seed):
    """N = 2; sample 1's x is 3 x + 2 of other data, so a tile that mixed the samples' statistics would show"""
    h, w = hw
    xh, xw = h >> xs, w >> xs
    x = _rand(2, xh, xw, c, seed=seed)
    x[1] = 3 * _rand(xh, xw, c, seed=seed + 1) + 2
    a = torch.full((2, h, w, 384), 50.0)                                     # the neighbouring slices hold other data
    a[..., 128:256] = _rand(2, h, w, 128, seed=seed + 2).abs()
    wg, wb = _rand(c, 128, 3, 3, seed=seed + 3) / math.sqrt(9 * 128), _rand(c, 128, 3, 3, seed=seed + 4) / math.sqrt(9 * 128)
    bg, bb = 0.1 * _rand(c, seed=seed + 5), 0.1 * _rand(c, seed=seed + 6)
    return x, a, wg, bg, wb, bb


def _mod64(x, a, wg, bg, wb, bb, xs, act):
    A = _nchw64(a[..., 128:256])
    gamma, beta = F.conv2d(A, wg.double(), bg.double(), padding=1), F.conv2d(A, wb.double(), bb.double(), padding=1)
    X = _nchw64(x)
    n = (X - X.mean((2, 3), keepdim=True)) / torch.sqrt(X.var((2, 3), unbiased=False, keepdim=True) + 1e-5)
    if xs:
        n = F.interpolate(n, scale_factor=2, mode="nearest")
    v = n * (1 + gamma) + beta
    first_order = float(n.abs().max()) * float((1 + gamma).abs().max()) + float(beta.abs().max())
    return (F.leaky_relu(v, 0.2) if act else v).permute(0, 2, 3, 1), first_order


@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("xs,hw", [(0, (6, 5)), (0, (12, 10)), (1, (12, 10))])
@pytest.mark.parametrize("c", [64, 512])
@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
def test_modulating_conv_matches_fp64_with_guard_bands(precision, tol, _, c, xs, hw, act):
    from e4s_amd import kernels as K, spade
    f32 = precision == "f32"
    x, a, wg, bg, wb, bb = _mod_case(c, xs, hw, seed=100 + c + 7 * xs)
    ref, first_order = _mod64(x, a, wg, bg, wb, bb, xs, act)
    wp = K.rconv_pack(spade.interleave_gamma_beta(wg, wb).to(DEV), f32)
    bias = spade.interleave_gamma_beta(bg, bb).to(DEV)
    xd = x.to(DEV)
    stats, _p = K.instnorm_stats(xd)
    guard = _GuardedTorch()
    y = guard.empty(2, *hw, c, device=DEV)
    K.spade_conv(a.to(DEV), 128, 128, wp, bias, xd, stats, y, xs=xs, act=act, f32=f32)
    guard.check()                                                            # nothing outside the output is written
    assert unwritten(y) == 0
    _abs_err(y, ref, tol * first_order, f"{precision} C {c} xs {xs} {hw} act {act}")
    # into a channel slice of a wider buffer: the neighbours stay
    wide = guard.empty(2, *hw, c + 64, device=DEV)
    K.spade_conv(a.to(DEV), 128, 128, wp, bias, xd, stats, wide, xs=xs, act=act, y_coff=32, f32=f32)
    guard.check()
    assert torch.equal(wide[..., 32:32 + c], y) and unwritten(wide) == wide[..., :64].numel()


# ---- mlp_shared through the nearest upsampling --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
def test_shared_conv_through_the_upsampling_matches_fp64(precision, tol, _, shift):
    from e4s_amd import kernels as K, spade
    f32 = precision == "f32"
    torch.manual_seed(3)
    spades = [spade.SPADE(64, 256) for _i in range(3)]
    for i, s in enumerate(spades):
        s.mlp_shared[0].weight.data = _rand(128, 256, 3, 3, seed=20 + i) / math.sqrt(9 * 256)
        s.mlp_shared[0].bias.data = 0.1 * _rand(128, seed=30 + i)
    seg = _rand(2, 5, 3, 256, seed=40)
    h, w = 5 << shift, 3 << shift
    up = F.interpolate(_nchw64(seg), size=(h, w), mode="nearest")
    wc, bc = spade.concat_shared(spades)
    guard = _GuardedTorch()
    y = guard.empty(2, h, w, 384 + 64, device=DEV)                           # the three SPADEs' slices behind 64 channels of another owner
    K.spade_shared(seg.to(DEV), 256, K.rconv_pack(wc.to(DEV), f32), 384, bc.to(DEV), y, shift=shift, y_coff=64, f32=f32)
    guard.check()
    assert unwritten(y[..., 64:]) == 0 and unwritten(y[..., :64]) == y[..., :64].numel()
    for i, s in enumerate(spades):
        conv = s.mlp_shared[0]
        ref = F.relu(F.conv2d(up, conv.weight.detach().double(), conv.bias.detach().double(), padding=1)).permute(0, 2, 3, 1)
        assert float((ref == 0).double().mean()) > 0.2
        pre = F.conv2d(up, conv.weight.detach().double(), conv.bias.detach().double(), padding=1)
        _abs_err(y[..., 64 + 128 * i:64 + 128 * (i + 1)], ref, tol * float(pre.abs().max()), f"{precision} shift {shift} SPADE {i}")
    if shift:                                                                # the upsampled seg, made in memory, gives the same bits
        direct = torch.empty(2, h, w, 384, device=DEV)
        K.spade_shared(up.permute(0, 2, 3, 1).float().contiguous().to(DEV), 256, K.rconv_pack(wc.to(DEV), f32), 384, bc.to(DEV), direct, f32=f32)
        assert torch.equal(direct, y[..., 64:])


# ---- the tail -----------------------------------------------------------------------------------------------------------------------
def test_tail_matches_fp64_and_its_uint8_is_the_rounding_rule(monkeypatch):
    from e4s_amd import kernels as K
    b, h, w = 2, 7, 9
    x = torch.full((b, h, w, 96), 9.0)
    x[..., :64] = 2 * _rand(b, h, w, 64, seed=50)
    wt, bias = _rand(3, 64, 3, 3, seed=51) / math.sqrt(9 * 64) * 2, 0.1 * _rand(3, seed=52)
    z = F.conv2d(F.leaky_relu(_nchw64(x[..., :64]), 0.2), wt.double(), bias.double(), padding=1)
    ref = torch.sigmoid(z)
    assert float(ref.min()) < 0.3 and float(ref.max()) > 0.7
    guard = _GuardedTorch()
    monkeypatch.setattr(K, "torch", guard)
    wp = K.spade_tail_pack(wt.to(DEV))
    logits = guard.empty(b, 3, h, w, device=DEV)
    out = K.spade_tail(x.to(DEV), wp, bias.to(DEV), logits=logits)
    nhwc = K.spade_tail(x.to(DEV), wp, bias.to(DEV), nchw=False)
    u8 = K.spade_tail(x.to(DEV), wp, bias.to(DEV), u8=True)
    guard.check()
    assert unwritten(out) == 0 and unwritten(nhwc) == 0 and unwritten(logits) == 0      # (u8: every element is compared below)
    assert tuple(out.shape) == (b, 3, h, w) and tuple(u8.shape) == (b, h, w, 3) and u8.dtype == torch.uint8
    _err(logits, z, STREAM_TOL, "tail logits")
    _abs_err(out, ref, 0.25 * STREAM_TOL * float(z.abs().max()) + STREAM_TOL, "tail prediction")
    assert torch.equal(nhwc, out.permute(0, 2, 3, 1))
    rule = torch.round(out.permute(0, 2, 3, 1).clamp(0, 1) * 255).to(torch.uint8)      # torch.round: half to even
    assert torch.equal(u8, rule)


# ---- the whole decoder against the reference's fp64 records -------------------------------------------------------------------------
def _decoder(g):
    from e4s_amd import spade
    if "dec" not in _STATE:
        dec = spade.SPADEDecoder()
        dec.load_state_dict(synth.synth_vid2vid_decoder_state_dict(dec, seed=g["dec_seed"]), strict=True)
        _STATE["dec"] = dec.to(DEV)
    return _STATE["dec"]


def _feature(g, case):
    c = g["cases"][case]
    return synth.synth_vid2vid_decoder_feature(c["n"], c["h"], c["w"], c["seed"]).to(DEV).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("precision,_,tol", PRECISIONS)
def test_decoder_against_the_reference(g, monkeypatch, precision, _, tol, case):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    dec = _decoder(g)
    feat = _feature(g, case)
    before = feat.clone()
    taps, cs = {}, g["tap_cstep"]
    pred = dec.run(feat, taps=taps)
    assert torch.equal(feat, before)                                         # read in place, left alone
    n, _c, h, w = feat.shape
    assert tuple(pred.shape) == (n, 3, 4 * h, 4 * w) and pred.dtype == torch.float32
    for name in g["taps"]:
        ref = g[f"{case}.tap.{name}"]
        _abs_err(taps[name].permute(0, 3, 1, 2)[:, ::cs], ref, tol * g[f"{case}.tap.{name}.scale"], f"{precision} {case} {name}")
    z = g[f"{case}.logits"]
    _abs_err(taps["logits"], z, tol * g[f"{case}.logits.scale"], f"{precision} {case} logits")
    _abs_err(pred, torch.sigmoid(z), 0.25 * tol * float(z.abs().max()) + 1e-5, f"{precision} {case} prediction")
    again = dec.run(feat.permute(0, 2, 3, 1))                               # the NHWC form, no taps: the same bits, a fresh tensor
    assert torch.equal(again, pred) and again.data_ptr() != pred.data_ptr()
    u8 = dec.run(feat, u8=True)
    assert tuple(u8.shape) == (n, 4 * h, 4 * w, 3) and torch.equal(u8, torch.round(pred.permute(0, 2, 3, 1).clamp(0, 1) * 255).to(torch.uint8))


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_batching_does_not_change_the_bits(g, monkeypatch, precision):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    dec = _decoder(g)
    three = synth.synth_vid2vid_decoder_feature(3, 9, 7, 33).to(DEV).contiguous(memory_format=torch.channels_last)
    together = dec.run(three)
    for i in range(3):
        alone = dec.run(three[i:i + 1].contiguous(memory_format=torch.channels_last))
        assert torch.equal(alone[0], together[i]), i
    assert not torch.equal(together[0], together[1])
    with pytest.raises(RuntimeError, match="channels-last"):
        dec.run(three.contiguous())                                         # a plain NCHW tensor would need a copy: refused


# ---- composition --------------------------------------------------------------------------------------------------------------------
def _generator():
    from e4s_amd import spade
    if "gen" not in _STATE:
        gen = spade.OcclusionAwareSPADEGenerator(**SMALL_GEN)
        sd = synth.synth_vid2vid_generator_state_dict(gen, seed=3)
        sd.update({"decoder." + k: v for k, v in synth.synth_vid2vid_decoder_state_dict(gen.decoder, seed=3).items()})
        gen.load_generator_state_dict(sd)
        _STATE["gen"] = gen.to(DEV)
    return _STATE["gen"]


def test_generator_and_reenactor_equal_the_composition_of_their_parts(golden):
    from e4s_amd import reenact, reenact_warp as rw, spade
    r = golden("reenact.pt")
    kp = reenact.KPDetector(**r["kp_cfg"], estimate_jacobian=True)
    kp.load_state_dict(synth.synth_vid2vid_state_dict(kp, seed=r["kp_seed"]), strict=True)
    he = reenact.HEEstimator(block_expansion=64, feature_channel=32, num_kp=15, image_channel=3, max_features=2048, num_bins=66)
    he.load_state_dict(synth.synth_vid2vid_state_dict(he, seed=r["he_seed"]), strict=True)
    fe = reenact.PoseFrontEnd(kp.to(DEV), he.to(DEV), True)
    gen = _generator()
    src = synth.synth_vid2vid_frames(*r["frame_A"])[0]                      # 64 x 48
    drv = synth.synth_vid2vid_frames(*r["frame_B"])[:, :, :48].contiguous()  # two driving frames, cut to the source's size
    ks, kd = fe.keypoints(src.numpy(), [f.numpy() for f in drv])
    out = gen.run(src.to(DEV), ks, kd)
    warp = rw.FeatureWarp.run(gen, src.to(DEV), ks, kd)
    assert set(out) == set(warp) | {"prediction"}
    for key in warp:
        assert torch.equal(out[key], warp[key]), key
    assert tuple(out["feature"].shape) == (2, 256, 16, 12) and tuple(out["prediction"].shape) == (2, 3, 64, 48)
    assert torch.equal(out["prediction"], gen.decoder.run(warp["feature"]))
    both = spade.Reenactor(fe, gen)
    frames = both.run(src.numpy(), [f.numpy() for f in drv])
    assert tuple(frames.shape) == (2, 64, 48, 3) and frames.is_cuda and torch.equal(frames, out["prediction"].permute(0, 2, 3, 1))
    u8 = both.run(src.numpy(), drv.numpy(), u8=True)
    assert u8.dtype == torch.uint8 and torch.equal(u8, torch.round(frames.clamp(0, 1) * 255).to(torch.uint8))
    ksf, kdf = fe.keypoints(src.numpy(), [f.numpy() for f in drv], free_view=True, yaw=10.0, pitch=None, roll=None)
    free = both.run(src.numpy(), drv.numpy(), free_view=True, yaw=10.0, pitch=None, roll=None)
    assert torch.equal(free, gen.run(src.to(DEV), ksf, kdf)["prediction"].permute(0, 2, 3, 1)) and not torch.equal(free, frames)
    anim = both.make_animation(src.numpy(), drv.numpy())
    assert isinstance(anim, list) and len(anim) == 2
    for i, f in enumerate(anim):
        assert f.shape == (64, 48, 3) and str(f.dtype) == "float32" and float(f.min()) >= 0.0 and float(f.max()) <= 1.0
        assert torch.equal(torch.from_numpy(f), frames[i].cpu())
    assert float(frames.min()) < 0.45 and float(frames.max()) > 0.55        # not a flat grey frame


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_what_the_kernels_cannot_take():
    from e4s_amd import kernels as K, spade
    c, h, w = 64, 4, 6
    x, a, wg, bg, wb, bb = _mod_case(c, 0, (h, w), seed=7)
    wp = K.rconv_pack(spade.interleave_gamma_beta(wg, wb).to(DEV), False)
    bias = spade.interleave_gamma_beta(bg, bb).to(DEV)
    xd, ad = x.to(DEV), a.to(DEV)
    stats, _p = K.instnorm_stats(xd)
    y = torch.zeros(2, h, w, c, device=DEV)
    ok = lambda **kw: K.spade_conv(kw.pop("a", ad), kw.pop("a_coff", 128), 128, kw.pop("wp", wp), bias, kw.pop("x", xd), stats, kw.pop("y", y), f32=False, **kw)
    ok()
    assert float(y.abs().max()) > 0.1
    y.zero_()                                                                # a refused call that launched all the same would fill it again

    def off_by_one_float(t):                                                 # the same values at a pointer that is 4 bytes off a 16-byte boundary
        buf = torch.zeros(t.numel() + 4, device=DEV)
        buf[1:1 + t.numel()] = t.reshape(-1)
        return buf[1:1 + t.numel()].view(t.shape)
    with pytest.raises(RuntimeError):
        ok(a=off_by_one_float(ad))                                           # a misaligned pointer
    with pytest.raises(RuntimeError):
        ok(x=off_by_one_float(xd))
    with pytest.raises(RuntimeError):
        ok(y=off_by_one_float(y))
    with pytest.raises(RuntimeError):
        ok(a_coff=130)                                                       # a channel offset that is no multiple of 4
    with pytest.raises(RuntimeError):
        ok(y=torch.zeros(2, h, w, c + 8, device=DEV), y_coff=2)
    with pytest.raises(RuntimeError):
        ok(y=xd)                                                             # the output over its own input
    with pytest.raises(RuntimeError):
        ok(a=torch.zeros(2, h, w, 128, device=DEV), a_coff=0, y=torch.zeros(2, h, w, 128, device=DEV)[..., :64])     # not contiguous
    with pytest.raises(RuntimeError, match="precision"):
        ok(wp=K.rconv_pack(spade.interleave_gamma_beta(wg, wb).to(DEV), True))          # a pack of the other precision
    with pytest.raises(RuntimeError, match="shifted by xs"):
        ok(xs=1)                                                             # x is not the output's size shifted by xs
    with pytest.raises(RuntimeError, match="shifted by xs"):
        ok(x=torch.zeros(2, h, w - 1, c, device=DEV))
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0                                       # no refused call launched anything
    seg = torch.zeros(1, 3, 3, 256, device=DEV)
    wsh = K.rconv_pack(torch.zeros(128, 256, 3, 3, device=DEV), False)
    out = torch.zeros(1, 6, 6, 128, device=DEV)
    K.spade_shared(seg, 256, wsh, 128, None, out, shift=1, f32=False)
    with pytest.raises(RuntimeError):
        K.spade_shared(seg, 256, wsh, 128, None, out, shift=3, f32=False)
    with pytest.raises(RuntimeError):
        K.spade_shared(seg, 256, wsh, 128, None, out, shift=2, f32=False)   # y of another size
    with pytest.raises(RuntimeError, match="precision"):
        K.spade_shared(seg, 256, wsh, 128, None, out, shift=1, f32=True)
    with pytest.raises(RuntimeError):
        K.spade_shared(seg, 256, wsh, 128, None, torch.zeros(1, 6, 6, 136, device=DEV), shift=1, y_coff=6, f32=False)
    with pytest.raises(RuntimeError):
        K.spade_shared(off_by_one_float(seg), 256, wsh, 128, None, out, shift=1, f32=False)
    with pytest.raises(RuntimeError):
        K.spade_tail(torch.zeros(1, 4, 4, 32, device=DEV), torch.zeros(9, 3, 64, device=DEV), torch.zeros(3, device=DEV))       # fewer than 64 channels
    with pytest.raises(RuntimeError):
        K.spade_tail(off_by_one_float(torch.zeros(1, 4, 4, 64, device=DEV)), torch.zeros(9, 3, 64, device=DEV), torch.zeros(3, device=DEV))


# ---- the shipped size ---------------------------------------------------------------------------------------------------------------
def test_shipped_size_smoke(golden, monkeypatch):
    """The shipped vox-256.yaml generator on one 256 x 256 frame, split-bf16, the weights left as constructed."""
    from e4s_amd import criteria, kernels as K, spade
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", True)
    torch.manual_seed(0)
    gen = spade.OcclusionAwareSPADEGenerator(**golden("reenact_warp.pt")["gen_shipped"]).to(DEV)
    ks, kd = synth.synth_vid2vid_keypoints(1, 7, False)
    frame = synth.synth_vid2vid_frames(1, 256, 256, seed=9).to(DEV)
    out = gen.run(frame, {"value": ks["value"].to(DEV), "jacobian": None}, {"value": kd["value"].to(DEV), "jacobian": None})
    pred = out["prediction"]
    assert tuple(pred.shape) == (1, 3, 256, 256) and bool(torch.isfinite(pred).all())
    assert 0.0 <= float(pred.min()) and float(pred.max()) <= 1.0
