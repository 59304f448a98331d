"""GPU tests of the RetinaFace-R50 detector (e4s_amd/retinaface.py, csrc/retinaface.hip) against the REAL reference's fp64 outputs and
its own post-processing (tests/golden/retinaface.pt, tests/golden/make_retinaface_golden.py) and fp64 torch restatements of the convs.

Bounds (those of test_gpu_parsenet.py / test_gpu_sr.py): a single layer 1e-5 x scale (f32) and 1e-3 x scale (bf16x3); the whole network
1e-4 x scale and 1e-3 x scale; scale = max |fp64 reference|.  Post-processing: the kept set and its order equal the reference's exactly
(the fixture's generation-time margins make the reference alone fix the answer), boxes and landmarks within 1e-4 px + 1e-6 |value|,
scores within 1e-6."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from e4s_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = [("f32", 1e-5, 1e-4), ("bf16x3", 1e-3, 1e-3)]                 # (PRECISION, single-layer bound, whole-network bound)
SENTINEL = 12345.0
PAIRS = [(64, 64), (64, 256), (256, 128), (512, 2048)]
SIZES = [(19, 28), (5, 7), (8, 16)]                                        # odd; smaller than a tile; exactly one 128-pixel tile
MEAN = (104.0, 117.0, 123.0)
_STATE = {}


@pytest.fixture(scope="module")
def g(golden):
    return golden("retinaface.pt")


def _detector(g):
    from e4s_amd.retinaface import RetinaFaceDetection
    if "det" not in _STATE:
        det = RetinaFaceDetection(None, device=DEV)
        det.net.load_state_dict(synth.synth_retinaface_state_dict(det.net, seed=g["weights_seed"]), strict=True)
        det.net.to(DEV).eval()
        _STATE["det"] = det
    return _STATE["det"]


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def _conv64(x_nhwc, w, k, stride):
    return F.conv2d(x_nhwc.double().permute(0, 3, 1, 2), w.double(), None, stride=stride, padding=k // 2).permute(0, 2, 3, 1)


def _err(got, ref, tol, what):
    scale = float(ref.abs().max())
    err = float((got.double().cpu() - ref).abs().max())
    print(f"{what}: err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, (what, err, tol * scale)


def _run(x, w, k, stride, f32, **kw):
    from e4s_amd import kernels as K
    cout, cin = w.shape[:2]
    b, h, wd, _ = x.shape
    y = kw.pop("y", None)
    if y is None:
        y = torch.empty(b, K.rconv_out_size(h, k, stride), K.rconv_out_size(wd, k, stride), cout, device=DEV)
    return K.rconv(x.to(DEV), cin, K.rconv_pack(w.to(DEV), f32), cout, k, y, stride=stride, f32=f32, **kw)


@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
def test_conv_family_matches_fp64_at_odd_sub_tile_and_one_tile_sizes(precision, tol, _):
    f32 = precision == "f32"
    for cin, cout in PAIRS:
        for k in (1, 3):
            w = _rand(cout, cin, k, k, seed=cin + cout + k) / (cin * k * k) ** 0.5
            bias = _rand(cout, seed=5)
            for stride in (1, 2):
                for h, wd in SIZES:
                    x = _rand(1 if cout >= 2048 else 2, h, wd, cin, seed=h * wd + k)
                    ref = F.relu(_conv64(x, w, k, stride) + bias.double())
                    assert tuple(ref.shape[1:3]) == (-(-h // stride), -(-wd // stride))
                    got = _run(x, w, k, stride, f32, bias=bias.to(DEV), act=True)
                    _err(got, ref, tol, f"{precision} {cin}->{cout} k{k} s{stride} {h}x{wd}")


@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
def test_conv_epilogues(precision, tol, _):
    f32 = precision == "f32"
    cin, cout, k = 256, 128, 3
    w = _rand(cout, cin, k, k, seed=1) / (cin * 9) ** 0.5
    bias = _rand(cout, seed=2)
    x = _rand(2, 5, 7, cin, seed=3)
    lin = _conv64(x, w, k, 1) + bias.double()
    r0 = _rand(2, 5, 7, cout + 4, seed=4)                                   # a wider residual buffer: its channel stride is honoured
    got = _run(x, w, k, 1, f32, bias=bias.to(DEV), act=True, r0=r0.to(DEV))
    _err(got, F.relu(lin + r0[..., :cout].double()), tol, "+ r0 then ReLU")
    # LeakyReLU(0.1), then + r0 read through a nearest upsampling from 3 x 4 to 5 x 7
    small = _rand(2, 3, 4, cout, seed=6)
    up = F.interpolate(small.double().permute(0, 3, 1, 2), size=(5, 7), mode="nearest").permute(0, 2, 3, 1)
    got = _run(x, w, k, 1, f32, bias=bias.to(DEV), act=True, slope=0.1, r0=small.to(DEV), r0_after=True)
    _err(got, F.leaky_relu(lin, 0.1) + up, tol, "lrelu then + nearest(r0)")
    # the same with the 1x1 lateral conv of the FPN, stride 2 on an odd map, upsampling 4 -> 7 and 5 -> 10 style ratios
    w1 = _rand(cout, cin, 1, 1, seed=7) / cin ** 0.5
    x1 = _rand(1, 10, 14, cin, seed=8)
    small = _rand(1, 5, 7, cout, seed=9)
    up = F.interpolate(small.double().permute(0, 3, 1, 2), size=(10, 14), mode="nearest").permute(0, 2, 3, 1)
    got = _run(x1, w1, 1, 1, f32, act=True, r0=small.to(DEV), r0_after=True)
    _err(got, F.relu(_conv64(x1, w1, 1, 1)) + up, tol, "1x1 relu then + nearest(r0) x2")
    # channel-offset write into a sentinel-filled wider buffer
    y = torch.full((2, 5, 7, 256 + 8), SENTINEL, device=DEV)
    got = _run(x, w, k, 1, f32, bias=bias.to(DEV), act=True, y=y, y_coff=128)
    assert got is y
    _err(y[..., 128:256], F.relu(lin), tol, "channel offset")
    assert bool((y[..., :128] == SENTINEL).all()) and bool((y[..., 256:] == SENTINEL).all())


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_batch_and_position_do_not_change_the_bits(precision):
    f32 = precision == "f32"
    w = _rand(64, 64, 3, 3, seed=1) / 24.0
    x = _rand(3, 19, 28, 64, seed=2)
    both = _run(x, w, 3, 2, f32)
    alone = _run(x[2:3].contiguous(), w, 3, 2, f32)
    assert torch.equal(both[2:3], alone)


def test_stem_and_pool_at_odd_sizes(g):
    from e4s_amd import kernels as K
    x = _rand(2, 75, 109, 3, seed=1) * 60
    w = _rand(64, 3, 7, 7, seed=2) / 147 ** 0.5 / 60
    bias = _rand(64, seed=3)
    ref = F.relu(F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), stride=2, padding=3))
    assert tuple(ref.shape[2:]) == (38, 55)
    y = K.retina_stem(x.to(DEV), K.pack_smallcin(w).to(DEV), bias.to(DEV), torch.empty(2, 38, 55, 64, device=DEV))
    _err(y, ref.permute(0, 2, 3, 1), 1e-5, "stem 75x109 -> 38x55")
    pooled = K.retina_pool(y, torch.empty(2, 19, 28, 64, device=DEV))
    refp = F.max_pool2d(y.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert tuple(refp.shape[1:3]) == (19, 28) and torch.equal(pooled, refp.contiguous())
    refp64 = F.max_pool2d(ref, 3, 2, 1).permute(0, 2, 3, 1)
    _err(pooled, refp64, 1e-5, "pool 38x55 -> 19x28")


def test_prep_mean_subtraction_is_exact_and_the_shrink_matches_fp64(g):
    from e4s_amd import kernels as K
    f = synth.synth_retinaface_frame_u8(2, 75, 109, 5)
    out = K.retina_prep(f.to(DEV), torch.empty(2, 75, 109, 3, device=DEV)).cpu()
    assert torch.equal(out, f.float() - torch.tensor(MEAN))
    h, w, seed = g["frame_thin"]
    thin = synth.synth_retinaface_frame_u8(1, h, w, seed)
    hd, wd = g["thin.size"]
    out = K.retina_prep(thin.to(DEV), torch.empty(1, hd, wd, 3, device=DEV), scale=max(h, w) / 1000.0).cpu()
    got = out[0, g["thin.rows"]].double() + torch.tensor(MEAN, dtype=torch.float64)
    err = float((got - g["thin.values"]).abs().max())
    print(f"shrink err {err:.3e} bound {1e-5 * 255:.3e}")
    assert err <= 1e-5 * 255


@pytest.mark.parametrize("precision,_,tol", PRECISIONS)
def test_raw_network_on_frame_a_and_batch_invariance_on_frame_b(g, monkeypatch, precision, _, tol):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    det = _detector(g)
    h, w, seed = g["frame_A"]
    taps = {}
    loc, conf, lm = det.raw(synth.synth_retinaface_frame_u8(1, h, w, seed).to(DEV), taps=taps)
    cs = g["A.tap_cstep"]
    for name in ("layer2", "layer3", "layer4", "fpn1", "fpn2", "fpn3", "ssh1", "ssh2", "ssh3"):
        ref = g[f"A.tap.{name}"].double()
        got = taps[name][0].permute(2, 0, 1)[::cs].double().cpu()
        err, scale = float((got - ref).abs().max()), g[f"A.tap.{name}.scale"]
        print(f"{precision} {name}: err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
        assert err <= tol * scale, name
    assert tuple(loc.shape) == (1, 374, 4) and tuple(conf.shape) == (1, 374, 2) and tuple(lm.shape) == (1, 374, 10)
    _err(loc[0], g["A.loc"], tol, precision + " loc")
    _err(conf[0], g["A.conf"], tol, precision + " conf")
    _err(lm[0], g["A.landms"], tol, precision + " landms")
    h, w, seed = g["frame_B"]
    fb = synth.synth_retinaface_frame_u8(2, h, w, seed).to(DEV)
    both = det.raw(fb)
    alone = det.raw(fb[1:2].contiguous())
    for a, b, name in zip(both, alone, ("loc", "conf", "landms")):
        assert torch.equal(a[1:2], b), name
        _err(a, g["B." + name], tol, f"{precision} B {name}")


def _check_post(dets, lm, counts, case):
    n = int(counts[0])
    ref_d, ref_l = case["dets"].numpy(), case["lm"].numpy()
    assert n == len(ref_d), (case["name"], n, len(ref_d))
    d, l = dets[0, :n].cpu().numpy(), lm[0, :n].cpu().numpy()
    assert d.shape == ref_d.shape and l.shape == ref_l.shape
    if n:
        # the same set in the same order: every row's score matches its counterpart's, and the scores are pairwise distinct
        assert np.all(np.abs(d[:, 4] - ref_d[:, 4]) <= 1e-6), case["name"]
        assert np.all(np.abs(d[:, :4] - ref_d[:, :4]) <= 1e-4 + 1e-6 * np.abs(ref_d[:, :4])), case["name"]
        assert np.all(np.abs(l - ref_l) <= 1e-4 + 1e-6 * np.abs(ref_l)), case["name"]
    assert bool((dets[0, n:] == 0).all()) and bool((lm[0, n:] == 0).all())


def test_post_processing_cases_equal_the_reference(g):
    det = _detector(g)
    for case in g["post"]:
        dets, lm, counts = det.postprocess(case["loc"][None].to(DEV), case["conf"][None].to(DEV), case["landms"][None].to(DEV),
                                           g["frame_A"][:2], resize=case["resize"], confidence_threshold=case["thr"],
                                           nms_threshold=case["nms_thr"], top_k=case["top_k"], keep_top_k=case["keep_top_k"], ss=case["ss"])
        assert tuple(dets.shape) == (1, case["keep_top_k"], 5) and tuple(lm.shape) == (1, case["keep_top_k"], 10)
        _check_post(dets, lm, counts, case)
        if case["name"] == "ii":
            assert int(counts[0]) == 0 and dets[0, :0].shape == (0, 5) and lm[0, :0].shape == (0, 10)
    # a batch of two different cases gives each image its own answer
    a, b = g["post"][0], g["post"][3]
    dets, lm, counts = det.postprocess(torch.stack([a["loc"], b["loc"]]).to(DEV), torch.stack([a["conf"], b["conf"]]).to(DEV),
                                       torch.stack([a["landms"], b["landms"]]).to(DEV), g["frame_A"][:2])
    _check_post(dets[:1], lm[:1], counts[:1], a)
    assert int(counts[1]) == len(b["dets"])


def test_end_to_end_detect_composition_allocation_and_face_restorer(g, monkeypatch):
    from e4s_amd import kernels as K
    from e4s_amd.face_paste import FaceRestorer
    monkeypatch.setattr(K, "PRECISION", "f32")
    det = _detector(g)
    h, w, seed = g["frame_A"]
    frame = synth.synth_retinaface_frame_u8(1, h, w, seed)[0]
    d_np, l_np = det.detect(frame.numpy())
    dets, lm, counts = det.detect_device(frame.to(DEV))
    n = int(counts[0])
    assert n > 0 and d_np.dtype == np.float32 and d_np.shape == (n, 5) and l_np.shape == (n, 10)
    assert np.array_equal(d_np, dets[0, :n].cpu().numpy()) and np.array_equal(l_np, lm[0, :n].cpu().numpy())
    # the detector is the composition of the two tested halves
    loc, conf, lms = det.raw(frame.to(DEV))
    d2, l2, c2 = det.postprocess(loc, conf, lms, (h, w))
    assert int(c2[0]) == n and torch.equal(d2, dets) and torch.equal(l2, lm)
    # a second call at the shape allocates nothing but its results
    fd = frame.to(DEV)
    det.detect_device(fd)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    res = det.detect_device(fd)
    torch.cuda.synchronize()
    extra = torch.cuda.memory_allocated() - before
    assert extra <= sum(-(-t.numel() * t.element_size() // 512) * 512 for t in res), extra
    # FaceRestorer asks the detector when it gets no boxes
    class Parser:
        def masks(self, faces, bgr=True):
            return torch.full(faces.shape[:3], 255, device=faces.device, dtype=torch.uint8)
    big = synth.synth_retinaface_frame_u8(1, 96, 128, 9)[0].to(DEV)
    bd, bl = det.detect(big.cpu().numpy())
    assert len(bd) > 0
    thr = float(np.sort(bd[:, 4])[-min(2, len(bd))])                       # the two best faces only: the paste is not under test here
    fr = FaceRestorer(lambda x: x, Parser(), in_size=512, threshold=thr, detector=det)
    got = fr.process(big)
    want = fr.process(big, bd, bl)
    assert len(bd) > 0 and all(torch.equal(a, b) for a, b in zip(got, want))
