"""GPU tests of the face-swap pipeline (e4s_amd/pipeline.py) and its four join kernels (csrc/pipeline.hip) against the host statements
of tests/pipeline_cases.py (checked on their own in tests/test_pipeline_cases_host.py)."""
import numpy as np
import pytest
import torch

import pipeline_cases as pc
from e4s_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _img(h, w, seed, b=None):
    shape = (h, w, 3) if b is None else (b, h, w, 3)
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- resize_aa4 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 12), (40, 72), (1024, 1024)])
def test_resize_aa4_against_the_fp64_statement(shape):
    """8 x 12: every output touches both mirrors; 40 x 72: crosses 16 x 16 tile edges, not square; 1024^2: the pipeline's size (the
    whole-dword staging path).  Bound 5e-6: 28 fp32 multiply-adds on [0,1], worst case 28 x 2^-24 = 1.7e-6, a factor 3 of margin."""
    b = 1 if shape[0] == 1024 else 2
    imgs = _img(*shape, seed=11, b=b)
    got = K.resize_aa4(_dev(imgs))
    assert got.dtype == torch.float32 and tuple(got.shape) == (b, shape[0] // 4, shape[1] // 4, 3)
    for i in range(b):
        want = pc.resize_aa4_closed(imgs[i]) if shape[0] == 1024 else pc.resize_aa4_scipy(imgs[i])
        err = float(np.abs(got[i].cpu().numpy().astype(np.float64) - want).max())
        print(f"resize_aa4 {shape} sample {i}: max err {err:.2e}")
        assert err <= 5e-6
    if b == 2:                                                 # a batch of 2 gives each sample the bits of a batch of 1
        for i in range(2):
            assert torch.equal(K.resize_aa4(_dev(imgs[i:i + 1]))[0], got[i])


def test_resize_aa4_refuses_sizes_a_single_mirror_cannot_serve():
    with pytest.raises(ValueError):
        K.resize_aa4(_dev(_img(10, 12, seed=1, b=1)))
    with pytest.raises(ValueError):
        K.resize_aa4(_dev(_img(4, 12, seed=1, b=1)))
    with pytest.raises(ValueError):
        K.resize_aa4(_dev(_img(8, 12, seed=1, b=1)).float())
    with pytest.raises(RuntimeError):
        K.resize_aa4(torch.from_numpy(_img(8, 12, seed=1, b=1)))


# ---- driven_seam ---------------------------------------------------------------------------------------------------------
def _pred(n, h, w, seed):
    """[N,3,h,w] in [0,1] with exact k / 255 values, 0 and 1 among random ones."""
    rng = np.random.RandomState(seed)
    p = rng.rand(n, 3, h, w).astype(np.float32)
    flat = p.reshape(-1)
    flat[::3] = (rng.randint(0, 256, size=flat[::3].size) / 255.0).astype(np.float32)
    flat[1], flat[4], flat[-1], flat[-2] = 0.0, 1.0, 1.0, 0.0
    return p


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("shape", [(5, 7), (16, 20), (256, 256)])
def test_driven_seam_is_bit_equal_to_the_numpy_statements(shape, n):
    p = _pred(n, *shape, seed=21)
    want_u8 = np.ascontiguousarray(pc.truncate_u8(p.transpose(0, 2, 3, 1))[..., ::-1])
    want_big = np.stack([pc.cv_resize_x4(f) for f in want_u8])
    assert (np.rint(p * np.float32(255)).astype(np.uint8) != pc.truncate_u8(p)).any()         # truncation is not rounding here
    assert (want_big != np.stack([pc.bilinear_x4_rounded(f) for f in want_u8])).any()         # nor is the enlargement exact
    got_u8, got_big = K.driven_seam(_dev(p))
    assert got_u8.dtype == torch.uint8 and np.array_equal(got_u8.cpu().numpy(), want_u8)
    assert tuple(got_big.shape) == (n, 4 * shape[0], 4 * shape[1], 3) and np.array_equal(got_big.cpu().numpy(), want_big)
    only, none = K.driven_seam(_dev(p), enlarge=False)                                          # the second output is optional
    assert none is None and torch.equal(only, got_u8)


# ---- face_to_net ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("size", [6, 1024])
def test_face_to_net_is_bit_equal_to_the_torch_cpu_statement(size, bgr):
    imgs = _img(size, size, seed=31, b=2 if size == 6 else 1)
    rgb = np.ascontiguousarray(imgs[..., ::-1]) if bgr else imgs
    got_rgb, got_net = K.face_to_net(_dev(imgs), bgr=bgr)
    assert np.array_equal(got_rgb.cpu().numpy(), rgb)
    assert torch.equal(got_net.cpu(), pc.to_net_torch(rgb))
    none, net_only = K.face_to_net(_dev(imgs), bgr=bgr, rgb=False)
    rgb_only, none2 = K.face_to_net(_dev(imgs), bgr=bgr, net=False)
    assert none is None and none2 is None and torch.equal(net_only, got_net) and torch.equal(rgb_only, got_rgb)


def test_face_to_net_into_a_slice_of_a_larger_buffer_touches_nothing_else():
    """GraphedFaceSwap.static lays driven | target out back to back in one buffer; the target half starts at a non-zero offset."""
    b, s = 2, 10
    imgs = _img(s, s, seed=32, b=b)
    buf = torch.full((2 * b + 1, 3, s, s), 7.5, device=DEV)
    K.face_to_net(_dev(imgs), rgb=False, out_net=buf[b:2 * b])
    assert torch.equal(buf[b:2 * b].cpu(), pc.to_net_torch(imgs))
    assert bool((buf[:b] == 7.5).all()) and bool((buf[2 * b:] == 7.5).all())
    with pytest.raises(ValueError):
        K.face_to_net(_dev(imgs), rgb=False, out_net=buf[:b + 1])


# ---- the pipeline with stub stages at the real sizes -----------------------------------------------------------------------
def _square_quad(cx, cy, half, deg):
    """nw, sw, se, ne of a square turned by deg degrees (as align.compute_quad orders them)."""
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    x, y = np.array([c, s]) * half, np.array([-s, c]) * half
    ctr = np.array([cx, cy], dtype=np.float64)
    return np.stack([ctr - x - y, ctr - x + y, ctr + x + y, ctr + x - y])


def _scene(b, quads):
    """Smooth-ish frames (so that parsing classes form regions) with noise on top: a 900 x 1000 source and 1280 x 1100 targets with
    quads, or 1024^2 faces without."""
    rng = np.random.RandomState(41)

    def frame(h, w):
        base = np.kron(rng.randint(0, 256, size=(h // 20 + 1, w // 20 + 1, 3)), np.ones((20, 20, 1)))[:h, :w]
        return np.clip(base + rng.randint(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)
    if not quads:
        return _dev(frame(1024, 1024)), _dev(np.stack([frame(1024, 1024) for _ in range(b)])), None, None
    sq = _square_quad(480.0, 450.0, 330.0, -7.0)
    tq = np.stack([_square_quad(560.0 + 30 * i, 600.0 - 25 * i, 400.0 - 30 * i, 9.0 + 4 * i) for i in range(b)])
    return _dev(frame(900, 1000)), _dev(np.stack([frame(1280, 1100) for _ in range(b)])), sq, tq


@pytest.mark.parametrize("quads", [False, True])
@pytest.mark.parametrize("b", [1, 2])
def test_pipeline_with_stub_stages_is_bit_equal_to_the_steps_by_hand(b, quads):
    from e4s_amd.pipeline import TAPS, FaceSwapPipeline
    stages = pc.stub_stages()
    src, tgt, sq, tq = _scene(b, quads)
    pipe = FaceSwapPipeline(*stages, batch=1 if quads else b, graph=False)          # with quads and b = 2: two chunks of one
    taps = {}
    got = pipe.swap(src, tgt, source_quad=sq, target_quads=tq, taps=taps)
    want, ref = pc.compose(stages, src, tgt, source_quad=sq, target_quads=tq)
    assert got.dtype == torch.uint8 and got.shape == tgt.shape
    assert set(taps) == set(TAPS)
    for k in TAPS:
        assert taps[k].shape == ref[k].shape and torch.equal(taps[k], ref[k]), k
    assert torch.equal(got, want)
    # the resize, the one join defined to a tolerance: compose carries the fp64 statement beside the kernel's values
    for k in ("S_256", "T_256"):
        err = float(np.abs(taps[k].cpu().numpy().astype(np.float64) - ref[k + "_f64"]).max())
        print(f"{k}: max err vs fp64 {err:.2e}")
        assert err <= 5e-6
    # the test can tell the rules apart
    pred, pred_bgr = ref["pred"], ref["pred_bgr"].cpu().numpy()
    assert (np.rint(pred * np.float32(255)).astype(np.uint8) != pc.truncate_u8(pred)).any()
    assert (ref["enlarged"][0].cpu().numpy() != pc.bilinear_x4_rounded(pred_bgr[0])).any()
    # every stage left a mark: the swap changed the face, the classes are mixed, and with quads the frame outside them is untouched
    assert len(torch.unique(taps["swapped_labels"])) > 4
    if quads:
        changed = (got != tgt).any(-1)
        assert bool(changed.any()) and not bool(changed.all())
        ys, xs = np.mgrid[0:tgt.shape[1], 0:tgt.shape[2]]
        for i in range(b):
            c = tq[i].mean(0)
            far = torch.from_numpy(np.hypot(xs - c[0], ys - c[1]) > np.hypot(*(tq[i][0] - c)) + 2).to(DEV)   # outside the quad's circle
            assert bool(far.any()) and torch.equal(got[i][far], tgt[i][far])
    else:
        assert not torch.equal(got, tgt)


def test_pipeline_refuses_bad_arguments_before_any_launch():
    from e4s_amd.pipeline import FaceSwapPipeline
    pipe = FaceSwapPipeline(*pc.stub_stages(), graph=False)
    face = torch.zeros(1024, 1024, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        pipe.swap(face.cpu(), face[None])
    with pytest.raises(RuntimeError):
        pipe.swap(face, face[None].cpu())
    with pytest.raises(ValueError):
        pipe.swap(face.float(), face[None])
    with pytest.raises(ValueError):
        pipe.swap(face, face)                                               # targets are a batch
    with pytest.raises(ValueError):
        pipe.swap(face, face[None, :512])                                   # un-cropped frames without quads
    with pytest.raises(ValueError):
        pipe.swap(face, face[None], source_quad=_square_quad(500, 500, 300, 0))
    with pytest.raises(ValueError):
        pipe.swap(face, face[None], target_labels=torch.zeros(1, 256, 256, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        FaceSwapPipeline(*pc.stub_stages(), graph=True)                     # a callable swap cannot be captured


# ---- the real Net3 (synthetic weights) between stubbed stages --------------------------------------------------------------
@torch.no_grad()
def test_pipeline_with_the_real_net_graph_replay_equals_eager():
    from e4s_amd import synth
    from e4s_amd.networks import Net3
    from e4s_amd.options import make_opts
    from e4s_amd.pipeline import FaceSwapPipeline
    net = Net3(make_opts(out_size=1024))
    net.load_state_dict(synth.synth_state_dict(1024, 13), strict=True)
    net.latent_avg = synth.synth_latent_avg(1024).to(DEV)
    net = net.to(DEV).eval()
    _, reenactor, sr, restorer, parser = pc.stub_stages()
    graphed = FaceSwapPipeline(net, reenactor, sr, restorer, parser, batch=1, graph=True)
    eager = FaceSwapPipeline(net, reenactor, sr, restorer, parser, batch=1, graph=False, noise=graphed.noise)
    src, tgt, _, _ = _scene(2, False)
    t1, t2 = {}, {}
    out_g = graphed.swap(src, tgt, taps=t1)                                 # two replays of the batch-1 graph
    out_e = eager.swap(src, tgt, taps=t2)
    assert torch.equal(t1["swapped_face"], t2["swapped_face"]) and torch.equal(out_g, out_e)
    assert not torch.equal(out_g[0], out_g[1]) and not torch.equal(out_g, tgt)
    # different frames through the captured graph: its static inputs are really rewritten (no stale buffer)
    src2, tgt2 = tgt[1].clone(), torch.stack([src, tgt[0]])
    out_g2 = graphed.swap(src2, tgt2)
    assert torch.equal(out_g2, eager.swap(src2, tgt2)) and not torch.equal(out_g2, out_g)
    graphed.validate()
    assert graphed.graphed is not None and graphed.graphed.graph is not None
    # a partial final chunk (1 target for a batch-2 swap) runs eagerly, with the same bits, and captures nothing
    partial = FaceSwapPipeline(net, reenactor, sr, restorer, parser, batch=2, graph=True)
    assert torch.equal(partial.swap(src, tgt[:1]), out_e[:1]) and partial.graphed is None
