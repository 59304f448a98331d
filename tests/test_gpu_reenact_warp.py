"""GPU tests of face-vid2vid's dense motion and 3-D feature warp (e4s_amd/reenact_warp.py, csrc/vid2vid.hip, csrc/vid2vid_warp.hip)
against the REAL reference's fp64 records (tests/golden/reenact_warp.pt, tests/golden/make_reenact_warp_golden.py) and fp64 torch
restatements of the single kernels.

Bounds (those of test_gpu_reenact.py): a single layer 1e-5 x scale (f32) and 1e-3 x scale (bf16x3); a whole network, up to the mask
logits, the hourglass prediction or the occlusion logit, 1e-4 x scale and 1e-3 x scale; scale = max |fp64 reference|.  The
streaming kernels (sampling, soft-max, reductions) are fp32 in either mode: 1e-5 x scale.

What follows a softmax or a sampling has no free tolerance:
    hg_input      a trilinear sample is a convex combination, so it moves by at most the compressed volume's error (the network
                  bound x its scale); the coordinates come from the exact keypoints, so only the kernel's own 1e-5 x scale is added
    mask          if every logit is within delta of the reference's, every weight changes by a factor within e^{+-2 delta}; weights
                  are <= 1, so |d mask| <= e^{2 delta} - 1, delta = the logit bound applied
    deformation   sum_k mask_k motion_k with sum_k mask_k = 1: |d| <= (e^{2 delta} - 1) max |sparse motion| (recorded by the maker),
                  plus the kernel's own 1e-5 x that
    occlusion     sigmoid is 1/4-Lipschitz: 0.25 x the network bound x max |logit(occlusion_map)|
    warped        a sample under a grid that moved by d_g: an index moves by d_g n_axis / 2, and the volume changes by at most
                  lip_axis per voxel (recorded), so |d| <= the volume's error + sum_axis d_g (n_axis / 2) lip_axis (+ 1e-5 x scale)
    third,        linear layers behind the sample: |d third| <= d_warped x the largest absolute row sum of third's folded weight
    feature       (LeakyReLU is 1-Lipschitz) + the layer bound; the same through fourth; feature = fourth x occlusion moves by at most
                  d_fourth + max |fourth| d_occlusion, max |fourth| <= rowsum(fourth) max |third| + max |bias|.
The propagated bound on third and feature is rigorous and LOOSE (two row sums of ~10 .. 40 on top of the sample's bound): it can
exceed the maps' own scale, so it shows consistency with the reference and little else.  The sharp check of those two layers, their
channel permutation and the occlusion product is test_tail_from_the_native_warped_map: fp64 recomputed from the native warped map
and occlusion, at the single-layer bound."""
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
VOLUMES = [(4, 6, 5), (16, 8, 8)]
_STATE = {}


@pytest.fixture(scope="module")
def g(golden):
    return golden("reenact_warp.pt")


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


def _conv3d_64(x, w, bias=None, up2=False, relu=False, res=None):
    """x [B,D,H,W,C] -> [B,D,Ho,Wo,Cout] in fp64; the padding is w's k / 2"""
    x = x.double().permute(0, 4, 1, 2, 3)
    if up2:
        x = F.interpolate(x, scale_factor=(1, 2, 2))
    y = F.conv3d(x, w.double(), None if bias is None else bias.double(), padding=w.shape[-1] // 2).permute(0, 2, 3, 4, 1)
    if res is not None:
        y = y + res.double()
    return F.relu(y) if relu else y


def _grid64(d, h, w):
    ax = lambda n: 2 * (torch.arange(n, dtype=torch.float64) / (n - 1)) - 1
    z, y, x = torch.meshgrid(ax(d), ax(h), ax(w), indexing="ij")
    return torch.stack([x, y, z], -1)


def _sparse_motions64(d, h, w, kps, kpd, jac):
    """[N,K+1,D,H,W,3] as create_sparse_motions builds them; jac = J_source inverse(J_driving) [N,K,3,3] or None"""
    n, k = kpd.shape[:2]
    grid = _grid64(d, h, w).view(1, 1, d, h, w, 3)
    c = grid - kpd.double().view(n, k, 1, 1, 1, 3)
    if jac is not None:
        c = torch.matmul(jac.double().view(n, k, 1, 1, 1, 3, 3), c.unsqueeze(-1)).squeeze(-1)
    c = c + kps.double().expand(n, k, 3).reshape(n, k, 1, 1, 1, 3)
    return torch.cat([grid.expand(n, 1, d, h, w, 3), c], 1)


def _hg_input64(feat, kps, kpd, jac, variance=0.01):
    """feat [1|N,D,H,W,4] -> [N,D,H,W,5 (K+1)]: dense_motion.py:71-106 in fp64"""
    n, k = kpd.shape[:2]
    _, d, h, w, c = feat.shape
    sm = _sparse_motions64(d, h, w, kps, kpd, jac)
    f = feat.double().permute(0, 4, 1, 2, 3).expand(n, c, d, h, w)
    rep = f.unsqueeze(1).expand(n, k + 1, c, d, h, w).reshape(n * (k + 1), c, d, h, w)
    samp = F.grid_sample(rep, sm.reshape(n * (k + 1), d, h, w, 3), align_corners=False).view(n, k + 1, c, d, h, w)
    grid = _grid64(d, h, w).view(1, 1, d, h, w, 3)
    gauss = lambda kp: torch.exp(-0.5 * ((grid - kp.double().expand(n, k, 3).reshape(n, k, 1, 1, 1, 3)) ** 2).sum(-1) / variance)
    heat = torch.cat([torch.zeros(n, 1, d, h, w, dtype=torch.float64), gauss(kpd) - gauss(kps)], 1)
    return torch.cat([heat.unsqueeze(2), samp], 2).view(n, (k + 1) * (c + 1), d, h, w).permute(0, 2, 3, 4, 1)


def _kps(n, k, seed, spread=0.8, jac=False):
    kps = (torch.rand(1, k, 3, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * spread
    kpd = kps + 0.3 * _rand(n, k, 3, seed=seed + 1)
    if not jac:
        return kps, kpd, None, None
    eye = torch.eye(3).view(1, 1, 3, 3)
    return kps, kpd, eye + 0.2 * _rand(1, k, 3, 3, seed=seed + 2), eye + 0.2 * _rand(n, k, 3, 3, seed=seed + 3)


# ---- the 3-D conv family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vol", VOLUMES)
@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
def test_conv3dx_forms_match_fp64_with_guard_bands(precision, tol, _, vol):
    from e4s_amd import kernels as K
    f32 = precision == "f32"
    d, h, w = vol
    b = 2
    guard = _GuardedTorch()
    # Cin 80 through a stride padded to 96 (a slice of a 128-wide concat buffer whose pad channels are zero), output into a channel slice
    cat = torch.zeros(b, d, h, w, 128)
    cat[..., 32:112] = _rand(b, d, h, w, 80, seed=1)
    cat[..., :32] = 7.0                                                      # the neighbouring slice must not be read
    wt, bias = _rand(64, 80, 3, 3, 3, seed=2) / math.sqrt(27 * 80), _rand(64, seed=3)
    y = guard.empty(b, d, h, w, 128, device=DEV)
    K.conv3dx(cat.to(DEV)[..., 32:128], K.conv3dx_pack(wt.to(DEV), f32, cin_pad=96), 64, y, y_coff=64, bias=bias.to(DEV), relu=True, f32=f32)
    guard.check()
    assert unwritten(y[..., 64:]) == 0 and unwritten(y[..., :64]) == y[..., :64].numel()
    _err(y[..., 64:], _conv3d_64(cat[..., 32:112], wt, bias, relu=True), tol, f"{precision} {vol} Cin 80 -> slice 64:128")
    # Cin 112 through a stride of 128, Cout 112 into a 128-wide buffer
    x = torch.zeros(b, d, h, w, 128)
    x[..., :112] = _rand(b, d, h, w, 112, seed=4)
    wt = _rand(112, 112, 3, 3, 3, seed=5) / math.sqrt(27 * 112)
    y = guard.empty(b, d, h, w, 128, device=DEV)
    K.conv3dx(x.to(DEV), K.conv3dx_pack(wt.to(DEV), f32, cin_pad=128), 112, y, f32=f32)
    guard.check()
    assert unwritten(y[..., :112]) == 0 and unwritten(y[..., 112:]) == y[..., 112:].numel()
    _err(y[..., :112], _conv3d_64(x[..., :112], wt), tol, f"{precision} {vol} Cin 112 -> 112")
    # ResBlock3d: norm1 + ReLU as a streaming launch (the padding is an exact zero, not relu(shift)), conv, residual from a strided view
    flat = _rand(b, h, w, d * 32, seed=6)
    xs = flat.view(b, h, w, d, 32).permute(0, 3, 1, 2, 4)                    # [B,D,H,W,32] through strides
    scale, shift = 1 + 0.1 * _rand(32, seed=7), 0.5 + 0.1 * _rand(32, seed=8)   # relu(shift) > 0: a padded tap that went through the prologue would show
    wt, bias = _rand(32, 32, 3, 3, 3, seed=9) / math.sqrt(27 * 32), _rand(32, seed=10)
    xs_dev = flat.to(DEV).view(b, h, w, d, 32).permute(0, 3, 1, 2, 4)
    a = K.bnrelu3d(xs_dev, scale.to(DEV), shift.to(DEV), guard.empty(b, d, h, w, 32, device=DEV))
    guard.check()
    a64 = F.relu(xs.double() * scale.double() + shift.double())
    _err(a, a64, STREAM_TOL, f"{vol} norm1 + ReLU")
    y = guard.empty(b, d, h, w, 32, device=DEV)
    K.conv3dx(a, K.conv3dx_pack(wt.to(DEV), f32), 32, y, bias=bias.to(DEV), res=xs_dev, f32=f32)
    guard.check()
    assert unwritten(y) == 0
    _err(y, _conv3d_64(a64, wt, bias, res=xs), tol, f"{precision} {vol} pre-activation block with its residual")
    # batch-1 broadcast: one input, three outputs, each the single-sample result
    one = _rand(1, d, h, w, 32, seed=11)
    y3 = guard.empty(3, d, h, w, 32, device=DEV)
    K.conv3dx(one.to(DEV), K.conv3dx_pack(wt.to(DEV), f32), 32, y3, bias=bias.to(DEV), relu=True, f32=f32)
    guard.check()
    _err(y3[2:3], _conv3d_64(one, wt, bias, relu=True), tol, f"{precision} {vol} broadcast")
    assert torch.equal(y3[0], y3[1]) and torch.equal(y3[0], y3[2])
    # ksize 1 (compress): 32 -> 4
    w1, b1 = _rand(4, 32, 1, 1, 1, seed=12) / math.sqrt(32), _rand(4, seed=13)
    y = guard.empty(1, d, h, w, 4, device=DEV)
    K.conv3dx(one.to(DEV), K.conv3dx_pack(w1.to(DEV), f32), 4, y, bias=b1.to(DEV), relu=True, f32=f32)
    guard.check()
    assert unwritten(y) == 0
    _err(y, _conv3d_64(one, w1, b1, relu=True), tol, f"{precision} {vol} 1x1x1")
    # an up block into the first channels of its concat buffer
    wu = _rand(32, 32, 3, 3, 3, seed=14) / math.sqrt(27 * 32)
    y = guard.empty(1, d, 2 * h, 2 * w, 96, device=DEV)
    K.conv3dx(one.to(DEV), K.conv3dx_pack(wu.to(DEV), f32), 32, y, relu=True, up2=True, f32=f32)
    guard.check()
    assert unwritten(y[..., :32]) == 0 and unwritten(y[..., 32:]) == y[..., 32:].numel()
    _err(y[..., :32], _conv3d_64(one, wu, up2=True, relu=True), tol, f"{precision} {vol} up block into a slice")


@pytest.mark.parametrize("vol", [(4, 5, 7), (16, 8, 6)])
@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
def test_conv7_matches_fp64_where_every_voxel_has_taps_outside(precision, tol, _, vol):
    from e4s_amd import kernels as K
    f32 = precision == "f32"
    d, h, w = vol
    x = torch.zeros(2, d, h, w, 128)
    x[..., :112] = _rand(2, d, h, w, 112, seed=20)
    wt, bias = _rand(16, 112, 7, 7, 7, seed=21) / math.sqrt(343 * 112), _rand(16, seed=22)
    guard = _GuardedTorch()
    y = guard.empty(2, d, h, w, 16, device=DEV)
    K.conv3dx(x.to(DEV), K.conv3dx_pack(wt.to(DEV), f32, cin_pad=128), 16, y, bias=bias.to(DEV), f32=f32)
    guard.check()
    assert unwritten(y) == 0
    _err(y, _conv3d_64(x[..., :112], wt, bias), tol, f"{precision} 7x7x7 on {vol}")


def test_conv3dx_refuses_what_it_cannot_take():
    from e4s_amd import kernels as K
    x, y = torch.zeros(1, 2, 3, 3, 32, device=DEV), torch.empty(1, 2, 3, 3, 32, device=DEV)
    with pytest.raises(RuntimeError):
        K.conv3dx_pack(torch.zeros(8, 32, 5, 5, 5, device=DEV), True)       # ksize 5
    with pytest.raises(RuntimeError):
        K.conv3dx_pack(torch.zeros(8, 80, 3, 3, 3, device=DEV), True)       # Cin 80 without a padded stride
    wp = K.conv3dx_pack(torch.zeros(32, 32, 3, 3, 3, device=DEV), True)
    with pytest.raises(RuntimeError):
        K.conv3dx(x, wp, 32, y, y_coff=2, f32=True)                          # a slice that is not 16-byte aligned
    with pytest.raises(RuntimeError):
        K.conv3dx(x, wp, 32, y, f32=False)                                   # a pack of the other precision
    with pytest.raises(RuntimeError):
        K.conv3dx(x, wp, 32, y, res=torch.zeros(1, 2, 3, 4, 32, device=DEV), f32=True)
    w7 = K.conv3dx_pack(torch.zeros(32, 32, 7, 7, 7, device=DEV), True)
    with pytest.raises(RuntimeError):
        K.conv3dx(x, w7, 32, torch.empty(1, 2, 6, 6, 32, device=DEV), up2=True, f32=True)      # the up-sampling goes with ksize 3


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_new_convs_batch_and_position_do_not_change_the_bits(precision):
    from e4s_amd import kernels as K
    f32 = precision == "f32"
    a, other = torch.zeros(1, 5, 9, 7, 128), torch.zeros(1, 5, 9, 7, 128)
    a[..., :112], other[..., :112] = _rand(1, 5, 9, 7, 112, seed=3), _rand(1, 5, 9, 7, 112, seed=4)
    res = _rand(3, 5, 9, 7, 16, seed=5)
    for k in (7, 3):
        wt, bias = _rand(16, 112, k, k, k, seed=1) / math.sqrt(k ** 3 * 112), _rand(16, seed=2)
        wp = K.conv3dx_pack(wt.to(DEV), f32, cin_pad=128)

        def run(x, r):
            y = torch.zeros(x.shape[0], 5, 9, 7, 32, device=DEV)
            return K.conv3dx(x.to(DEV), wp, 16, y, y_coff=16, bias=bias.to(DEV), res=r.to(DEV), relu=True, f32=f32)[..., 16:]
        alone, three = run(a, res[:1]), run(torch.cat([a, other, a]), torch.cat([res[:1], res[1:2], res[:1]]))
        assert torch.equal(three[0], alone[0]) and torch.equal(three[2], alone[0])
        assert not torch.equal(three[1], alone[0])
        # a voxel's bits do not depend on its place in the tile: the same volume behind 3 more depth planes of other data
        if k == 3:
            continue
        deep = torch.cat([other[:, :3], a], 1)                               # a's planes at depth 3 .. 7 see other data 3 planes away
        # the last plane of `a` is 4 planes from `other`: its 7-deep window (3 either way) never reaches it
        yd = K.conv3dx(deep.to(DEV), wp, 16, torch.zeros(1, 8, 9, 7, 16, device=DEV), bias=bias.to(DEV), f32=f32)
        ya = K.conv3dx(a.to(DEV), wp, 16, torch.zeros(1, 5, 9, 7, 16, device=DEV), bias=bias.to(DEV), f32=f32)
        assert torch.equal(yd[0, 7], ya[0, 4]) and torch.equal(yd[0, 6], ya[0, 3])


# ---- the streaming kernels -------------------------------------------------------------------------------------------------------------
def test_avgpool_into_a_slice_scale_rows_and_kp_jacobian():
    from e4s_amd import kernels as K, reenact_warp as rw
    guard = _GuardedTorch()
    x = _rand(6, 9, 7, 64, seed=40)                                          # B D = 6 planes, odd sizes drop the last row and column
    y = guard.empty(6, 4, 3, 128, device=DEV)
    K.avgpool2_into(x.to(DEV), 64, y, 64)
    guard.check()
    assert unwritten(y[..., 64:]) == 0 and unwritten(y[..., :64]) == y[..., :64].numel()
    _err(y[..., 64:], F.avg_pool2d(x.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), STREAM_TOL, "avgpool into a slice")
    m, rows = _rand(5, 3, seed=41), _rand(5, 3, 8, seed=42)
    out = guard.place(rows)
    K.scale_rows(out, m.to(DEV))
    guard.check()
    _err(out, rows.double() * m.double().unsqueeze(-1), STREAM_TOL, "scale_rows")
    _, _, js, jd = _kps(3, 15, 43, jac=True)
    for src in (js, js.expand(3, 15, 3, 3).contiguous()):
        got = K.kp_jacobian(src.to(DEV), jd.to(DEV), guard.empty(3, 15, 3, 3, device=DEV))
        guard.check()
        _err(got, src.double() @ torch.inverse(jd.double()), STREAM_TOL, "J_source inverse(J_driving)")
    assert float((rw.inverse3x3(jd.double()) - torch.inverse(jd.double())).abs().max()) < 1e-12


@pytest.mark.parametrize("jac", [False, True])
@pytest.mark.parametrize("vol", [(3, 6, 5), (4, 16, 12)])
def test_sparse_warp_matches_grid_sample_fp64(vol, jac):
    """D = 3: the identity grid's middle plane lands exactly on a voxel centre (index 1 n / (n - 1) - 1 / 2 = 1); keypoints near +-0.8
    with offsets of 0.3 x randn push most grids outside [-1, 1] somewhere."""
    from e4s_amd import kernels as K
    d, h, w = vol
    n, k = 2, 15
    kps, kpd, js, jd = _kps(n, k, 50 + d, jac=jac)
    feat = _rand(1, d, h, w, 4, seed=51)
    jmat = js.double() @ torch.inverse(jd.double()) if jac else None
    sm = _sparse_motions64(d, h, w, kps, kpd, jmat)
    assert float(sm.abs().max()) > 1.2 and bool((sm.abs() <= 1).all(-1).any())
    guard = _GuardedTorch()
    jdev = K.kp_jacobian(js.to(DEV), jd.to(DEV)) if jac else None
    y = guard.empty(n, d, h, w, 128, device=DEV)
    K.sparse_warp(feat.to(DEV), kps.to(DEV), kpd.to(DEV), jdev, y, y_coff=32)
    guard.check()
    assert unwritten(y[..., 32:112]) == 0 and unwritten(y[..., :32]) == y[..., :32].numel() and unwritten(y[..., 112:]) == y[..., 112:].numel()
    ref = _hg_input64(feat, kps, kpd, jmat)
    _err(y[..., 32:112], ref, STREAM_TOL, f"sparse warp {vol} jac={jac}")
    # a per-sample compressed volume and per-sample source keypoints give the same as the broadcast ones
    y2 = torch.empty(n, d, h, w, 80, device=DEV)
    K.sparse_warp(feat.expand(n, d, h, w, 4).contiguous().to(DEV), kps.expand(n, k, 3).contiguous().to(DEV), kpd.to(DEV), jdev, y2)
    assert torch.equal(y2, y[..., 32:112])


@pytest.mark.parametrize("jac", [False, True])
def test_motion_combine_matches_fp64(jac):
    from e4s_amd import kernels as K
    n, k, (d, h, w) = 2, 15, (4, 7, 5)
    kps, kpd, js, jd = _kps(n, k, 60, jac=jac)
    logits = torch.zeros(n, d, h, w, 32)
    logits[..., :16] = 2 * _rand(n, d, h, w, 16, seed=61)
    logits[..., 16:] = 50.0                                                  # channels past K + 1 are not part of the softmax
    jmat = js.double() @ torch.inverse(jd.double()) if jac else None
    guard = _GuardedTorch()
    mask, deform = K.motion_combine(logits.to(DEV), kps.to(DEV), kpd.to(DEV), K.kp_jacobian(js.to(DEV), jd.to(DEV)) if jac else None,
                                    guard.empty(n, d, h, w, 16, device=DEV), guard.empty(n, d, h, w, 3, device=DEV))
    guard.check()
    assert unwritten(mask) == 0 and unwritten(deform) == 0
    m64 = torch.softmax(logits[..., :16].double(), -1)
    sm = _sparse_motions64(d, h, w, kps, kpd, jmat)                          # [N,16,D,H,W,3]
    _err(mask, m64, STREAM_TOL, f"mask jac={jac}")
    _err(deform, (sm * m64.permute(0, 4, 1, 2, 3).unsqueeze(-1)).sum(1), STREAM_TOL, f"deformation jac={jac}")
    assert float((mask.sum(-1) - 1).abs().max()) <= 1e-5


def test_warp3d_matches_grid_sample_fp64():
    from e4s_amd import kernels as K
    d, h, w, c, n = 4, 8, 5, 32, 2                                          # centres with exact fp32 coordinates: x 2 of 5, y 3 of 8, z 1 of 4
    flat = _rand(1, h, w, d * c, seed=70)
    vol = flat.view(1, h, w, d, c).permute(0, 3, 1, 2, 4)                    # a strided volume, as `second` leaves it
    grid = 1.4 * (torch.rand(n, d, h, w, 3, generator=torch.Generator().manual_seed(71)) * 2 - 1)      # about 30 % outside per axis
    centre = lambda i, m: (2 * i + 1) / m - 1                                # the coordinate that lands exactly on voxel i of m
    grid[0, 0, 0, 0] = torch.tensor([centre(2, w), centre(3, h), centre(1, d)])
    grid[0, 0, 0, 1] = torch.tensor([centre(0, w), centre(0, h), centre(0, d)])
    grid[0, 0, 0, 2] = torch.tensor([centre(w - 1, w), centre(h - 1, h), centre(d - 1, d)])
    grid[0, 0, 0, 3] = torch.tensor([-1.0, 1.0, -1.0])                       # the volume's corner: half a voxel outside the first centre
    grid[0, 0, 0, 4] = torch.tensor([5.0, -7.0, 1e9])
    assert 0.1 < float((grid.abs() > 1).any(-1).float().mean()) < 0.9
    ref = F.grid_sample(vol.double().permute(0, 4, 1, 2, 3).expand(n, c, d, h, w), grid.double(), align_corners=False)      # [N,C,D,H,W]
    guard = _GuardedTorch()
    vdev = flat.to(DEV).view(1, h, w, d, c).permute(0, 3, 1, 2, 4)
    y = K.warp3d(vdev, grid.to(DEV), guard.empty(n, h, w, d * c, device=DEV))
    guard.check()
    assert unwritten(y) == 0
    _err(y.view(n, h, w, d, c).permute(0, 4, 3, 1, 2), ref, STREAM_TOL, "warp3d")
    assert torch.equal(y[0, 0, 0].view(d, c)[0].cpu(), vol[0, 1, 3, 2])      # an exact centre returns the voxel itself
    assert torch.equal(K.warp3d(vdev.contiguous(), grid.to(DEV)), y)
    with pytest.raises(RuntimeError):
        K.warp3d(vdev, grid[:, :, :3].contiguous().to(DEV))                  # a deformation of another size: not built


def test_occlusion_head_matches_fp64():
    from e4s_amd import kernels as K
    n, d, h, w, c = 2, 4, 7, 5, 112
    x = torch.zeros(n, d, h, w, 128)
    x[..., :c] = _rand(n, d, h, w, c, seed=80).abs()
    x[..., c:] = 9.0                                                         # the pad channels are not part of the head
    wt, bias = _rand(1, c * d, 7, 7, seed=81) / math.sqrt(49 * c * d) * 4, _rand(1, seed=82)
    ref = torch.sigmoid(F.conv2d(x[..., :c].double().permute(0, 4, 1, 2, 3).reshape(n, c * d, h, w), wt.double(), bias.double(), padding=3))
    guard = _GuardedTorch()
    out = K.occlusion(x.to(DEV), c, K.occlusion_pack(wt.to(DEV), d), bias.to(DEV), guard.empty(n, h, w, device=DEV))
    guard.check()
    assert unwritten(out) == 0
    assert float(ref.min()) < 0.3 and float(ref.max()) > 0.7
    _err(out, ref[:, 0], STREAM_TOL, "occlusion head")
    alone = K.occlusion(x[1:].to(DEV), c, K.occlusion_pack(wt.to(DEV), d), bias.to(DEV))
    assert torch.equal(alone[0], out[1])


# ---- the reduced network against the reference's fp64 records ----------------------------------------------------------------------
def _net(g):
    from e4s_amd import reenact_warp as rw
    if "fw" not in _STATE:
        fw = rw.FeatureWarp(**g["gen_cfg"])
        fw.load_generator_state_dict(synth.synth_vid2vid_generator_state_dict(fw, seed=g["gen_seed"]))
        _STATE["fw"] = fw.to(DEV)
    return _STATE["fw"]


def _case(g, case):
    c = g["cases"][case]
    ks, kd = synth.synth_vid2vid_keypoints(c["n"], c["seed"], c["jacobian"])
    dev = lambda dct: {k: None if v is None else v.to(DEV) for k, v in dct.items()}
    return c["n"], dev(ks), dev(kd)


def _folded64(sd, conv, norm):
    """fp64 (weight, bias) of conv + eval BatchNorm from a state dict"""
    s = sd[norm + ".weight"].double() / torch.sqrt(sd[norm + ".running_var"].double() + 1e-5)
    return sd[conv + ".weight"].double() * s.view(-1, 1, 1, 1), sd[norm + ".bias"].double() + (sd[conv + ".bias"].double() - sd[norm + ".running_mean"].double()) * s


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("precision,_,tol", PRECISIONS)
def test_reduced_network_against_the_reference(g, monkeypatch, precision, _, tol, case):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    fw = _net(g)
    n, ks, kd = _case(g, case)
    frame = synth.synth_vid2vid_frames(*g["frame_A"]).to(DEV)
    taps, cs = {}, g["tap_cstep"]
    out = fw.run(frame, ks, kd, taps=taps)
    vol5 = lambda t: t.permute(3, 0, 1, 2)                                  # [D,H,W,C] -> [C,D,H,W]
    for name in ("first", "down0", "down1"):
        _abs_err(taps[name][0].permute(2, 0, 1)[::cs], g[f"src.tap.{name}"], tol * g[f"src.tap.{name}.scale"], f"{precision} {name}")
    for name in ("second", "res0", "res1", "compressed"):
        _abs_err(vol5(taps[name][0])[::cs], g[f"src.tap.{name}"], tol * g[f"src.tap.{name}.scale"], f"{precision} {name}")
    d, h, w = taps["res1"].shape[1:4]
    ref_logits, ref_deform, ref_occ = g[f"{case}.logits"], g[f"{case}.deformation"], g[f"{case}.occlusion_map"]
    d_vol, d_comp = tol * g["src.tap.res1.scale"], tol * g["src.tap.compressed.scale"]
    delta = tol * float(ref_logits.abs().max())
    grow = math.exp(2 * delta) - 1
    motion = g[f"{case}.motion_max"]
    d_g = grow * motion + STREAM_TOL * motion
    lip = g["src.lip"]
    d_warp = d_vol + d_g * (w / 2 * lip[0] + h / 2 * lip[1] + d / 2 * lip[2])
    for i in range(n):
        pre = f"{case}.{i}.tap."
        hs = g[pre + "hg_input.scale"]
        _abs_err(vol5(taps["hg_input"][i])[::cs], g[pre + "hg_input"], d_comp + STREAM_TOL * hs, f"{precision} {case}{i} hg_input")
        for name in ("enc0", "enc1", "dec0", "dec1", "prediction"):
            _abs_err(vol5(taps[name][i])[::cs], g[pre + name], tol * g[pre + name + ".scale"], f"{precision} {case}{i} {name}")
        ws = g[pre + "warped.scale"]
        _abs_err(taps["warped"][i].view(h, w, d, -1).permute(3, 2, 0, 1)[::cs], g[pre + "warped"], d_warp + STREAM_TOL * ws, f"{precision} {case}{i} warped")
    _err(taps["logits"].permute(0, 4, 1, 2, 3), ref_logits, tol, f"{precision} {case} logits")
    assert tuple(out["mask"].shape) == (n, 16, d, h, w) and tuple(out["deformation"].shape) == (n, d, h, w, 3)
    assert tuple(out["occlusion_map"].shape) == (n, 1, h, w) and tuple(out["feature"].shape) == (n, 128, h, w)
    ref_mask = torch.softmax(ref_logits, 1)
    assert float((ref_mask[:, ::cs] - g[f"{case}.mask"]).abs().max()) <= 1e-15
    _abs_err(out["mask"], ref_mask, grow, f"{precision} {case} mask")
    _abs_err(out["deformation"], ref_deform, d_g, f"{precision} {case} deformation")
    z = torch.log(ref_occ / (1 - ref_occ))
    d_occ = 0.25 * tol * float(z.abs().max()) + STREAM_TOL
    _abs_err(out["occlusion_map"], ref_occ, d_occ, f"{precision} {case} occlusion_map")
    # third and feature: the propagated (loose) bound of the docstring
    sd = synth.synth_vid2vid_generator_state_dict(fw, seed=g["gen_seed"])
    w3, b3 = _folded64(sd, "third.conv", "third.norm")
    w4, b4 = sd["fourth.weight"].double(), sd["fourth.bias"].double()
    row3, row4 = float(w3.abs().sum((1, 2, 3)).max()), float(w4.abs().sum((1, 2, 3)).max())
    t_scale = max(g[f"{case}.{i}.tap.third.scale"] for i in range(n))
    d_third = row3 * (d_warp + STREAM_TOL * g[f"{case}.0.tap.warped.scale"]) + tol * t_scale
    fourth_max = row4 * t_scale + float(b4.abs().max())
    d_feat = row4 * d_third + tol * fourth_max + fourth_max * d_occ + STREAM_TOL * fourth_max
    for i in range(n):
        _abs_err(taps["third"][i].permute(2, 0, 1)[::cs], g[f"{case}.{i}.tap.third"], d_third, f"{precision} {case}{i} third")
    _abs_err(out["feature"][:, ::cs], g[f"{case}.feature"], d_feat, f"{precision} {case} feature")
    assert out["feature"].permute(0, 2, 3, 1).is_contiguous()               # a channels-last view


@pytest.mark.parametrize("precision,tol,_", PRECISIONS)
def test_tail_from_the_native_warped_map(g, monkeypatch, precision, tol, _):
    """third, fourth and the occlusion product recomputed in fp64, in the REFERENCE's channel order, from the native warped map and
    occlusion map: two layers, each at the single-layer bound (the second also carries the first's error through its row sum)."""
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    fw = _net(g)
    n, ks, kd = _case(g, "b")
    taps = {}
    out = fw.run(synth.synth_vid2vid_frames(*g["frame_A"]).to(DEV), ks, kd, taps=taps)
    d, c = fw.reshape_depth, fw.reshape_channel
    _, h, w, _ = taps["warped"].shape
    warped = taps["warped"].double().cpu().view(n, h, w, d, c).permute(0, 4, 3, 1, 2).reshape(n, c * d, h, w)      # .view(bs, c d, h, w)
    sd = synth.synth_vid2vid_generator_state_dict(fw, seed=g["gen_seed"])
    w3, b3 = _folded64(sd, "third.conv", "third.norm")
    third = F.leaky_relu(F.conv2d(warped, w3, b3, padding=1), 0.01)
    _err(taps["third"].permute(0, 3, 1, 2), third, tol, f"{precision} third from the native warped map")
    w4, b4 = sd["fourth.weight"].double(), sd["fourth.bias"].double()
    fourth = F.conv2d(third, w4, b4)
    feat = fourth * out["occlusion_map"].double().cpu()
    bound = tol * float(fourth.abs().max()) + float(w4.abs().sum((1, 2, 3)).max()) * tol * float(third.abs().max()) + STREAM_TOL * float(fourth.abs().max())
    _abs_err(out["feature"], feat, bound, f"{precision} feature from the native warped map")


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_cached_source_and_batching_do_not_change_the_bits(g, monkeypatch, precision):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    fw = _net(g)
    n, ks, kd = _case(g, "b")
    frame = synth.synth_vid2vid_frames(*g["frame_A"]).to(DEV)
    direct = fw.run(frame, ks, kd)
    handle = fw.encode_source(frame[0])
    cached = fw.run(handle, ks, kd)
    again = fw.run(handle, ks, [{k: None if v is None else v[i:i + 1] for k, v in kd.items()} for i in range(n)])      # a list of per-frame dicts
    for key in ("mask", "deformation", "occlusion_map", "feature"):
        assert torch.equal(direct[key], cached[key]) and torch.equal(direct[key], again[key]), key
        assert direct[key].data_ptr() != cached[key].data_ptr()             # fresh tensors
    for i in range(n):
        one = fw.run(handle, ks, {k: None if v is None else v[i:i + 1] for k, v in kd.items()})
        for key in ("mask", "deformation", "occlusion_map", "feature"):
            assert torch.equal(one[key][0], direct[key][i]), (key, i)
    u8 = (frame * 255).round().to(torch.uint8)                              # uint8 frames are read as x / 255
    as_float = u8.float() / torch.full_like(u8, 255, dtype=torch.float32)
    assert torch.equal(fw.encode_source(u8).volume, fw.encode_source(as_float).volume)
    with pytest.raises(RuntimeError, match="device frames only"):
        fw.run(frame.cpu(), ks, kd)


def test_reenact_warp_equals_the_composition_of_its_parts(g, golden):
    from e4s_amd import reenact, reenact_warp as rw
    r = golden("reenact.pt")
    kp = reenact.KPDetector(**r["kp_cfg"], estimate_jacobian=True)
    kp.load_state_dict(synth.synth_vid2vid_state_dict(kp, seed=r["kp_seed"]), strict=True)
    he = reenact.HEEstimator(block_expansion=64, feature_channel=32, num_kp=15, image_channel=3, max_features=2048, num_bins=66)
    he.load_state_dict(synth.synth_vid2vid_state_dict(he, seed=r["he_seed"]), strict=True)
    fe = reenact.PoseFrontEnd(kp.to(DEV), he.to(DEV), True)
    fw = _net(g)
    src = synth.synth_vid2vid_frames(*r["frame_A"])[0]
    drv = synth.synth_vid2vid_frames(*r["frame_B"])
    both = rw.ReenactWarp(fe, fw)
    got = both.run(src.numpy(), [f.numpy() for f in drv], free_view=True, yaw=10.0, pitch=None, roll=None)
    ks, kd = fe.keypoints(src.numpy(), [f.numpy() for f in drv], free_view=True, yaw=10.0, pitch=None, roll=None)
    want = fw.run(src.to(DEV), ks, kd)
    assert tuple(got["feature"].shape) == (2, 128, 16, 12) and bool(torch.isfinite(got["feature"]).all())
    for key in ("mask", "deformation", "occlusion_map", "feature"):
        assert torch.equal(got[key], want[key]), key


def test_shipped_size_smoke(g, monkeypatch):
    """The shipped vox-256.yaml generator on a 256 x 256 frame, N = 1, split-bf16, synthetic weights left as constructed."""
    from e4s_amd import criteria, kernels as K, reenact_warp as rw
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", True)
    torch.manual_seed(0)
    fw = rw.FeatureWarp(**g["gen_shipped"]).to(DEV)
    ks, kd = synth.synth_vid2vid_keypoints(1, 7, False)
    frame = synth.synth_vid2vid_frames(1, 256, 256, seed=9).to(DEV)
    out = fw.run(frame, {"value": ks["value"].to(DEV), "jacobian": None}, {"value": kd["value"].to(DEV), "jacobian": None})
    assert tuple(out["mask"].shape) == (1, 16, 16, 64, 64) and tuple(out["deformation"].shape) == (1, 16, 64, 64, 3)
    assert tuple(out["occlusion_map"].shape) == (1, 1, 64, 64) and tuple(out["feature"].shape) == (1, 256, 64, 64)
    for key, t in out.items():
        assert bool(torch.isfinite(t).all()), key
    assert float((out["mask"].sum(1) - 1).abs().max()) <= 1e-5
    assert 0.0 <= float(out["occlusion_map"].min()) and float(out["occlusion_map"].max()) <= 1.0
