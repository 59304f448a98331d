"""GPU tests of the native latent optimisation (e4s_amd.invert; scripts/optimization.py): FusedSGD / FusedAdamax against torch.optim,
their capture in a GraphedStep, the device loss log, LatentOptimizer against the loop written out by hand, a batch as independent
inversions, and the files Optimizer.invert_image writes."""
import copy
import os
import types

import numpy as np
import pytest
import torch

from e4s_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"

OPTS = {   # name -> (native class name, torch class, constructor arguments)
    "sgd": ("FusedSGD", torch.optim.SGD, dict(lr=1e-2)),
    "sgdm": ("FusedSGD", torch.optim.SGD, dict(lr=1e-2, momentum=0.9, weight_decay=0.01)),
    "adamax": ("FusedAdamax", torch.optim.Adamax, dict(lr=2e-3)),
    "adamax_wd": ("FusedAdamax", torch.optim.Adamax, dict(lr=2e-3, betas=(0.6, 0.99), weight_decay=0.01)),   # (lerp's other branch)
}


def _native(name, params, **kw):
    from e4s_amd import optim
    return getattr(optim, OPTS[name][0])(params, **{**OPTS[name][2], **kw})


def _inputs(sizes, steps=6, seed=11):
    """Parameters and `steps` gradients per tensor, about 10 % of the gradient elements exactly zero."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g) for n in sizes]
    grads = []
    for s in range(steps):
        row = []
        for n in sizes:
            gr = torch.randn(n, generator=g) * (0.1 + s)
            gr[torch.rand(n, generator=g) < 0.1] = 0.0
            row.append(gr)
        grads.append(row)
    return params, grads


def _torch_run(cls, kw, params, grads, dtype):
    ps = [p.to(dtype).clone().requires_grad_(True) for p in params]
    opt = cls(ps, **kw)
    for row in grads:
        for p, gr in zip(ps, row):
            p.grad = gr.to(dtype).clone()
        opt.step()
    return [p.detach() for p in ps]


@pytest.mark.parametrize("name", ["sgd", "sgdm", "adamax", "adamax_wd"])
@pytest.mark.parametrize("case", ["sizes", "more_than_a_launch"])
def test_fused_sgd_and_adamax_match_torch_optim(name, case):
    """6 steps against torch.optim on the CPU.  Bound per tensor, test_gpu_ranger.py's convention: 4 x max(e32 of the tensor, e32 over
    the case), e32 = |torch.optim in fp32 - the same class in fp64| on the CPU: the kernel is another fp32 rounding of the same fp64
    computation.  'sizes': n = 1, 63, 4099 (a full 16-byte block and a 3-element tail), 15360 (full blocks only) and a tensor of 4100
    elements that starts one element into its storage: 4-byte aligned, so its full block goes the scalar way too.
    'more_than_a_launch': 49 tensors, one more than a launch carries."""
    _, cls, kw = OPTS[name]
    sizes = [1, 63, 4099, 15360, 4100] if case == "sizes" else [5 + 3 * i for i in range(49)]
    params, grads = _inputs(sizes)
    p64 = _torch_run(cls, kw, params, grads, torch.float64)
    p32 = _torch_run(cls, kw, params, grads, torch.float32)
    e32 = [float((a.double() - b).abs().max()) for a, b in zip(p32, p64)]
    assert max(e32) > 0
    ps = []
    for i, p in enumerate(params):
        if case == "sizes" and i == 4:
            t = torch.empty(p.numel() + 1, device=DEV)[1:]
            t.copy_(p)
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        else:
            t = p.to(DEV)
        ps.append(t.requires_grad_(True))
    opt = _native(name, ps)
    for row in grads:
        for p, gr in zip(ps, row):
            p.grad = gr.to(DEV)
        opt.step()
    for i, p in enumerate(ps):
        err = float((p.detach().cpu().double() - p64[i]).abs().max())
        tol = 4 * max(e32[i], max(e32))
        moved = float((p.detach().cpu() - params[i]).abs().max())
        print(f"{name} {case} tensor {i} n={sizes[i]}: err {err:.3e} e32 {e32[i]:.3e} tol {tol:.3e} moved {moved:.4f}")
        assert moved > 0 and (moved > 1e-3 or sizes[i] < 63)    # (a tensor of a few elements may happen to end near its start)
        assert err <= tol, (i, sizes[i], err, tol)
    st = opt.state[ps[2]]
    assert set(st) == {"sgd": set(), "sgdm": {"momentum_buffer"}}.get(name, {"step", "exp_avg", "exp_inf"})
    if name.startswith("adamax"):
        assert int(st["step"].item()) == 6


@pytest.mark.parametrize("name", ["sgd", "sgdm", "adamax"])
def test_graphed_step_equals_eager_and_follows_lr(name):
    """A GraphedStep over loss = (w * p).sum() == the eager loop bit for bit over 5 steps (2 warm-ups + 3 replays); a changed
    group['lr'] reaches the replay; a changed momentum / beta makes step() refuse."""
    from e4s_amd.optim import GraphedStep
    g = torch.Generator().manual_seed(4)
    w = [torch.randn(n, generator=g).to(DEV) for n in (1000, 37)]
    p0 = [torch.randn(n, generator=g).to(DEV) for n in (1000, 37)]

    def make():
        ps = [p.clone().requires_grad_(True) for p in p0]
        opt = _native(name, ps)

        def body():
            loss = (w[0] * ps[0]).sum() + (w[1] * ps[1] * ps[1]).sum()
            loss.backward()
            opt.step()
            return loss.detach()
        return ps, opt, body

    def eager(steps, halve_at=None):
        ps, opt, body = make()
        losses = []
        for s in range(steps):
            if s == halve_at:
                opt.param_groups[0]["lr"] *= 0.5
            opt.zero_grad(set_to_none=True)
            losses.append(float(body()))
        return [p.detach().clone() for p in ps], losses
    ps, opt, body = make()
    gs = GraphedStep(opt, body, warmup=2)
    losses = [float(gs.step()) for _ in range(3)]
    want, want_losses = eager(5)
    assert all(torch.equal(a.detach(), b) for a, b in zip(ps, want)) and losses == want_losses[2:]
    # a new learning rate goes through device memory into the replay
    opt.param_groups[0]["lr"] *= 0.5
    gs.step()
    halved, _ = eager(6, halve_at=5)
    plain, _ = eager(6)
    assert all(torch.equal(a.detach(), b) for a, b in zip(ps, halved))
    assert not torch.equal(halved[0], plain[0])
    # momentum / betas travel by value: the captured launches would ignore a change, so the replay refuses
    before = [p.detach().clone() for p in ps]
    if name == "adamax":
        opt.param_groups[0]["betas"] = (0.8, 0.999)
    else:
        opt.param_groups[0]["momentum"] = 0.5
    with pytest.raises(RuntimeError, match="re-capture"):
        gs.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a.detach(), b) for a, b in zip(ps, before))


@pytest.mark.parametrize("name", ["sgd", "sgdm", "adamax"])
def test_state_dict_round_trips_with_torch_optim(name):
    _, cls, kw = OPTS[name]
    params, grads = _inputs([300, 4100], steps=5, seed=2)
    ps = [p.to(DEV).requires_grad_(True) for p in params]
    opt = _native(name, ps)
    for row in grads[:3]:
        for p, gr in zip(ps, row):
            p.grad = gr.to(DEV)
        opt.step()
    # native -> torch: the torch class continues from the native state
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    ref = cls(qs, **kw)
    ref.load_state_dict(copy.deepcopy(opt.state_dict()))
    ref.param_groups[0]["foreach"] = False
    for key in ("momentum_buffer", "exp_avg", "exp_inf"):
        if key in opt.state[ps[0]]:
            assert torch.equal(ref.state[qs[0]][key], opt.state[ps[0]][key])
    for p, q, gr in zip(ps, qs, grads[3]):
        p.grad, q.grad = gr.to(DEV), gr.to(DEV)
    opt.step()
    ref.step()
    for p, q in zip(ps, qs):
        assert float((p.detach() - q.detach()).abs().max()) <= 4e-7 * float(q.detach().abs().max())
    # torch -> native: a fresh native optimiser continues from torch's state
    rs = [q.detach().clone().requires_grad_(True) for q in qs]
    back = _native(name, rs)
    back.load_state_dict(copy.deepcopy(ref.state_dict()))
    for q, r, gr in zip(qs, rs, grads[4]):
        q.grad, r.grad = gr.to(DEV), gr.to(DEV)
    ref.step()
    back.step()
    for q, r in zip(qs, rs):
        assert float((r.detach() - q.detach()).abs().max()) <= 4e-7 * float(q.detach().abs().max())
    if name == "adamax":
        assert int(back.state[rs[0]]["step"].item()) == 5 and back.state[rs[0]]["step"].dtype == torch.int64


def test_scalar_log_rows_and_guard_band():
    from e4s_amd import kernels as K
    rows = 5
    for count in (7, 16):
        vals = torch.arange(1, count + 1, device=DEV, dtype=torch.float32)
        srcs = [vals[j:j + 1] for j in range(count)]
        buf = torch.full(((rows + 2) * count,), -7.0, device=DEV)
        log = buf[count:(rows + 1) * count].view(rows, count)
        step = torch.zeros(1, device=DEV, dtype=torch.int64)
        want = torch.full((rows + 2, count), -7.0)
        for t in (0, rows + 1, -3, 2, 5, 1):
            step.fill_(t)
            vals.copy_(torch.arange(1, count + 1, dtype=torch.float32) + 100.0 * t)
            K.scalar_log(srcs, step, log)
            if 1 <= t <= rows:
                want[t] = torch.arange(1, count + 1, dtype=torch.float32) + 100.0 * t
            assert torch.equal(buf.cpu().view(rows + 2, count), want), (count, t)
    with pytest.raises(RuntimeError):
        K.scalar_log([vals[:1]] * 17, step, torch.zeros(rows, 17, device=DEV))


# ---- the application ----------------------------------------------------------------------------------------------------------------
SIZE, LPIPS_SIZES, STEPS = 256, (256, 128), 5


@pytest.fixture(scope="module")
def world():
    """Net3(256) and the three loss networks at synthetic weights, targets, a mask, fixed noise and an initial latent."""
    from e4s_amd.criteria import FaceParsingLoss, IDLoss, LPIPS
    from e4s_amd.networks import Net3
    from e4s_amd.options import make_opts
    net = Net3(make_opts(out_size=SIZE))
    net.load_state_dict(synth.synth_state_dict(SIZE, 13), strict=True)
    net.latent_avg = synth.synth_latent_avg(SIZE).to(DEV)
    net = net.to(DEV).eval()
    for p in net.parameters():
        p.requires_grad = False
    lp = LPIPS()
    lp.load_state_dict(synth.synth_module_state_dict(lp, 0, "lp."))
    idl = IDLoss(types.SimpleNamespace(id_loss_multiscale=True))
    idl.load_state_dict(synth.synth_module_state_dict(idl, 0, "id."))
    fpl = FaceParsingLoss(types.SimpleNamespace())
    fpl.load_state_dict(synth.synth_module_state_dict(fpl, 0, "fp."))
    crit = {"lpips": lp.to(DEV).eval(), "id": idl.to(DEV).eval(), "parsing": fpl.to(DEV).eval()}
    targets = [synth.synth_image_pair(1, SIZE, seed=s)[1].to(DEV) for s in (12, 13, 14)]
    labels = synth.synth_labels_face(1, 512, seed=6)
    g = torch.Generator().manual_seed(6)
    return types.SimpleNamespace(net=net, crit=crit, targets=targets, labels=labels, mask=synth.onehot(labels).to(DEV),
                                 noise=[n.to(DEV) for n in synth.synth_noise(SIZE)],
                                 sv=(torch.randn(2, 12, 1280, generator=g) * 0.1).to(DEV))


@pytest.fixture(scope="module")
def hand_loop(world):
    """scripts/optimization.py:209-222 written out with FusedAdam, one stream, a float() per number: latent, last image, the seven
    numbers of every step."""
    from e4s_amd.optim import FusedAdam
    from e4s_amd.train import mse_loss
    net, c, target = world.net, world.crit, world.targets[0]
    latent = world.sv[:1].clone().requires_grad_(True)
    opt = FusedAdam([latent], lr=1e-2, capturable=True)
    rows = []
    for _ in range(STEPS):
        opt.zero_grad(set_to_none=True)
        img, _, _ = net.gen_img(None, net.cal_style_codes(latent), world.mask, noise=world.noise)
        loss_id, id_improve, _ = c["id"](img, target)
        loss_l2 = mse_loss(img, target)
        loss_lpips = c["lpips"].forward_pooled(img, target, LPIPS_SIZES)
        loss_fp, fp_improve = c["parsing"](img, target)
        loss = 0.1 * loss_id + loss_l2 + 0.8 * loss_lpips + 0.1 * loss_fp
        loss.backward()
        opt.step()
        rows.append([float(v.detach()) for v in (loss_id, id_improve, loss_l2, loss_lpips, loss_fp, fp_improve, loss)])
    return latent.detach().clone(), img.detach().clone(), torch.tensor(rows, dtype=torch.float64)


@pytest.mark.parametrize("graph", [True, False])
def test_latent_optimizer_equals_the_hand_loop(world, hand_loop, graph):
    from e4s_amd.invert import LatentOptimizer
    lat, img, rows = hand_loop
    lo = LatentOptimizer(world.net, world.crit, lpips_sizes=LPIPS_SIZES, W_steps=STEPS, graph=graph, noise=world.noise)
    res = lo.invert(world.targets[0], world.mask, init=world.sv[:1])
    assert res.latent.shape == (1, 12, 1280) and not res.latent.requires_grad
    assert torch.equal(res.latent, lat) and torch.equal(res.recon, img)
    hist = res.history.cpu().double()
    assert hist.shape == (STEPS, 7) and res.history.dtype == torch.float32 and res.history.is_cuda
    print("loss per step", hist[:, 6].tolist(), "hand", rows[:, 6].tolist())
    assert torch.equal(hist, rows)                              # every column is the hand loop's float(), the loss among them
    assert hist[-1, 6] < hist[0, 6]
    assert res.loss_dict(STEPS)["loss"] == float(rows[-1, 6])
    assert res.recon0.shape == img.shape and not torch.equal(res.recon0, res.recon)


def test_absent_terms_and_fresh_noise(world):
    """noise=None draws new noise in every (replayed) step and starts from the encoder's vectors; the run stays finite and descends.
    A term without lambda leaves its columns 0."""
    from e4s_amd.invert import LatentOptimizer
    torch.manual_seed(5)
    lo = LatentOptimizer(world.net, world.crit, lpips_sizes=LPIPS_SIZES, W_steps=6, face_parsing_lambda=0.0)
    res = lo.invert(world.targets[0], world.mask)
    hist = res.history.cpu()
    print("fresh-noise loss per step", hist[:, 6].tolist())
    assert bool(torch.isfinite(hist).all()) and bool(torch.isfinite(res.latent).all()) and bool(torch.isfinite(res.recon).all())
    assert bool((hist[:, 4:6] == 0).all()) and bool((hist[:, [0, 2, 3, 6]] != 0).all())
    assert hist[-1, 6] < hist[0, 6]
    with torch.no_grad():
        sv, _ = world.net.get_style_vectors(world.targets[0], world.mask)
    assert float((res.latent - sv).abs().max()) > 0


def test_a_batch_is_independent_inversions(world, monkeypatch):
    """B = 2 in exact fp32.  (a) slot 0 does not see what slot 1 is fitted to: its latent after 3 Adam steps is the same bit for bit
    with another image in slot 1.  (b) the step backpropagates B x the batch loss, the sum of the per-image objectives: after one SGD
    step slot 0 moved as the B = 1 run on its image does, within 2 x 2e-3 of the largest movement (2e-3: the project's bound for this
    gradient against the reference's autograd, test_gpu_timed_path.py; either side may be that far from the truth).  A missing factor B
    would be off by half the scale."""
    from e4s_amd import kernels as K
    from e4s_amd.invert import LatentOptimizer
    monkeypatch.setattr(K, "PRECISION", "f32")
    a, b, c = world.targets
    mask2 = world.mask.expand(2, -1, -1, -1).contiguous()
    kw = dict(lpips_sizes=LPIPS_SIZES, noise=world.noise)
    lo = LatentOptimizer(world.net, world.crit, W_steps=3, **kw)
    r_ab = lo.invert(torch.cat([a, b]), mask2, init=world.sv)
    r_ac = lo.invert(torch.cat([a, c]), mask2, init=world.sv)
    assert not torch.equal(r_ab.latent[1], r_ac.latent[1])
    assert torch.equal(r_ab.latent[0], r_ac.latent[0])
    sgd = LatentOptimizer(world.net, world.crit, W_steps=1, opt_name="sgd", lr=1.0, **kw)
    d2 = sgd.invert(torch.cat([a, b]), mask2, init=world.sv).latent[0] - world.sv[0]
    d1 = sgd.invert(a, world.mask, init=world.sv[:1]).latent[0] - world.sv[0]
    scale = float(d1.abs().max())
    diff = float((d2 - d1).abs().max())
    print(f"one SGD step: max|delta| {scale:.4e}, B=2 slot 0 vs B=1 {diff:.4e} ({diff / scale:.2e} of it)")
    assert scale > 1e-4                                        # (far above the rounding of latent - init)
    assert diff < 2 * 2e-3 * scale


def test_optimizer_invert_image_writes_the_scripts_files(world, tmp_path):
    from PIL import Image
    from e4s_amd.invert import Optimizer

    class Stub(list):
        imgs = ["/data/CelebAMask-HQ/test/images/123.jpg"]
    ds = Stub([(world.targets[0][0].cpu(), world.labels[0].float() / 255, None)])
    opts = types.SimpleNamespace(l2_lambda=1.0, lpips_lambda=0.8, id_lambda=0.1, face_parsing_lambda=0.1, lpips_sizes=LPIPS_SIZES,
                                 opt_name="adam", lr=1e-2, W_steps=4, output_dir=str(tmp_path), save_intermediate=True, save_interval=2,
                                 device=DEV, num_seg_cls=12, out_size=SIZE, verbose=False)
    torch.manual_seed(1)
    res = Optimizer(opts, dataset=ds, net=world.net, crit=world.crit).invertion(0)
    d = tmp_path / "123"
    assert sorted(os.listdir(d)) == ["123_0002.npy", "123_0002.png", "123_0004.npy", "123_0004.png", "123_gt.png", "123_recon.png"]
    lat = np.load(d / "123_0004.npy")
    assert lat.dtype == np.float32 and np.array_equal(lat, res.latent.cpu().numpy())
    mid = np.load(d / "123_0002.npy")
    assert mid.shape == lat.shape and not np.array_equal(mid, lat)

    def rule(x):
        return ((x[0].cpu() + 1) / 2).clamp(0, 1).mul(255).byte().permute(1, 2, 0).numpy()
    assert np.array_equal(np.asarray(Image.open(d / "123_0004.png")), rule(res.recon))
    assert np.array_equal(np.asarray(Image.open(d / "123_recon.png")), rule(res.recon0))
    assert np.array_equal(np.asarray(Image.open(d / "123_gt.png")), rule(world.targets[0]))
    assert not np.array_equal(np.asarray(Image.open(d / "123_0002.png")), np.asarray(Image.open(d / "123_0004.png")))
