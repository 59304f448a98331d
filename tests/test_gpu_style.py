"""The native StyleLoss (e4s_amd.criteria.StyleLoss) against the reference's own fp64 record (tests/golden/style.pt, made by
tests/golden/make_style_golden.py on the seeded synthetic VGG16 weights), its target cache, and the term inside the train step.

Tolerances in exact fp32 (E4S_PRECISION=f32).  The kernels sum in another order than ATen, but over fp32 chains of the same lengths, so
the yardstick is the reference's OWN fp32-vs-fp64 error, recorded in the fixture per case: the relative error of the loss and the relative
L2 error of dL/dx are required to be at most 4x those figures (the factor is for the spread between two summation orders).

The sampled Gram entries follow the same rule, relative to the largest entry of the layer's Gram matrices: at most eps_g = 4x the
reference's own fp32 error of its sampled entries.  A recorded figure is the largest of 256 samples of ONE run, so the level is taken as the
largest figure of the whole fixture (all cases, all layers: the chains have the same lengths everywhere), and never below u = 2^-24.  The
per-layer terms follow from that by Cauchy-Schwarz, with no further assumption: if every entry of G_x and of G_xhat is off by at most
dG = eps_g max|G|, then D = G_x - G_xhat is off by at most dD = 2 dG and term = mean(D^2) by at most 2 dD mean|D| + dD^2; mean|D| and
max|G| are in the fixture.  That is a worst case over the signs of the errors and loose by design (1e-5 .. 3e-4 of a term); the loss,
the mean of the terms, carries the tight rule.  Each measured ratio is printed before it is asserted.

In the split-bf16 arithmetic (auto / bf16x3) the relative L2 error of dL/dx against fp64 is within 1e-2, the bound tests/test_gpu_train.py
puts on gradients in that arithmetic.

The train-step cases run at 256^2, batch 2, the smallest size the synthetic Net3 of tests/test_gpu_train.py is built for (a 64^2 generator
has fewer layers than the mask-guided split at layer 13 needs)."""
import copy
import os
import types

import pytest
import torch

import style_cases as sc
from e4s_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "style.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


@pytest.fixture(scope="module")
def vgg_weights():
    return synth.synth_vgg16_state_dict(seed=0)


def _module(case, weights):
    from e4s_amd.criteria import StyleLoss
    return StyleLoss(case["taps"], normalize=case["normalize"], weights=weights).to(DEV)


def _run(case, weights):
    x, x_hat, mask = (None if t is None else t.to(DEV) for t in sc.golden_inputs(case))
    mod = _module(case, weights)
    xv = x.clone().requires_grad_(True)
    loss = mod(xv, x_hat, mask_x=mask, mask_x_hat=mask)
    loss.backward()
    torch.cuda.synchronize()
    return mod, x, mask, loss.detach(), mod.last_terms, xv.grad


@pytest.mark.parametrize("case", sc.GOLDEN_CASES, ids=[c["name"] for c in sc.GOLDEN_CASES])
def test_style_loss_vs_the_references_f64_record(case, golden, vgg_weights, monkeypatch):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", "f32")
    rec = golden[case["name"]]
    mod, x, mask, loss, terms, grad = _run(case, vgg_weights)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.shape == x.shape
    rel_loss = abs(float(loss.double().cpu()) - float(rec["loss"])) / float(rec["loss"])
    rel_grad = float((grad.double().cpu() - rec["grad"]).norm() / rec["grad"].norm())
    rel_terms = ((terms.double().cpu() - rec["terms"]).abs() / rec["terms"]).tolist()
    print(f"\n[style {case['name']}] loss error / reference's fp32 error: {rel_loss / rec['ref_f32_rel_loss']:.2f} ({rel_loss:.2e} / {rec['ref_f32_rel_loss']:.2e})")
    print(f"[style {case['name']}] dL/dx L2 error / reference's fp32 error: {rel_grad / rec['ref_f32_rel_grad']:.2f} ({rel_grad:.2e} / {rec['ref_f32_rel_grad']:.2e})")
    grams = mod.grams(x, mask)
    rel_grams = []
    for g, want in zip(grams, rec["grams"]):
        rows, cols = sc.gram_sample_index(g.shape[0])
        got = g.cpu()[rows][:, cols].double()
        rel_grams.append(float((got - want).abs().max()) / rec["gram_max"][len(rel_grams)])
    eps_g = 4 * max([U] + [f for c in sc.GOLDEN_CASES for f in golden[c["name"]]["ref_f32_rel_grams"]])
    term_tol = []
    for k in range(len(case["taps"])):
        dd = 2 * eps_g * rec["gram_max"][k]
        term_tol.append((2 * dd * rec["d_absmean"][k] + dd * dd) / float(rec["terms"][k]))
    print(f"[style {case['name']}] sampled Gram error / eps_g ({eps_g:.2e} of the largest entry):", [f"{a / eps_g:.3f}" for a in rel_grams],
          "; / the reference's own fp32 error:", [f"{a / max(b, U):.2f}" for a, b in zip(rel_grams, rec["ref_f32_rel_grams"])])
    print(f"[style {case['name']}] term error / tolerance:", [f"{a / b:.4f}" for a, b in zip(rel_terms, term_tol)],
          "; / the reference's own fp32 error:", [f"{a / max(b, U):.2f}" for a, b in zip(rel_terms, rec["ref_f32_rel_terms"])])
    assert rel_loss <= 4 * rec["ref_f32_rel_loss"]
    assert rel_grad <= 4 * rec["ref_f32_rel_grad"]
    for k in range(len(case["taps"])):
        assert rel_grams[k] <= eps_g, f"Gram matrix of tap {case['taps'][k]}"
        assert rel_terms[k] <= term_tol[k], f"term of tap {case['taps'][k]}"


@pytest.mark.parametrize("prec", ["auto", "bf16x3"])
def test_style_loss_gradient_in_split_bf16(prec, golden, vgg_weights, monkeypatch):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", prec)
    case = sc.GOLDEN_CASES[0]
    rec = golden[case["name"]]
    _, _, _, loss, _, grad = _run(case, vgg_weights)
    rel_grad = float((grad.double().cpu() - rec["grad"]).norm() / rec["grad"].norm())
    rel_loss = abs(float(loss.double().cpu()) - float(rec["loss"])) / float(rec["loss"])
    print(f"\n[style {prec}] relative L2 error of dL/dx vs fp64: {rel_grad:.3e}; relative error of the loss: {rel_loss:.3e}")
    assert rel_grad <= 1e-2


def test_the_targets_grams_are_cached_per_target(vgg_weights, monkeypatch):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", "f32")
    case = sc.GOLDEN_CASES[0]
    x, x_hat, mask = (t.to(DEV) for t in sc.golden_inputs(case))
    mod = _module(case, vgg_weights)
    calls = {"gram": 0, "style_prep": 0}
    for name in calls:
        def counted(*a, _fn=getattr(K, name), _name=name, **k):
            calls[_name] += 1
            return _fn(*a, **k)
        monkeypatch.setattr(K, name, counted)
    taps = len(case["taps"])
    first = mod(x, x_hat, mask_x=mask, mask_x_hat=mask)
    assert calls == {"gram": 2 * taps, "style_prep": 2}
    second = mod(x, x_hat, mask_x=mask, mask_x_hat=mask)
    assert calls == {"gram": 3 * taps, "style_prep": 3}, "the second forward on the same target launched target-side work"
    assert torch.equal(first, second)
    x_hat.mul_(0.5)                                                     # an in-place edit of the target: recompute
    third = mod(x, x_hat, mask_x=mask, mask_x_hat=mask)
    assert calls == {"gram": 5 * taps, "style_prep": 5}
    assert not torch.equal(third, second)
    mask[:, :, :4].zero_()                                              # ... and of its mask
    mod(x, x_hat, mask_x=mask, mask_x_hat=mask)
    assert calls == {"gram": 7 * taps, "style_prep": 7}
    fresh = _module(case, vgg_weights)(x, x_hat, mask_x=mask, mask_x_hat=mask)
    assert torch.equal(fresh, mod(x, x_hat, mask_x=mask, mask_x_hat=mask))


# ---- the term inside the train step -------------------------------------------------------------------------------------------------------
SIZE, BATCH = 256, 2


def _iteration(vgg_weights, style_lambda, with_style, ema=False):
    from e4s_amd.criteria import FaceParsingLoss, IDLoss, LPIPS, StyleLoss
    from e4s_amd.networks import Net3
    from e4s_amd.optim import FusedAdam
    from e4s_amd.options import make_opts
    from e4s_amd.stylegan2 import Discriminator
    from e4s_amd.train import LossOpts, TrainIteration
    net = Net3(make_opts(out_size=SIZE, train_G=False))
    net.load_state_dict(synth.synth_state_dict(SIZE, 13), strict=True)
    net.latent_avg = synth.synth_latent_avg(SIZE).to(DEV)
    net = net.to(DEV).train()
    lp, idl, fpl = LPIPS(), IDLoss(types.SimpleNamespace(id_loss_multiscale=True)), FaceParsingLoss(types.SimpleNamespace())
    for m, tag in ((lp, "lp."), (idl, "id."), (fpl, "fp.")):
        m.load_state_dict(synth.synth_module_state_dict(m, 0, tag))
    crit = {"lpips": lp.to(DEV).eval(), "id": idl.to(DEV).eval(), "parsing": fpl.to(DEV).eval()}
    lo = LossOpts(lpips_sizes=(256, 128, 64), style_lambda=style_lambda)
    if with_style:
        crit["style"] = StyleLoss([3, 8, 15, 22], normalize=lo.style_loss_norm == 1, weights=vgg_weights).to(DEV)
    disc = Discriminator(SIZE)
    disc.load_state_dict(synth.synth_disc_state_dict(SIZE), strict=True)
    opt = FusedAdam([p for p in net.parameters() if p.requires_grad], lr=1e-4, capturable=True)
    net_ema = copy.deepcopy(net).eval() if ema else None
    return TrainIteration(net, disc.to(DEV).eval(), crit, opt, None, lo=lo, net_ema=net_ema), net


def _batch(i):
    return (synth.synth_image(BATCH, SIZE, tag="style_img%d" % i).to(DEV),
            synth.onehot(synth.synth_labels_face(BATCH, 512, seed=71 + i)).to(DEV))


@pytest.fixture
def _train_f32(monkeypatch):
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", "f32")


def test_g_step_with_and_without_the_style_term(vgg_weights, _train_f32):
    img, onehot = _batch(0)
    out = {}
    for name, lam, entry in (("plain", 0.0, False), ("entry", 0.0, True), ("style", 1.0, True)):
        it, net = _iteration(vgg_weights, lam, entry)
        loss, terms = it.g_step(img, onehot, randomize_noise=False)
        torch.cuda.synchronize()
        out[name] = (loss, terms, [p.detach().clone() for p in net.parameters()])
    # style_lambda = 0 with a "style" entry in crit: nothing changes, bit for bit
    assert "style" not in out["entry"][1] and list(out["entry"][1]) == list(out["plain"][1])
    assert torch.equal(out["entry"][0], out["plain"][0])
    for a, b in zip(out["entry"][2], out["plain"][2]):
        assert torch.equal(a, b)
    # style_lambda = 1: the term is there, last of calc_loss's terms, and the loss is the default loss + 1 * style
    loss, terms, _ = out["style"]
    keys = list(terms)
    assert "style" in keys and keys.index("style") == keys.index("lpips") + 1
    style = float(terms["style"])
    assert style > 0 and style == style
    want = float(out["plain"][0].double() + terms["style"].double())
    assert abs(float(loss) - want) <= 8 * U * abs(want)               # the sum of six terms in fp32


def test_graphed_g_step_with_the_style_term_equals_the_eager_loop(vgg_weights, _train_f32):
    """Captured on one batch, replayed after the static img / onehot were refilled with another: the replay must recompute the target's
    Gram matrices (TrainIteration.forget_targets inside the captured body), or it serves the first batch's.  style_lambda is large so
    that the term carries weight in the parameters' bits."""
    lam = 1e5
    batches = [_batch(0), _batch(1)]
    it_e, net_e = _iteration(vgg_weights, lam, True, ema=True)
    img_e, hot_e = batches[0][0].clone(), batches[0][1].clone()
    for _ in range(3):
        it_e.forget_targets()
        it_e.g_step(img_e, hot_e, randomize_noise=False)
    img_e.copy_(batches[1][0])
    hot_e.copy_(batches[1][1])
    it_e.forget_targets()
    loss_e, terms_e = it_e.g_step(img_e, hot_e, randomize_noise=False)
    assert lam * float(terms_e["style"]) > 1e-3 * float(loss_e)          # the term matters at this weight

    it_g, net_g = _iteration(vgg_weights, lam, True, ema=True)
    img_g, hot_g = batches[0][0].clone(), batches[0][1].clone()
    gs = it_g.graphed_g_step(img_g, hot_g, warmup=2, randomize_noise=False)
    gs.step()
    img_g.copy_(batches[1][0])
    hot_g.copy_(batches[1][1])
    loss_g = gs.step()
    gs.validate()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, loss_e)
    for (n, pe), (_, pg) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert torch.equal(pe, pg), n
