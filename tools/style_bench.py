"""Times the VGG16 Gram-matrix StyleLoss (e4s_amd.criteria.StyleLoss) with HIP events beside a plain-torch statement of it on the same
weights in eager fp32, each new kernel alone per layer, and the G step of the train loop with and without the term.

    python tools/style_bench.py [--iters 30] [--warmup 3] [--batch 2] [--size 1024] [--no-eager] [--no-layers] [--no-step] [--step-iters 10]

StyleLoss forward + backward (target pass included: a training step sees a new target every time) on `batch` images of size x size with
512 x 512 masks, taps [3, 8, 15, 22], both arithmetics (E4S_PRECISION f32 and bf16x3).  The eager leg is written below: F.interpolate,
the normalisation, nn.Conv2d / ReLU / MaxPool2d up to features[22], torch.mm Gram matrices, F.mse_loss and autograd.  Then every
launch of csrc/gram.hip alone at the shapes of that call, and TrainIteration.g_step / graphed_g_step (train_G, full losses, synthetic
weights) with style_lambda 0 and 1.  Weights are synthetic: the speed does not depend on their values.  Medians; one JSON line per row."""
import argparse
import copy
import json
import os
import sys
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("E4S_ALLOW_UNINITIALIZED_LOSS_NETS", "1")

from e4s_amd import criteria, kernels as K, synth  # noqa: E402

TAPS = [3, 8, 15, 22]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0]


def eager_style(features, x, x_hat, mask, normalize=True):
    """style_loss.py:133-221 restated in plain torch (NCHW, autograd), features[0..22] only"""
    mean, std = (torch.tensor(v, device=x.device).view(1, 3, 1, 1) for v in (MEAN, STD))
    m = F.interpolate(mask, size=(256, 256), mode="bilinear")

    def grams(img):
        t = F.interpolate(img, size=(256, 256), mode="bilinear")
        if normalize:
            t = ((t + 1) / 2 - mean) / std
        t = t * m
        out = []
        for i, layer in enumerate(features):
            t = layer(t)
            if i in TAPS:
                n, c, h, w = t.shape
                v = t.reshape(n * c, h * w)
                out.append(torch.mm(v, v.t()) / (n * c * h * w))
        return out
    with torch.no_grad():
        gy = grams(x_hat)
    return sum(F.mse_loss(a, b) for a, b in zip(grams(x), gy)) / len(TAPS)


def kernel_rows(batch, size, iters, warmup):
    dev = "cuda"
    row = lambda what, layer, med, best, **kw: print(json.dumps({"what": what, "layer": layer, "ms": round(med, 4), "best_ms": round(best, 4), **kw}),
                                                     flush=True)
    x = torch.randn(batch, 3, size, size, device=dev)
    mask = (torch.rand(batch, 1, 512, 512, device=dev) > 0.5).float()
    y = K.style_prep(x, mask, (256, 256), True)
    row("style_prep", f"{size}->256", *timed(lambda: K.style_prep(x, mask, (256, 256), True), iters, warmup))
    row("style_prep_bwd", f"256->{size}", *timed(lambda: K.style_prep_bwd(y, mask, tuple(x.shape), True), iters, warmup))
    g1 = torch.ones(1, device=dev)
    for c, h in ((64, 256), (128, 128), (256, 64), (512, 32)):
        f = torch.rand(batch, h, h, c, device=dev)
        nc = batch * c
        flop = 2.0 * nc * nc * h * h
        ga, gb = K.gram(f), K.gram(torch.rand_like(f))
        acc = torch.zeros(1, device=dev)
        _, d = K.gram_mse(ga, gb, acc, 0.25, init=True)
        med, best = timed(lambda: K.gram(f), iters, warmup)
        row("gram", f"{c}@{h}", med, best, gflop=round(flop / 1e9, 2), tflops=round(flop / (med * 1e-3) / 1e12, 2))
        row("gram_mse", f"{nc}x{nc}", *timed(lambda: K.gram_mse(ga, gb, acc, 0.25), iters, warmup))
        med, best = timed(lambda: K.gram_grad(f, d, g1, 1e-3), iters, warmup)
        row("gram_grad", f"{c}@{h}", med, best, gflop=round(flop / 1e9, 2), tflops=round(flop / (med * 1e-3) / 1e12, 2))


def step_rows(batch, size, iters, warmup, weights):
    from e4s_amd.criteria import FaceParsingLoss, IDLoss, LPIPS, StyleLoss
    from e4s_amd.networks import Net3
    from e4s_amd.optim import FusedAdam
    from e4s_amd.options import make_opts
    from e4s_amd.stylegan2 import Discriminator
    from e4s_amd.train import LossOpts, TrainIteration
    dev = "cuda"
    img = synth.synth_image(batch, size, seed=7, tag="train_img").to(dev)
    mask = synth.onehot(synth.synth_labels_face(batch, 512, seed=21)).to(dev)
    for lam in (0.0, 1.0):
        net = Net3(make_opts(out_size=size, train_G=True))
        net.load_state_dict(synth.synth_state_dict(size, 13), strict=True)
        net.latent_avg = synth.synth_latent_avg(size).to(dev)
        net = net.to(dev).train()
        lp, idl, fpl = LPIPS(), IDLoss(types.SimpleNamespace(id_loss_multiscale=True)), FaceParsingLoss(types.SimpleNamespace())
        for m, tag in ((lp, "lp."), (idl, "id."), (fpl, "fp.")):
            m.load_state_dict(synth.synth_module_state_dict(m, 0, tag))
        crit = {"lpips": lp.to(dev).eval(), "id": idl.to(dev).eval(), "parsing": fpl.to(dev).eval(),
                "style": StyleLoss(TAPS, normalize=True, weights=weights).to(dev)}
        disc = Discriminator(size)
        disc.load_state_dict(synth.synth_disc_state_dict(size), strict=True)
        opt = FusedAdam([p for p in net.parameters() if p.requires_grad], lr=1e-4, capturable=True)
        it = TrainIteration(net, disc.to(dev).train(), crit, opt, None, lo=LossOpts(style_lambda=lam), net_ema=copy.deepcopy(net).eval())
        gs = it.graphed_g_step(img, mask, warmup=warmup)           # captured before any eager step (bench.py:train_leg says why)
        med_g, best_g = timed(gs.step, iters, 2)

        def eager():
            it.forget_targets()
            it.g_step(img, mask)
        med_e, best_e = timed(eager, iters, 2)
        print(json.dumps({"what": "g_step", "size": size, "batch": batch, "style_lambda": lam, "graph_ms": round(med_g, 3),
                          "graph_best_ms": round(best_g, 3), "eager_ms": round(med_e, 3), "eager_best_ms": round(best_e, 3)}), flush=True)
        del it, gs, net, crit, disc, opt
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("style_bench: needs the GPU (no CPU timing is meaningful)")
    dev = "cuda"
    weights = synth.synth_vgg16_state_dict(seed=0)
    mod = criteria.StyleLoss(TAPS, normalize=True, weights=weights).to(dev)
    x = synth.synth_image(a.batch, a.size, seed=3, tag="style_x").to(dev)
    x_hat = synth.synth_image(a.batch, a.size, seed=4, tag="style_y").to(dev)
    mask = synth.onehot(synth.synth_labels_face(a.batch, 512, seed=21)).to(dev)[:, 3:4].contiguous()

    def native():
        mod._target = None
        xv = x.detach().requires_grad_(True)
        mod(xv, x_hat, mask_x=mask, mask_x_hat=mask).backward()
    row = {"what": "StyleLoss forward+backward", "size": a.size, "batch": a.batch, "taps": TAPS}
    for prec in ("f32", "bf16x3"):
        K.PRECISION = prec
        med, best = timed(native, a.iters, a.warmup)
        row[prec + "_ms"], row[prec + "_best_ms"] = round(med, 3), round(best, 3)
    if not a.no_eager:
        feats = torch.nn.ModuleList(list(criteria.vgg16_features())[:23]).to(dev)
        feats.load_state_dict({k[len("features."):]: v for k, v in weights.items()})
        for p in feats.parameters():
            p.requires_grad = False

        def eager():
            xv = x.detach().requires_grad_(True)
            eager_style(feats, xv, x_hat, mask).backward()
        med, best = timed(eager, a.iters, a.warmup)
        row["eager_f32_ms"], row["eager_f32_best_ms"] = round(med, 3), round(best, 3)
    print(json.dumps(row), flush=True)
    K.PRECISION = os.environ.get("E4S_PRECISION", "auto")
    if not a.no_layers:
        kernel_rows(a.batch, a.size, a.iters, a.warmup)
    if not a.no_step:
        step_rows(a.batch, a.size, a.step_iters, a.warmup, weights)


if __name__ == "__main__":
    main()
