"""Times SPADEDecoder.run and Reenactor.run (e4s_amd/spade.py) with HIP events beside torch eager fp32 of the same weights, and every
launch of the decoder alone.

    python tools/spade_bench.py [--iters 30] [--warmup 3] [--batches 1,8] [--no-eager] [--no-layers] [--no-reenactor]

SPADEDecoder.run on a 64 x 64 feature (a 256 x 256 frame) for N = 1 and 8, both arithmetics (E4S_PRECISION f32 and bf16x3), and
Reenactor.run (front end + generator, the shipped vox-256.yaml sizes) on 256 x 256 frames.  The eager leg is a plain-torch statement
of the decoder (NCHW; F.conv2d / F.instance_norm / F.interpolate), written below, with the spectral norm folded once outside the
timed region as the native path caches it.  Weights are synthetic: the speed does not depend on their values.  The layers are timed
one launch at a time at N = 1; `frac` is algorithmic FLOP (2 H W Cin Cout 9, every tap counted whether or not it falls outside) /
time / 2500 TFLOP/s, the BF16 dense MFMA rate bench.py's roofline_dominant uses (split-bf16 executes three MFMAs per product, so its
ceiling is 1/3; the exact-fp32 MFMA's own rate is 16 times lower).  One JSON line per configuration."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("E4S_ALLOW_UNINITIALIZED_LOSS_NETS", "1")

from e4s_amd import kernels as K, reenact, spade, synth  # noqa: E402

PEAK_BF16_MFMA_TFLOPS = 2500.0
GEN = dict(image_channel=3, feature_channel=32, num_kp=15, estimate_jacobian=False, block_expansion=64, max_features=512, num_down_blocks=2,
           reshape_channel=32, reshape_depth=16, num_resblocks=6, estimate_occlusion_map=True,
           dense_motion_params=dict(block_expansion=32, max_features=1024, num_blocks=5, reshape_depth=16, compress=4))
KP = dict(temperature=0.1, block_expansion=32, max_features=1024, scale_factor=0.25, num_blocks=5, reshape_channel=16384, reshape_depth=16,
          num_kp=15, image_channel=3, feature_channel=32, estimate_jacobian=False)
HE = dict(block_expansion=64, max_features=2048, num_bins=66, num_kp=15, image_channel=3, feature_channel=32, estimate_jacobian=False)


def eager_weights(dec):
    """{conv name: (weight, bias)} with the spectral norm folded, fp32"""
    out = {}
    for name, blk in [(n, b) for _, blocks in dec.stages() for n, b in blocks]:
        for cname in ("conv_0", "conv_1") + (("conv_s",) if blk.learned_shortcut else ()):
            c = getattr(blk, cname)
            out[f"{name}.{cname}"] = (spade.spectral_weight(c.weight_orig, c.weight_u, c.weight_v).float(), c.bias)
    return out


def eager_spade(sp, x, seg):
    a = F.relu(F.conv2d(F.interpolate(seg, size=x.shape[2:], mode="nearest"), sp.mlp_shared[0].weight, sp.mlp_shared[0].bias, padding=1))
    gamma = F.conv2d(a, sp.mlp_gamma.weight, sp.mlp_gamma.bias, padding=1)
    beta = F.conv2d(a, sp.mlp_beta.weight, sp.mlp_beta.bias, padding=1)
    return F.instance_norm(x, eps=1e-5) * (1 + gamma) + beta


def eager_decoder(dec, wts, seg):
    x = F.conv2d(seg, dec.fc.weight, dec.fc.bias, padding=1)
    for shift, blocks in dec.stages():
        for name, blk in blocks:
            if shift:
                x = F.interpolate(x, scale_factor=2, mode="nearest")
            x_s = F.conv2d(eager_spade(blk.norm_s, x, seg), wts[f"{name}.conv_s"][0]) if blk.learned_shortcut else x
            dx = F.conv2d(F.leaky_relu(eager_spade(blk.norm_0, x, seg), 0.2), *wts[f"{name}.conv_0"], padding=1)
            dx = F.conv2d(F.leaky_relu(eager_spade(blk.norm_1, dx, seg), 0.2), *wts[f"{name}.conv_1"], padding=1)
            x = x_s + dx
    return torch.sigmoid(F.conv2d(F.leaky_relu(x, 0.2), dec.conv_img.weight, dec.conv_img.bias, padding=1))


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


def layer_rows(dec, h, iters, warmup):
    """Every distinct launch of SPADEDecoder.run at N = 1 on an h x h feature, alone: (row dict) per launch"""
    dev = "cuda"
    rnd = lambda *s: torch.randn(*s, device=dev)

    def report(what, layer, flop, count, run):
        row = {"what": what, "layer": layer, "gflop": round(flop / 1e9, 3), "per_frame": count}
        for prec, f32 in (("f32", True), ("bf16x3", False)):
            fn = run(f32)
            med, best = timed(fn, iters, warmup)
            row[prec + "_ms"], row[prec + "_best_ms"] = round(med, 4), round(best, 4)
            if flop:
                row[prec + "_tflops"] = round(flop / (med * 1e-3) / 1e12, 2)
                row[prec + "_frac"] = round(flop / (med * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4)
        print(json.dumps(row), flush=True)

    def plain(cin, cout, k, hh, res):
        x, y, r0 = rnd(1, hh, hh, cin), torch.empty(1, hh, hh, cout, device=dev), rnd(1, hh, hh, cout) if res else None
        w, b = rnd(cout, cin, k, k), torch.zeros(cout, device=dev)
        return lambda f32: (lambda wp: (lambda: K.rconv(x, cin, wp, cout, k, y, bias=b, r0=r0, f32=f32)))(K.rconv_pack(w, f32))

    def shared(shift, nspade):
        hh, cout = h << shift, 128 * nspade
        seg, y = rnd(1, h, h, 256), torch.empty(1, hh, hh, cout, device=dev)
        w, b = rnd(cout, 256, 3, 3), torch.zeros(cout, device=dev)
        return lambda f32: (lambda wp: (lambda: K.spade_shared(seg, 256, wp, cout, b, y, shift=shift, f32=f32)))(K.rconv_pack(w, f32))

    def modulating(c, hh, xs):
        a, x, y = rnd(1, hh, hh, 384), rnd(1, hh >> xs, hh >> xs, c), torch.empty(1, hh, hh, c, device=dev)
        stats, _ = K.instnorm_stats(x)
        w, b = rnd(2 * c, 128, 3, 3), torch.zeros(2 * c, device=dev)
        return lambda f32: (lambda wp: (lambda: K.spade_conv(a, 128, 128, wp, b, x, stats, y, xs=xs, f32=f32)))(K.rconv_pack(w, f32))

    def stats(c, hh):
        x = rnd(1, hh, hh, c)
        return lambda f32: (lambda: K.instnorm_stats(x))

    conv = lambda cin, cout, k, hh: 2.0 * hh * hh * cin * cout * k * k
    report("rconv", f"fc 256->512 k3@{h}", conv(256, 512, 3, h), 1, plain(256, 512, 3, h, False))
    for shift, nspade in ((0, 12), (1, 3), (2, 3)):
        report("spade_shared", f"mlp_shared x{nspade} 256->{128 * nspade} k3@{h << shift}", conv(256, 128 * nspade, 3, h << shift), 1, shared(shift, nspade))
    for c, hh, xs, count in ((512, h, 0, 12), (512, 2 * h, 1, 2), (256, 2 * h, 0, 1), (256, 4 * h, 1, 2), (64, 4 * h, 0, 1)):
        report("spade_conv", f"gamma+beta 128->2x{c} k3@{hh} xs{xs}", conv(128, 2 * c, 3, hh), count, modulating(c, hh, xs))
    for cin, cout, k, hh, res, count, name in ((512, 512, 3, h, False, 6, "conv_0"), (512, 512, 3, h, True, 6, "conv_1+res"),
                                              (512, 256, 3, 2 * h, False, 1, "up_0.conv_0"), (256, 256, 3, 2 * h, True, 1, "up_0.conv_1+res"),
                                              (512, 256, 1, 2 * h, False, 1, "up_0.conv_s"), (256, 64, 3, 4 * h, False, 1, "up_1.conv_0"),
                                              (64, 64, 3, 4 * h, True, 1, "up_1.conv_1+res"), (256, 64, 1, 4 * h, False, 1, "up_1.conv_s")):
        report("rconv", f"{name} {cin}->{cout} k{k}@{hh}", conv(cin, cout, k, hh), count, plain(cin, cout, k, hh, res))
    for c, hh, count in ((512, h, 13), (256, 2 * h, 2), (64, 4 * h, 1)):
        report("instnorm_stats", f"{c}@{hh}", 0.0, count, stats(c, hh))
    x = rnd(1, 4 * h, 4 * h, 64)
    wp, b = K.spade_tail_pack(rnd(3, 64, 3, 3)), torch.zeros(3, device=dev)
    report("spade_tail", f"conv_img 64->3 k3@{4 * h}", conv(64, 3, 3, 4 * h), 1, lambda f32: (lambda: K.spade_tail(x, wp, b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--no-reenactor", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spade_bench: needs the GPU (no CPU timing is meaningful)")
    dec = spade.SPADEDecoder()
    dec.load_state_dict(synth.synth_vid2vid_decoder_state_dict(dec, seed=1), strict=True)
    dec = dec.to("cuda")
    wts = eager_weights(dec)
    for n in (int(v) for v in a.batches.split(",")):
        feat = synth.synth_vid2vid_decoder_feature(n, 64, 64, 2).to("cuda").contiguous(memory_format=torch.channels_last)
        row = {"what": "SPADEDecoder.run", "feature": [64, 64], "frames": n}
        for prec in ("f32", "bf16x3"):
            K.PRECISION = prec
            med, best = timed(lambda: dec.run(feat), a.iters, a.warmup)
            row[prec + "_ms"], row[prec + "_best_ms"] = round(med, 3), round(best, 3)
        if not a.no_eager:
            seg = feat.contiguous()
            with torch.no_grad():
                med, best = timed(lambda: eager_decoder(dec, wts, seg), a.iters, a.warmup)
            row["eager_f32_ms"], row["eager_f32_best_ms"] = round(med, 3), round(best, 3)
        print(json.dumps(row), flush=True)
        dec.release_workspace()
    if not a.no_reenactor:
        gen = spade.OcclusionAwareSPADEGenerator(**GEN)
        sd = synth.synth_vid2vid_generator_state_dict(gen, seed=1)
        sd.update({"decoder." + k: v for k, v in dec.state_dict().items()})
        gen.load_generator_state_dict(sd)
        kp, he = reenact.KPDetector(**KP), reenact.HEEstimator(**HE)
        kp.load_state_dict(synth.synth_vid2vid_state_dict(kp, seed=1), strict=True)
        he.load_state_dict(synth.synth_vid2vid_state_dict(he, seed=2), strict=True)
        both = spade.Reenactor(reenact.PoseFrontEnd(kp.to("cuda"), he.to("cuda"), False), gen.to("cuda"))
        src = synth.synth_vid2vid_frames(1, 256, 256, 3).to("cuda")
        for n in (int(v) for v in a.batches.split(",")):
            drv = synth.synth_vid2vid_frames(n, 256, 256, 4).to("cuda")
            row = {"what": "Reenactor.run", "size": [256, 256], "driving": n}
            for prec in ("f32", "bf16x3"):
                K.PRECISION = prec
                med, best = timed(lambda: both.run(src[0], drv, u8=True), a.iters, a.warmup)
                row[prec + "_ms"], row[prec + "_best_ms"] = round(med, 3), round(best, 3)
            print(json.dumps(row), flush=True)
        del both, gen
    if not a.no_layers:
        layer_rows(dec, 64, a.iters, a.warmup)


if __name__ == "__main__":
    main()
