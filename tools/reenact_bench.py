"""Times PoseFrontEnd.keypoints_device (e4s_amd/reenact.py) with HIP events beside torch eager fp32 of the same weights, and the five
up-block launches of e4s_conv3d_f32 alone.

    python tools/reenact_bench.py [--iters 30] [--warmup 3] [--drivings 1,8] [--no-eager]

The shipped vox-256.yaml networks on 256 x 256 frames: one source frame and B driving frames, both arithmetics (E4S_PRECISION f32 and
bf16x3).  The eager leg is a plain-torch statement of the same modules (NCHW, F.conv2d / F.conv3d / F.batch_norm / F.interpolate /
F.avg_pool2d, softmax and the keypoint transformation), written below.  Weights are synthetic: the speed does not depend on their
values.  The 3-D layers are timed one launch at a time at B = 1; `frac` is algorithmic FLOP (2 D H W Cin Cout 27) / time / 2500 TFLOP/s,
the BF16 dense MFMA rate that bench.py's roofline_dominant uses (split-bf16 executes three MFMAs per product, so its ceiling is 1/3;
the exact-fp32 MFMA's own rate is 16 times lower).  One JSON line per configuration."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("E4S_ALLOW_UNINITIALIZED_LOSS_NETS", "1")

from e4s_amd import kernels as K, reenact, synth  # noqa: E402

PEAK_BF16_MFMA_TFLOPS = 2500.0
KP = dict(temperature=0.1, block_expansion=32, max_features=1024, scale_factor=0.25, num_blocks=5, reshape_channel=16384, reshape_depth=16,
          num_kp=15, image_channel=3, feature_channel=32, estimate_jacobian=False)
HE = dict(block_expansion=64, max_features=2048, num_bins=66, num_kp=15, image_channel=3, feature_channel=32, estimate_jacobian=False)


def _cb(x, conv, bn, relu=True):
    f = F.conv3d if conv.weight.dim() == 5 else F.conv2d
    y = F.batch_norm(f(x, conv.weight, conv.bias, conv.stride, conv.padding), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    return F.relu(y) if relu else y


def eager_kp(net, x):
    p = net.predictor
    x = F.conv2d(F.pad(x, (6, 6, 6, 6)), net.down.weight, groups=3)[:, :, ::4, ::4]
    for blk in p.down_blocks:
        x = F.avg_pool2d(_cb(x, blk.conv, blk.norm), 2)
    x = F.conv2d(x, p.conv.weight, p.conv.bias)
    b, c, h, w = x.shape
    x = x.view(b, c // p.reshape_depth, p.reshape_depth, h, w)
    for blk in p.up_blocks:
        x = _cb(F.interpolate(x, scale_factor=(1, 2, 2)), blk.conv, blk.norm)
    logits = F.conv3d(x, net.kp.weight, net.kp.bias, padding=1)
    heat = F.softmax(logits.view(b, logits.shape[1], -1) / net.temperature, dim=2)
    d, h, w = logits.shape[2:]
    ax = lambda n: 2 * (torch.arange(n, device=x.device, dtype=x.dtype) / (n - 1)) - 1
    zz, yy, xx = torch.meshgrid(ax(d), ax(h), ax(w), indexing="ij")
    return {"value": (heat.unsqueeze(-1) * torch.stack([xx, yy, zz], -1).view(1, 1, -1, 3)).sum(2)}


def eager_he(net, x):
    def bottleneck(blk, x):
        t = _cb(_cb(x, blk.conv1, blk.norm1), blk.conv2, blk.norm2)
        idt = x if blk.stride == 1 else _cb(x, blk.skip, blk.norm4, False)
        return F.relu(_cb(t, blk.conv3, blk.norm3, False) + idt)
    x = F.max_pool2d(_cb(x, net.conv1, net.norm1), 3, 2, 1)
    for conv, norm, strided, same in ((net.conv2, net.norm2, None, net.block1), (net.conv3, net.norm3, net.block2, net.block3),
                                      (net.conv4, net.norm4, net.block4, net.block5), (net.conv5, net.norm5, net.block6, net.block7)):
        x = _cb(x, conv, norm)
        for blk in ([strided] if strided is not None else []) + list(same):
            x = bottleneck(blk, x)
    x = x.mean((2, 3))
    return {"yaw": net.fc_roll(x), "pitch": net.fc_pitch(x), "roll": net.fc_yaw(x), "t": net.fc_t(x), "exp": net.fc_exp(x)}


def eager_keypoints(kp, he, source, driving):
    can = eager_kp(kp, source)
    ks = reenact.keypoint_transformation(can, eager_he(he, source), False)
    hd = eager_he(he, driving)
    return ks, [reenact.keypoint_transformation(can, {k: v[i:i + 1] for k, v in hd.items()}, False) for i in range(driving.shape[0])]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--drivings", default="1,8")
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    kp, he = reenact.KPDetector(**KP), reenact.HEEstimator(**HE)
    kp.load_state_dict(synth.synth_vid2vid_state_dict(kp, seed=1), strict=True)
    he.load_state_dict(synth.synth_vid2vid_state_dict(he, seed=2), strict=True)
    kp, he = kp.to("cuda"), he.to("cuda")
    fe = reenact.PoseFrontEnd(kp, he, False)
    src = synth.synth_vid2vid_frames(1, 256, 256, 3).to("cuda")
    for n in (int(v) for v in a.drivings.split(",")):
        drv = synth.synth_vid2vid_frames(n, 256, 256, 4).to("cuda")
        row = {"what": "keypoints_device", "size": [256, 256], "driving": n}
        for prec in ("f32", "bf16x3"):
            K.PRECISION = prec
            med, best = timed(lambda: fe.keypoints_device(src[0], drv), a.iters, a.warmup)
            row[prec + "_ms"], row[prec + "_best_ms"] = round(med, 3), round(best, 3)
        if not a.no_eager:
            s_nchw, d_nchw = src.permute(0, 3, 1, 2).contiguous(), drv.permute(0, 3, 1, 2).contiguous()
            with torch.no_grad():
                med, best = timed(lambda: eager_keypoints(kp, he, s_nchw, d_nchw), a.iters, a.warmup)
            row["eager_f32_ms"], row["eager_f32_best_ms"] = round(med, 3), round(best, 3)
        print(json.dumps(row), flush=True)
    # ---- the five up-block launches alone, B = 1 ----
    d, h = 16, 2
    for blk in kp.predictor.up_blocks:
        cin, cout = blk.conv.in_channels, blk.conv.out_channels
        x = torch.randn(1, d, h, h, cin, device="cuda")
        y = torch.empty(1, d, 2 * h, 2 * h, cout, device="cuda")
        bias = torch.zeros(cout, device="cuda")
        flop = 2.0 * d * (2 * h) * (2 * h) * cin * cout * 27
        row = {"what": "conv3d", "layer": f"{cin}->{cout}@{d}x{2 * h}x{2 * h}", "gflop": round(flop / 1e9, 3)}
        for prec, f32 in (("f32", True), ("bf16x3", False)):
            wp = K.conv3d_pack(blk.conv.weight.detach(), f32)
            med, best = timed(lambda: K.conv3d(x, wp, cout, y, bias=bias, relu=True, up2=True, f32=f32), a.iters, a.warmup)
            row[prec + "_ms"], row[prec + "_best_ms"] = round(med, 4), round(best, 4)
            row[prec + "_tflops"] = round(flop / (med * 1e-3) / 1e12, 2)
            row[prec + "_frac"] = round(flop / (med * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4)
        print(json.dumps(row), flush=True)
        h *= 2


if __name__ == "__main__":
    main()
