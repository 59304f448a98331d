"""Times FeatureWarp.encode_source and FeatureWarp.run (e4s_amd/reenact_warp.py) with HIP events beside torch eager fp32 of the same
weights, and every 3-D conv launch of the shipped generator alone.

    python tools/reenact_warp_bench.py [--iters 30] [--warmup 3] [--drivings 1,8] [--no-eager] [--no-layers]

The shipped vox-256.yaml generator (without its SPADE decoder) on a 256 x 256 source: encode_source once, then run against the cached
handle for N driving keypoint sets, both arithmetics (E4S_PRECISION f32 and bf16x3).  The eager leg is a plain-torch statement of
the same stages (NCHW; F.conv2d / F.conv3d / F.batch_norm / F.interpolate / F.avg_pool3d / F.grid_sample), written below; like
make_animation it encodes the source for every driving frame, so `eager_f32_ms` is per call of N frames INCLUDING N source encodes
and `eager_warp_only_f32_ms` is the same without them.  Weights are synthetic: the speed does not depend on their values.  The 3-D
layers are timed one launch at a time at B = 1; `frac` is algorithmic FLOP (2 D H W Cin Cout k^3, real channel counts, every tap
counted whether or not it falls outside) / time / 2500 TFLOP/s, the BF16 dense MFMA rate bench.py's roofline_dominant uses (split-bf16
executes three MFMAs per product, so its ceiling is 1/3; the exact-fp32 MFMA's own rate is 16 times lower).  One JSON line per
configuration."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("E4S_ALLOW_UNINITIALIZED_LOSS_NETS", "1")

from e4s_amd import kernels as K, reenact_warp as rw, synth  # noqa: E402

PEAK_BF16_MFMA_TFLOPS = 2500.0
GEN = dict(image_channel=3, feature_channel=32, num_kp=15, estimate_jacobian=False, block_expansion=64, max_features=512, num_down_blocks=2,
           reshape_channel=32, reshape_depth=16, num_resblocks=6, estimate_occlusion_map=True,
           dense_motion_params=dict(block_expansion=32, max_features=1024, num_blocks=5, reshape_depth=16, compress=4))


def _bn(x, bn):
    return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)


def _cb(x, conv, bn):
    f = F.conv3d if conv.weight.dim() == 5 else F.conv2d
    return _bn(f(x, conv.weight, conv.bias, conv.stride, conv.padding), bn)


def eager_encode(net, x):
    x = F.relu(_cb(x, net.first.conv, net.first.norm))
    for blk in net.down_blocks:
        x = F.avg_pool2d(F.relu(_cb(x, blk.conv, blk.norm)), 2)
    x = F.conv2d(x, net.second.weight, net.second.bias)
    b, _, h, w = x.shape
    v = x.view(b, net.reshape_channel, net.reshape_depth, h, w)
    for blk in net.resblocks_3d:
        t = F.conv3d(F.relu(_bn(v, blk.norm1)), blk.conv1.weight, blk.conv1.bias, padding=1)
        v = F.conv3d(F.relu(_bn(t, blk.norm2)), blk.conv2.weight, blk.conv2.bias, padding=1) + v
    return v


def _grid(d, h, w, like):
    ax = lambda n: 2 * (torch.arange(n, device=like.device, dtype=like.dtype) / (n - 1)) - 1
    zz, yy, xx = torch.meshgrid(ax(d), ax(h), ax(w), indexing="ij")
    return torch.stack([xx, yy, zz], -1)


def eager_warp(net, vol, kps, kpd):
    """vol [N,C,D,h,w], keypoint values [N,K,3] each (no jacobians: the shipped config) -> the decoder's input"""
    dm = net.dense_motion_network
    n, _, d, h, w = vol.shape
    k = kpd.shape[1]
    feat = F.relu(_cb(vol, dm.compress, dm.norm))
    grid = _grid(d, h, w, vol).view(1, 1, d, h, w, 3)
    motions = torch.cat([grid.expand(n, 1, d, h, w, 3), grid - kpd.view(n, k, 1, 1, 1, 3) + kps.view(n, k, 1, 1, 1, 3)], 1)
    rep = feat.unsqueeze(1).expand(n, k + 1, -1, d, h, w).reshape(n * (k + 1), -1, d, h, w)
    deformed = F.grid_sample(rep, motions.reshape(n * (k + 1), d, h, w, 3), align_corners=False).view(n, k + 1, -1, d, h, w)
    gauss = lambda kp: torch.exp(-0.5 * ((grid - kp.view(n, k, 1, 1, 1, 3)) ** 2).sum(-1) / 0.01)
    heat = torch.cat([torch.zeros(n, 1, d, h, w, device=vol.device), gauss(kpd) - gauss(kps)], 1).unsqueeze(2)
    x = torch.cat([heat, deformed], 2).view(n, -1, d, h, w)
    outs = [x]
    for blk in dm.hourglass.encoder.down_blocks:
        outs.append(F.avg_pool3d(F.relu(_cb(outs[-1], blk.conv, blk.norm)), (1, 2, 2)))
    out = outs.pop()
    for blk in dm.hourglass.decoder.up_blocks:
        out = torch.cat([F.relu(_cb(F.interpolate(out, scale_factor=(1, 2, 2)), blk.conv, blk.norm)), outs.pop()], 1)
    pred = F.relu(_cb(out, dm.hourglass.decoder.conv, dm.hourglass.decoder.norm))
    mask = F.softmax(F.conv3d(pred, dm.mask.weight, dm.mask.bias, padding=3), dim=1)
    deformation = (motions.permute(0, 1, 5, 2, 3, 4) * mask.unsqueeze(2)).sum(1).permute(0, 2, 3, 4, 1)
    occ = torch.sigmoid(F.conv2d(pred.reshape(n, -1, h, w), dm.occlusion.weight, dm.occlusion.bias, padding=3))
    warped = F.grid_sample(vol, deformation, align_corners=False).reshape(n, -1, h, w)
    t = F.leaky_relu(_cb(warped, net.third.conv, net.third.norm), 0.01)
    return F.conv2d(t, net.fourth.weight, net.fourth.bias) * occ


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


def conv_layers(net):
    """(name, conv, cin_pad, D, H, W, up2) of every 3-D conv launch of run / encode_source at the shipped sizes, B = 1"""
    dm, d = net.dense_motion_network, net.reshape_depth
    lay = dm.layout["levels"]
    out = [("resblock conv", net.resblocks_3d[0].conv1, None, d, 64, 64, False), ("compress", dm.compress, None, d, 64, 64, False)]
    h = 64
    for i, blk in enumerate(dm.hourglass.encoder.down_blocks):
        out.append((f"down{i}", blk.conv, lay[i]["skip_read"], d, h, h, False))
        h //= 2
    for j, blk in enumerate(dm.hourglass.decoder.up_blocks):
        out.append((f"up{j}", blk.conv, None, d, h, h, True))
        h *= 2
    out.append(("decoder conv", dm.hourglass.decoder.conv, 128, d, 64, 64, False))
    out.append(("mask", dm.mask, 128, d, 64, 64, False))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--drivings", default="1,8")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-layers", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reenact_warp_bench: needs the GPU (no CPU timing is meaningful)")
    net = rw.FeatureWarp(**GEN)
    net.load_generator_state_dict(synth.synth_vid2vid_generator_state_dict(net, seed=1))
    net = net.to("cuda")
    src = synth.synth_vid2vid_frames(1, 256, 256, 3).to("cuda")
    row = {"what": "encode_source", "size": [256, 256]}
    for prec in ("f32", "bf16x3"):
        K.PRECISION = prec
        med, best = timed(lambda: net.encode_source(src), a.iters, a.warmup)
        row[prec + "_ms"], row[prec + "_best_ms"] = round(med, 3), round(best, 3)
    s_nchw = src.permute(0, 3, 1, 2).contiguous()
    if not a.no_eager:
        with torch.no_grad():
            med, best = timed(lambda: eager_encode(net, s_nchw), a.iters, a.warmup)
        row["eager_f32_ms"], row["eager_f32_best_ms"] = round(med, 3), round(best, 3)
    print(json.dumps(row), flush=True)
    for n in (int(v) for v in a.drivings.split(",")):
        ks, kd = synth.synth_vid2vid_keypoints(n, 5, False)
        ks, kd = {"value": ks["value"].to("cuda"), "jacobian": None}, {"value": kd["value"].to("cuda"), "jacobian": None}
        row = {"what": "run (cached source)", "size": [256, 256], "driving": n}
        for prec in ("f32", "bf16x3"):
            K.PRECISION = prec
            handle = net.encode_source(src)
            med, best = timed(lambda: net.run(handle, ks, kd), a.iters, a.warmup)
            row[prec + "_ms"], row[prec + "_best_ms"] = round(med, 3), round(best, 3)
        if not a.no_eager:
            kps, kpd = ks["value"].expand(n, 15, 3).contiguous(), kd["value"]
            with torch.no_grad():
                vol = eager_encode(net, s_nchw).expand(n, -1, -1, -1, -1).contiguous()
                med, best = timed(lambda: eager_warp(net, vol, kps, kpd), a.iters, a.warmup)
                row["eager_warp_only_f32_ms"], row["eager_warp_only_f32_best_ms"] = round(med, 3), round(best, 3)
                rep = s_nchw.expand(n, -1, -1, -1).contiguous()
                med, best = timed(lambda: eager_warp(net, eager_encode(net, rep), kps, kpd), a.iters, a.warmup)
                row["eager_f32_ms"], row["eager_f32_best_ms"] = round(med, 3), round(best, 3)
        print(json.dumps(row), flush=True)
        net.dense_motion_network.release_workspace()
        net.release_workspace()
    if a.no_layers:
        return
    for name, conv, cin_pad, d, h, w, up2 in conv_layers(net):
        cin, cout, k = conv.in_channels, conv.out_channels, conv.kernel_size[0]
        cp = cin if cin_pad is None else cin_pad
        x = torch.zeros(1, d, h, w, cp, device="cuda")
        x[..., :cin] = torch.randn(1, d, h, w, cin, device="cuda")
        ho, wo = (2 * h, 2 * w) if up2 else (h, w)
        y = torch.empty(1, d, ho, wo, -(-cout // 4) * 4, device="cuda")
        bias = torch.zeros(cout, device="cuda")
        flop = 2.0 * d * ho * wo * cin * cout * k ** 3
        row = {"what": "conv3dx", "layer": f"{name} {cin}->{cout} k{k}@{d}x{ho}x{wo}", "gflop": round(flop / 1e9, 3)}
        for prec, f32 in (("f32", True), ("bf16x3", False)):
            wp = K.conv3dx_pack(conv.weight.detach(), f32, cin_pad=cin_pad)
            med, best = timed(lambda: K.conv3dx(x, wp, cout, y, bias=bias, relu=True, up2=up2, f32=f32), a.iters, a.warmup)
            row[prec + "_ms"], row[prec + "_best_ms"] = round(med, 4), round(best, 4)
            row[prec + "_tflops"] = round(flop / (med * 1e-3) / 1e12, 2)
            row[prec + "_frac"] = round(flop / (med * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
