"""Time of the native Real-ESRNet x4 (e4s_amd.sr.RealESRNet.upscale) on 256^2 uint8 frames, run on the GPU box.

For B = 1 and 8 and both arithmetics (E4S precision f32 / bf16x3): HIP-event ms per image of `upscale` (eager, and replayed from a
HIP graph), algorithmic TFLOP/s against the FLOPs counted from the shapes (2 per MAC of the 351 convs: 1.297 TFLOP per 256^2
image), for bf16x3 the fraction of the split-bf16 ceiling (1/3 of the dense bf16 MFMA peak: three MFMAs per product), and the
ratio to the same state_dict in a plain torch nn.Conv2d restatement (eager fp32, MIOpen) on the same GPU.  The two are also
compared on the timed input (max |difference| of the uint8 results).  Prints one JSON line per configuration.

    python tools/sr_bench.py [--iters 10] [--batches 1,8] [--size 256]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from e4s_amd import kernels as K  # noqa: E402
from e4s_amd import synth  # noqa: E402
from e4s_amd.sr import RealESRNet  # noqa: E402

BF16_DENSE_PEAK_TFLOPS = 2516.6          # MI355X v_mfma_f32_32x32x16_bf16, chip peak


class TorchRRDBNet(nn.Module):
    """RRDBNet (scale 4, 32 features) in plain torch ops, with the state_dict keys of e4s_amd.sr.RRDBNet."""

    class RDB(nn.Module):
        def __init__(self):
            super().__init__()
            for k in range(5):
                setattr(self, f"conv{k + 1}", nn.Conv2d(32 * (k + 1), 32, 3, 1, 1))

        def forward(self, x):
            feats = [x]
            for k in range(4):
                feats.append(F.leaky_relu(getattr(self, f"conv{k + 1}")(torch.cat(feats, 1)), 0.2))
            return self.conv5(torch.cat(feats, 1)) * 0.2 + x

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.rdb1, self.rdb2, self.rdb3 = TorchRRDBNet.RDB(), TorchRRDBNet.RDB(), TorchRRDBNet.RDB()

        def forward(self, x):
            return self.rdb3(self.rdb2(self.rdb1(x))) * 0.2 + x

    def __init__(self, num_block=23):
        super().__init__()
        self.conv_first = nn.Conv2d(3, 32, 3, 1, 1)
        self.body = nn.Sequential(*[TorchRRDBNet.Block() for _ in range(num_block)])
        for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
            setattr(self, name, nn.Conv2d(32, 32, 3, 1, 1))
        self.conv_last = nn.Conv2d(32, 3, 3, 1, 1)

    def forward(self, x):
        feat = self.conv_first(x)
        feat = feat + self.conv_body(self.body(feat))
        feat = F.leaky_relu(self.conv_up1(F.interpolate(feat, scale_factor=2, mode="nearest")), 0.2)
        feat = F.leaky_relu(self.conv_up2(F.interpolate(feat, scale_factor=2, mode="nearest")), 0.2)
        return self.conv_last(F.leaky_relu(self.conv_hr(feat), 0.2))

    def upscale(self, img_u8):
        y = self(img_u8.permute(0, 3, 1, 2).float() / 255)
        return torch.round(y.clamp(0, 1) * 255.0).to(torch.uint8).permute(0, 2, 3, 1)


def count_flops(net, h, w):
    """2 per MAC of every conv of one h x w image (trunk at h x w, conv_up1 at 2x, conv_up2 / conv_hr / conv_last at 4x)."""
    total = 0
    for name, m in net.named_modules():
        if isinstance(m, nn.Conv2d):
            up = {"conv_up1": 4, "conv_up2": 16, "conv_hr": 16, "conv_last": 16}.get(name, 1)
            total += 2 * m.weight.numel() * h * w * up
    return total


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sr_bench needs the GPU: a time taken anywhere else says nothing")
    dev = "cuda"
    sr = RealESRNet(device="cpu")
    sd = synth.synth_rrdb_state_dict(sr.srmodel)
    sr.srmodel.load_state_dict(sd, strict=True)
    sr.srmodel.to(dev)
    sr.device = dev
    ref = TorchRRDBNet()
    ref.load_state_dict(sd, strict=True)
    ref = ref.to(dev).eval()
    flops = count_flops(ref, args.size, args.size)
    with torch.no_grad():
        for b in [int(v) for v in args.batches.split(",")]:
            img = synth.synth_sr_input_u8(b, args.size, args.size, seed=41).to(dev)
            torch_ms = timed(lambda: ref.upscale(img), max(2, args.iters // 2), warmup=1)
            want = ref.upscale(img)
            rows = [("torch_eager_fp32", "f32", torch_ms, 0)]
            for prec in ("f32", "bf16x3"):
                K.PRECISION = prec
                ms = timed(lambda: sr.upscale(img), args.iters)
                out = sr.upscale(img)
                diff = int((out.int() - want.int()).abs().max())
                rows.append(("native_eager", prec, ms, diff))
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    sr.upscale(img)
                torch.cuda.current_stream().wait_stream(s)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    sr.upscale(img)
                rows.append(("native_graph", prec, timed(graph.replay, args.iters), diff))
                del graph
            for mode, prec, ms, diff in rows:
                tf = flops * b / ms / 1e9
                line = {"tool": "sr_bench", "batch": b, "input": f"{args.size}x{args.size} uint8 NHWC", "mode": mode, "precision": prec,
                        "ms_per_image": round(ms / b, 3), "tflop_per_image": round(flops / 1e12, 3), "tflops_algorithmic": round(tf, 1),
                        "ratio_to_torch_eager": round(torch_ms / ms, 2), "max_u8_diff_vs_torch": diff}
                if prec == "bf16x3":
                    line["fraction_of_split_bf16_ceiling"] = round(tf / (BF16_DENSE_PEAK_TFLOPS / 3), 3)
                print(json.dumps(line), flush=True)
            sr.srmodel.release_workspace()


if __name__ == "__main__":
    main()
