"""Throughput of the native BiSeNet face parser (e4s_amd.face_parser.FaceParser.parse) on 1024^2 uint8 batches.

For B = 1 and 8, eager and captured in a HIP graph: HIP-event ms per batch, images/s and algorithmic TFLOP/s (FLOPs counted
from the shapes below, the `parse` path only: bicubic /2, ResNet-18, ARMs, FFM, main head; the auxiliary heads are not run).
For comparison, the same network restated in torch eager fp32 (F.conv2d & co. on the same weights, the same GPU).
Prints one JSON line per configuration.

    python tools/parser_bench.py [--iters 20] [--batches 1,8]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("E4S_ALLOW_UNINITIALIZED_LOSS_NETS", "1")

from e4s_amd import synth  # noqa: E402
from e4s_amd.face_parser import SEG19_TO_12, FaceParser, bicubic_taps  # noqa: E402

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def torch_parse(net, img_u8, taps, flops=None):
    """The parse path restated in torch ops (NCHW fp32, BatchNorm in eval mode): uint8 NHWC -> seg12 labels uint8.
    flops: a one-element list that collects 2*MACs of every conv when given (works on meta tensors)."""
    def conv(x, m, bn=None, relu=False, stride=None, padding=None):
        y = F.conv2d(x, m.weight, None, m.stride if stride is None else stride, m.padding if padding is None else padding)
        if flops is not None:
            flops[0] += 2 * y.numel() * m.weight[0].numel()
        if bn is not None:
            y = F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        return F.relu(y) if relu else y

    def cbr(m, x):
        return conv(x, m.conv, m.bn, relu=True)

    x = img_u8.permute(0, 3, 1, 2).float() / 255
    k = taps.to(x.device, x.dtype)
    x = F.conv2d(F.pad(x, (0, 0, 3, 3), mode="reflect"), k.view(1, 1, 8, 1).repeat(3, 1, 1, 1), stride=(2, 1), groups=3)
    x = F.conv2d(F.pad(x, (3, 3, 0, 0), mode="reflect"), k.view(1, 1, 1, 8).repeat(3, 1, 1, 1), stride=(1, 2), groups=3)
    if flops is not None:
        flops[0] += 2 * 8 * 3 * (x.shape[0] * x.shape[2] * img_u8.shape[2] + x.numel() // 3)
    mean = torch.tensor(MEAN, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=x.device).view(1, 3, 1, 1)
    x = (x.clamp(0, 1) - mean) / std
    size = x.shape[2:]
    r = net.cp.resnet
    x = F.max_pool2d(conv(x, r.conv1, r.bn1, relu=True), 3, 2, 1)
    feats = []
    for layer in (r.layer1, r.layer2, r.layer3, r.layer4):
        for blk in layer:
            y = conv(conv(x, blk.conv1, blk.bn1, relu=True), blk.conv2, blk.bn2)
            sc = x if blk.downsample is None else conv(x, blk.downsample[0], blk.downsample[1])
            x = F.relu(sc + y)
        feats.append(x)
    feat8, feat16, feat32 = feats[1:]
    cp = net.cp

    def arm(a, f):
        f = cbr(a.conv, f)
        return f * torch.sigmoid(conv(f.mean((2, 3), keepdim=True), a.conv_atten, a.bn_atten))

    avg = cbr(cp.conv_avg, feat32.mean((2, 3), keepdim=True))
    up32 = cbr(cp.conv_head32, F.interpolate(arm(cp.arm32, feat32) + avg, feat16.shape[2:], mode="nearest"))
    up16 = cbr(cp.conv_head16, F.interpolate(arm(cp.arm16, feat16) + up32, feat8.shape[2:], mode="nearest"))
    ffm = net.ffm
    feat = cbr(ffm.convblk, torch.cat([feat8, up16], 1))
    g = torch.sigmoid(conv(F.relu(conv(feat.mean((2, 3), keepdim=True), ffm.conv1)), ffm.conv2))
    out = conv(cbr(net.conv_out.conv, feat * g + feat), net.conv_out.conv_out)
    if flops is not None:
        return None
    out = F.interpolate(out, size, mode="bilinear", align_corners=True)
    return torch.tensor(SEG19_TO_12, device=out.device, dtype=torch.uint8)[out.argmax(1)]


def count_flops(net, b, size=1024):
    """Algorithmic FLOPs of one parse of b size^2 images (2 per MAC of every conv and of the bicubic filter)."""
    import copy
    meta = copy.deepcopy(net).to("meta")
    fl = [0]
    with torch.no_grad():
        torch_parse(meta, torch.empty(b, size, size, 3, device="meta", dtype=torch.uint8), torch.empty(8, device="meta"), fl)
    return fl[0]


def timed(fn, iters, warmup=3):
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    dev = "cuda"
    fp = FaceParser(None, device="cpu")
    fp.seg.load_state_dict(synth.synth_module_state_dict(fp.seg, tag="bisenet."), strict=True)
    fp = fp.to(dev)
    taps = bicubic_taps(2)
    for b in [int(v) for v in args.batches.split(",")]:
        x = synth.synth_image(b, 1024, seed=1, tag="bisenet.bench")
        img = ((x + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)
        flops = count_flops(fp.seg, b)
        with torch.no_grad():
            eager_ms = timed(lambda: fp.parse(img, onehot=True), args.iters)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                fp.parse(img, onehot=True)
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                lab, _ = fp.parse(img, onehot=True)
            graph_ms = timed(graph.replay, args.iters)
            torch_ms = timed(lambda: torch_parse(fp.seg, img, taps), args.iters)
            agree = float((torch_parse(fp.seg, img, taps) == lab).double().mean())
        for mode, ms in (("native_eager", eager_ms), ("native_graph", graph_ms), ("torch_eager_fp32", torch_ms)):
            print(json.dumps({"tool": "parser_bench", "batch": b, "input": "1024x1024 uint8 NHWC", "mode": mode,
                              "ms_per_batch": round(ms, 4), "images_per_s": round(b * 1000.0 / ms, 1),
                              "gflop_per_batch": round(flops / 1e9, 2), "tflops_algorithmic": round(flops / ms / 1e9, 2),
                              "labels_agree_with_torch": round(agree, 6)}), flush=True)


if __name__ == "__main__":
    main()
