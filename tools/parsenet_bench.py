"""HIP-event times of the native GPEN face parser (e4s_amd/parsenet.py) beside torch eager fp32 on the same module tree.

    python tools/parsenet_bench.py [--repeats 30] [--warmup 5] [--batches 1 8]

For each batch size: FaceParse.masks (uint8 faces -> uint8 masks) with E4S_PRECISION f32 and bf16x3, and the reference's forward
restated with torch ops on the same parameters (reflect pad, conv2d, batch_norm, leaky_relu, nearest upsampling, argmax, colour
map).  Then FaceRestorer.process (e4s_amd/face_paste.py) with one and four faces in a 1024^2 frame, with an identity stand-in for
the generator: crop, parse, mask post-processing, warps back, merge and blend.  Each figure is the median of `repeats` timed calls after `warmup` untimed ones, with the 10th / 90th percentiles; every
timed call is bracketed by its own pair of events on the current stream.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("E4S_ALLOW_UNINITIALIZED_LOSS_NETS", "1")

GFLOP_PER_FACE = 469.0                                                     # 2 x MACs of the 512^2 net without out_img_conv, rounded


def eager_layer(layer, x):
    if layer.scale == "up":
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    x = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), layer.conv2d.weight, layer.conv2d.bias, stride=layer.stride)
    if layer.norm.norm_type == "bn":
        bn = layer.norm.norm
        x = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    return F.leaky_relu(x, 0.2) if layer.relu.relu_type == "leakyrelu" else x


def eager_block(block, x):
    identity = x if block.shortcut_func is None else eager_layer(block.shortcut_func, x)
    return identity + eager_layer(block.conv2, eager_layer(block.conv1, x))


@torch.no_grad()
def eager_masks(net, faces_u8, lut):
    x = faces_u8.flip(-1).permute(0, 3, 1, 2).float() / 255.0 * 2 - 1
    feat = eager_layer(net.encoder[0], x)
    for block in list(net.encoder)[1:]:
        feat = eager_block(block, feat)
    x = feat
    for block in net.body:
        x = eager_block(block, x)
    x = feat + x
    for block in net.decoder:
        x = eager_block(block, x)
    return lut[eager_layer(net.out_mask_conv, x).argmax(1)]


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "p10_ms": ms[len(ms) // 10], "p90_ms": ms[(9 * len(ms)) // 10], "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    args = ap.parse_args()
    if args.repeats < 20:
        raise SystemExit("--repeats: 20 or more timed calls")
    from e4s_amd import kernels as K
    from e4s_amd import synth
    from e4s_amd.parsenet import MASK_COLORMAP, FaceParse
    fp = FaceParse(base_dir=None, device="cuda")
    fp.faceparse.load_state_dict(synth.synth_parsenet_state_dict(fp.faceparse), strict=True)
    lut = torch.tensor(MASK_COLORMAP, dtype=torch.uint8, device="cuda")
    for b in args.batches:
        faces = synth.synth_sr_input_u8(b, 512, 512, seed=7).cuda()
        for precision in ("f32", "bf16x3"):
            K.PRECISION = precision
            r = timed(lambda: fp.masks(faces), args.warmup, args.repeats)
            r.update(what="FaceParse.masks", batch=b, arithmetic=precision, tflops=GFLOP_PER_FACE * b / r["median_ms"])
            print(json.dumps(r), flush=True)
        native = fp.masks(faces)
        r = timed(lambda: eager_masks(fp.faceparse, faces, lut), args.warmup, args.repeats)
        agree = float((eager_masks(fp.faceparse, faces, lut) == native).float().mean())
        r.update(what="torch eager fp32", batch=b, arithmetic="torch", tflops=GFLOP_PER_FACE * b / r["median_ms"], mask_agreement=agree)
        print(json.dumps(r), flush=True)
        fp.faceparse.release_workspace()
    # FaceRestorer.process: one and four faces in a 1024^2 frame, the parser above and an identity stand-in for the generator
    from e4s_amd import face_paste
    import numpy as np
    frame = synth.synth_sr_input_u8(1, 1024, 1024, seed=9)[0].cuda()
    ref5 = face_paste.reference_5pts(512)
    centres = [(300, 300), (720, 300), (300, 720), (720, 720)]
    landms = np.stack([((ref5 - 256.0) * 0.6 + np.array(c)).T.reshape(10) for c in centres])
    boxes = np.array([[c[0] - 150, c[1] - 150, c[0] + 150, c[1] + 150, 0.99] for c in centres], dtype=np.float64)
    for nf in (1, 4):
        for precision in ("f32", "bf16x3"):
            K.PRECISION = precision
            restorer = face_paste.FaceRestorer(lambda f: f, fp, in_size=512)
            r = timed(lambda: restorer.process(frame, boxes[:nf], landms[:nf]), args.warmup, args.repeats)
            r.update(what="FaceRestorer.process (identity restore)", faces=nf, frame=1024, arithmetic=precision)
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
