"""Times RetinaFaceDetection.detect_device (e4s_amd/retinaface.py) with HIP events beside torch eager fp32 of the same weights.

    python tools/retinaface_bench.py [--iters 10] [--warmup 3] [--sizes 1000x1000,1000x667] [--batches 1,8]

Both arithmetics (E4S_PRECISION f32 and bf16x3) at every size and batch.  The eager leg is a plain-torch restatement of the same
network (NCHW, F.conv2d / F.batch_norm / F.max_pool2d / F.interpolate) up to the three head convs, fed the prepared input; it has no
decode, sort or NMS, so it is a lower bound of what an eager detector costs.  Weights are synthetic (the speed does not depend on
their values; the number of NMS candidates does, and is printed).  One JSON line per configuration."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("E4S_ALLOW_UNINITIALIZED_LOSS_NETS", "1")

from e4s_amd import kernels as K, synth  # noqa: E402
from e4s_amd.retinaface import RetinaFaceDetection  # noqa: E402


def eager_forward(net, x):
    """fp32 NCHW torch eager: the prepared input -> the 9 head maps."""
    def cb(seq, x, relu=True):
        conv, bn = seq
        y = F.batch_norm(F.conv2d(x, conv.weight, None, conv.stride, conv.padding), bn.running_mean, bn.running_var, bn.weight, bn.bias,
                         False, 0.0, bn.eps)
        return F.relu(y) if relu else y
    b = net.body
    x = F.max_pool2d(cb((b.conv1, b.bn1), x), 3, 2, 1)
    feats = []
    for li in range(1, 5):
        for blk in getattr(b, f"layer{li}"):
            idt = x if blk.downsample is None else cb(tuple(blk.downsample), x, False)
            t = cb((blk.conv2, blk.bn2), cb((blk.conv1, blk.bn1), x))
            x = F.relu(cb((blk.conv3, blk.bn3), t, False) + idt)
        if li >= 2:
            feats.append(x)
    f = net.fpn
    o1, o2, o3 = cb(tuple(f.output1), feats[0]), cb(tuple(f.output2), feats[1]), cb(tuple(f.output3), feats[2])
    o2 = cb(tuple(f.merge2), o2 + F.interpolate(o3, size=o2.shape[2:], mode="nearest"))
    o1 = cb(tuple(f.merge1), o1 + F.interpolate(o2, size=o1.shape[2:], mode="nearest"))
    outs = []
    for i, (ssh, x) in enumerate(((net.ssh1, o1), (net.ssh2, o2), (net.ssh3, o3))):
        c51 = cb(tuple(ssh.conv5X5_1), x)
        y = F.relu(torch.cat([cb(tuple(ssh.conv3X3), x, False), cb(tuple(ssh.conv5X5_2), c51, False),
                              cb(tuple(ssh.conv7x7_3), cb(tuple(ssh.conv7X7_2), c51), False)], 1))
        for head in (net.BboxHead[i], net.ClassHead[i], net.LandmarkHead[i]):
            outs.append(F.conv2d(y, head.conv1x1.weight, head.conv1x1.bias))
    return outs


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000x1000,1000x667")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    det = RetinaFaceDetection(None, device="cuda")
    det.net.load_state_dict(synth.synth_retinaface_state_dict(det.net, seed=7), strict=True)
    det.net.to("cuda").eval()
    for size in a.sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        for bsz in (int(v) for v in a.batches.split(",")):
            frames = synth.synth_retinaface_frame_u8(bsz, h, w, 3).to("cuda")
            row = {"size": [h, w], "batch": bsz}
            for prec in ("f32", "bf16x3"):
                K.PRECISION = prec
                med, best = timed(lambda: det.detect_device(frames), a.iters, a.warmup)
                row[prec + "_ms"], row[prec + "_best_ms"] = round(med, 3), round(best, 3)
                row["kept_" + prec] = det.detect_device(frames)[2].tolist()
            if not a.no_eager:
                x = (frames.float() - torch.tensor([104.0, 117.0, 123.0], device="cuda")).permute(0, 3, 1, 2).contiguous()
                with torch.no_grad():
                    med, best = timed(lambda: eager_forward(det.net, x), a.iters, a.warmup)
                row["eager_f32_ms"], row["eager_f32_best_ms"] = round(med, 3), round(best, 3)
            det.net.release_workspace()
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
