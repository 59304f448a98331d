"""Times resize.pil_resize (csrc/resize.hip) beside Pillow on the CPU, and FaceSwapPipeline.swap(any_size=True) on 512^2 inputs beside
the same swap on 1024^2 inputs.

    python tools/resize_bench.py [--iters 30] [--warmup 3] [--runs 2] [--no-pipeline] [--no-pillow]

Shapes: BICUBIC 512^2 -> 1024^2 and 1536^2 -> 1024^2 at B = 1 and 8 (what any_size=True does to un-cropped frames), and LANCZOS 4320 x
7680 -> half size with a 1300 x 1300 window at B = 1 (the shrink branch of a close-up in an 8K frame).  Every shape is warmed up
first, then HIP events around each of `iters` calls, the median and the best; the whole table is made `runs` times.  The resize is
two launches, horizontal into a workspace and vertical out of it; a fused kernel does not exist, so `fused_ms` is null.  `mbytes` is
what the two launches must move, computed here from the shapes: the input pixels the window's taps reach, the workspace written
and read once, the result written; it stands beside the 8 TB/s of bench.py's roofline_hbm.  The plan of every shape (bytes, rows of
the workspace, taps) is printed before the first device call, so the arithmetic can be read on a machine without a GPU.  One JSON
line per row."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("E4S_ALLOW_UNINITIALIZED_LOSS_NETS", "1")

from e4s_amd import resize  # noqa: E402

HBM_TBS = 8.0
DEV = "cuda"
# (name, filter, (W, H) in, (w, h) out, window in output pixels or None, batches)
SHAPES = (("bicubic 512^2 -> 1024^2", resize.BICUBIC, (512, 512), (1024, 1024), None, (1, 8)),
          ("bicubic 1536^2 -> 1024^2", resize.BICUBIC, (1536, 1536), (1024, 1024), None, (1, 8)),
          ("lanczos 7680x4320 -> 3840x2160, window 1300^2", resize.LANCZOS, (7680, 4320), (3840, 2160), (1270, 430, 2570, 1730), (1,)))
NAMES = {resize.BICUBIC: "BICUBIC", resize.LANCZOS: "LANCZOS"}


def plan(filt, in_wh, size, window):
    """What one image of the call moves, from the shapes alone (the host's coefficient tables give the taps' reach)."""
    (W, H), (w, h) = in_wh, size
    x0, y0, x1, y1 = window or (0, 0, w, h)
    bx, kx = resize.coefficients(W, w, filt, 0.0, float(W))
    by, ky = resize.coefficients(H, h, filt, 0.0, float(H))
    cols = int(bx[x1 - 1, 0] + bx[x1 - 1, 1] - bx[x0, 0])                 # input columns the window's horizontal taps reach
    ry0, ry1 = int(by[y0, 0]), int(by[y1 - 1, 0] + by[y1 - 1, 1])         # input rows its vertical taps reach
    pitch = ((x1 - x0) * 3 + 15) // 16 * 16
    read_in, ws, out = (ry1 - ry0) * cols * 3, (ry1 - ry0) * pitch, (y1 - y0) * (x1 - x0) * 3
    return {"input_rows": ry1 - ry0, "input_cols": cols, "ksize_x": int(kx.shape[1]), "ksize_y": int(ky.shape[1]),
            "bytes_read_input": read_in, "bytes_workspace": ws, "bytes_out": out, "bytes_moved": read_in + 2 * ws + out}


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


def pillow_ms(imgs, filt, size, window, reps):
    """Median wall time of the same call on the CPU: every image resized (Pillow makes the whole result) and cut to the window."""
    from PIL import Image
    pil = [Image.fromarray(i) for i in imgs]
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        for p in pil:
            r = p.resize(size, filt)
            if window:
                r = r.crop(window)
        ms.append((time.perf_counter() - t) * 1e3)
    return sorted(ms)[len(ms) // 2]


def resize_rows(run, iters, warmup, with_pillow):
    rng = np.random.default_rng(0)
    for name, filt, in_wh, size, window, batches in SHAPES:
        for b in batches:
            p = plan(filt, in_wh, size, window)
            imgs = rng.integers(0, 256, (b, in_wh[1], in_wh[0], 3), dtype=np.uint8)
            x = torch.from_numpy(imgs).to(DEV)
            out = resize.pil_resize(x, size, filt, window=window)
            med, best = timed(lambda: resize.pil_resize(x, size, filt, window=window, out=out), iters, warmup)
            nbytes = b * p["bytes_moved"]
            row = {"what": "pil_resize", "run": run, "shape": name, "filter": NAMES[filt], "batch": b, "two_launch_ms": round(med, 4),
                   "two_launch_best_ms": round(best, 4), "fused_ms": None, "mbytes": round(nbytes / 1e6, 2),
                   "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3), "frac_of_hbm": round(nbytes / (med * 1e-3) / 1e12 / HBM_TBS, 4),
                   "pillow_cpu_ms": round(pillow_ms(imgs, filt, size, window, 3), 2) if with_pillow else None}
            print(json.dumps(row), flush=True)
            del x, out


def pipeline_rows(run, stages, iters, warmup):
    from e4s_amd import kernels as K
    from e4s_amd import synth
    from e4s_amd.pipeline import FaceSwapPipeline
    pipe = FaceSwapPipeline(*stages, batch=1, graph=True, any_size=True)
    row = {"what": "FaceSwapPipeline.swap(any_size=True)", "run": run, "batch": 1, "precision": K.PRECISION}
    for side in (1024, 512):
        src = synth.synth_sr_input_u8(1, side, side, seed=5)[0].to(DEV)
        tgt = synth.synth_sr_input_u8(1, side, side, seed=6).to(DEV)
        med, best = timed(lambda: pipe.swap(src, tgt), iters, warmup)
        row[f"inputs_{side}_ms"], row[f"inputs_{side}_best_ms"] = round(med, 3), round(best, 3)
    print(json.dumps(row), flush=True)
    pipe.validate()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--no-pillow", action="store_true")
    a = ap.parse_args()
    for name, filt, in_wh, size, window, batches in SHAPES:
        print(json.dumps({"what": "plan", "shape": name, "filter": NAMES[filt], "window": window, **plan(filt, in_wh, size, window)}), flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench: needs the GPU (no CPU timing of the kernels is meaningful)")
    with torch.no_grad():
        for run in range(a.runs):
            resize_rows(run, a.iters, a.warmup, not a.no_pillow)
        if not a.no_pipeline:
            from tools.pipeline_bench import build_stages
            stages = build_stages()
            for run in range(a.runs):
                pipeline_rows(run, stages, a.iters, a.warmup)


if __name__ == "__main__":
    main()
