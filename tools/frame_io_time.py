"""Time the frame I/O kernels of e4s_amd.align (csrc/align.hip) on the GPU and the same work through Pillow on this box's CPU.

    timeout -k 10 600 python tools/frame_io_time.py [--batch 8] [--size 1024] [--pil-repeats 3]

B frames at 1080p and at 2160p, faces of side S: the crop (uint8 only, and with the fp32 normalised output), the paste into a second
buffer and the paste in place.  Each figure is the median over `--repeats` windows of `--launches` back-to-back launches between two
HIP events, after a warm-up.  Bytes are counted from the shapes: every output byte once; of the inputs the crop's windows, the faces,
and for the out-of-place paste the whole frames; the in-place paste writes only the covered pixels.  `hbm_share` divides by the
8 TB/s peak (about 6.3 TB/s is achievable); a working set below the 256 MiB Infinity Cache is served from it, not from HBM, and is
marked so.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
L3_BYTES = 256 * 2 ** 20


def quads_for(b, h, w, rng):
    out = []
    for _ in range(b):
        c = np.array([w / 2, h / 2]) + rng.uniform(-0.1, 0.1, 2) * np.array([w, h])
        t = np.deg2rad(rng.uniform(-15, 15))
        x = 0.2 * h * np.array([np.cos(t), np.sin(t)])
        y = np.array([-x[1], x[0]])
        out.append(np.stack([c - x - y, c - x + y, c + x + y, c + x - y]))
    return np.stack(out)


def gpu_ms(fn, warmup, repeats, launches):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) / launches)
    return statistics.median(times), min(times), max(times)


def pil_ms(frames, quads, size, repeats):
    """crop_image's crop + QUAD transform and the paste-back lines of scripts/face_swap.py:313-327, frame by frame."""
    from PIL import Image
    from e4s_amd import align
    imgs = [Image.fromarray(f) for f in frames]
    inv = align.paste_parameters(quads, size)
    crop_t, paste_t = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        crops = []
        for img, quad in zip(imgs, quads):
            win = align.crop_window(quad, (img.size[1], img.size[0]), size)
            passed = quad - np.array(win[:2], dtype=np.float64) + 0.5
            crops.append(img.crop(win).transform((size, size), Image.QUAD, passed.flatten(), Image.BILINEAR))
        t1 = time.perf_counter()
        for img, face, coeffs in zip(imgs, crops, inv):
            rgba = face.convert("RGBA")
            dst = img.convert("RGBA")
            rgba.putalpha(255)
            dst.alpha_composite(rgba.transform(img.size, Image.PERSPECTIVE, coeffs, Image.BILINEAR))
        t2 = time.perf_counter()
        crop_t.append((t1 - t0) * 1e3), paste_t.append((t2 - t1) * 1e3)
    return statistics.median(crop_t), statistics.median(paste_t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--pil-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_io_time.py measures on the GPU; none is visible")
    from e4s_amd import align
    b, s = args.batch, args.size
    rng = np.random.default_rng(0)
    result = {"tool": "frame_io_time", "device": torch.cuda.get_device_name(0), "batch": b, "size": s, "hbm_peak_bytes_per_s": HBM_PEAK,
              "repeats": args.repeats, "launches_per_repeat": args.launches, "cases": {}}
    for name, (h, w) in (("1080p", (1080, 1920)), ("2160p", (2160, 3840))):
        frames_np = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
        quads = quads_for(b, h, w, rng)
        coeffs, windows = align.crop_parameters(quads, (h, w), s)
        frames = torch.from_numpy(frames_np).cuda()
        qc, win = torch.from_numpy(coeffs).cuda(), torch.from_numpy(windows).cuda()
        pc = torch.from_numpy(align.paste_parameters(quads, s)).cuda()
        faces = torch.empty(b, s, s, 3, device="cuda", dtype=torch.uint8)
        norm = torch.empty(b, 3, s, s, device="cuda", dtype=torch.float32)
        out = torch.empty_like(frames)
        align.crop_faces_by_coeffs(frames, qc, win, s, out=faces)
        out.zero_()                                                        # count the covered pixels: white faces onto black frames
        covered = int((align.paste_back_by_coeffs(torch.full_like(faces, 255), out, pc, out=out) != 0).any(-1).sum())
        window_bytes = int(((windows[:, 2] - windows[:, 0]) * (windows[:, 3] - windows[:, 1])).sum()) * 3
        face_bytes, frame_bytes = b * s * s * 3, b * h * w * 3
        runs = {
            "crop_u8": (lambda: align.crop_faces_by_coeffs(frames, qc, win, s, out=faces), window_bytes + face_bytes),
            "crop_u8_and_normalized": (lambda: align.crop_faces_by_coeffs(frames, qc, win, s, out=faces, out_normalized=norm),
                                       window_bytes + face_bytes + 4 * face_bytes),
            "paste_out_of_place": (lambda: align.paste_back_by_coeffs(faces, frames, pc, out=out), 2 * frame_bytes + face_bytes),
            "paste_in_place": (lambda: align.paste_back_by_coeffs(faces, frames, pc, out=frames), face_bytes + covered * 3),
        }
        case = {"frame_hw": [h, w], "covered_pixels": covered, "working_set_bytes": 2 * frame_bytes + 5 * face_bytes,
                "fits_infinity_cache": 2 * frame_bytes + 5 * face_bytes < L3_BYTES, "gpu": {}}
        for key, (fn, nbytes) in runs.items():
            med, lo, hi = gpu_ms(fn, args.warmup, args.repeats, args.launches)
            case["gpu"][key] = {"ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes": nbytes,
                                "bytes_per_s": round(nbytes / (med * 1e-3), 1), "hbm_share": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}
        crop_ms, paste_ms = pil_ms(frames_np, quads, s, args.pil_repeats)
        case["pil_cpu"] = {"crop_ms": round(crop_ms, 2), "paste_ms": round(paste_ms, 2), "threads": 1}
        result["cases"][name] = case
    print(json.dumps(result))


if __name__ == "__main__":
    main()
