"""Times the native latent optimisation (e4s_amd.invert.LatentOptimizer) with HIP events: does a batched step cost less per image?

    python tools/invert_bench.py [--steps 30] [--batches 1,2,4,8] [--no-kernels] [--no-leg]

LatentOptimizer at 1024^2 with Net3 and the three loss networks at synthetic weights (the speed does not depend on their values), the
script's default objective (l2 + 0.8 LPIPS at 1024 / 512 / 256 + 0.1 ID + 0.1 parsing), fresh noise, Adam, the step replayed as one
HIP graph, B = 1, 2, 4, 8 images per step, both arithmetics (E4S_PRECISION f32 and bf16x3).  An event is recorded after every step is
enqueued (invert's on_step); a step's time is the distance between two consecutive events of replayed steps, the host running ahead
of the device; the median of `steps` of them is reported per step and per image.  Beside it, at B = 1, bench.py's optimisation_leg:
the loop this module replaces (same networks, same objective, no loss log, l2 first), by its own host clock.  Then the optimiser
kernels alone -- e4s_sgd_multi_dev_f32 without and with momentum, e4s_adamax_multi_dev_f32, and e4s_adam_multi_dev_f32 for scale --
on one [8,12,1280] latent and on Net3's parameter tensors, each call between its own pair of events, with bytes / time beside 8 TB/s;
bytes per element: SGD 12 (g read; p read and written), with momentum 20, Adamax and Adam 28.  e4s_scalar_log_f32 alone, 7 scalars.
One JSON line per row."""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("E4S_ALLOW_UNINITIALIZED_LOSS_NETS", "1")

from e4s_amd import kernels as K, synth  # noqa: E402

PEAK_HBM_TBPS = 8.0
SIZE = 1024


def median(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2]


def timed_calls(fn, iters=30, warmup=3):
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


def build_world(dev):
    from e4s_amd.criteria import FaceParsingLoss, IDLoss, LPIPS
    from e4s_amd.networks import Net3
    from e4s_amd.options import make_opts
    net = Net3(make_opts(out_size=SIZE))
    net.load_state_dict(synth.synth_state_dict(SIZE, 13), strict=True)
    net.latent_avg = synth.synth_latent_avg(SIZE).to(dev)
    net = net.to(dev).eval()
    lp, idl, fpl = LPIPS(), IDLoss(types.SimpleNamespace(id_loss_multiscale=True)), FaceParsingLoss(types.SimpleNamespace())
    for m, tag in ((lp, "lp."), (idl, "id."), (fpl, "fp.")):
        m.load_state_dict(synth.synth_module_state_dict(m, 0, tag))
    return net, {"lpips": lp.to(dev).eval(), "id": idl.to(dev).eval(), "parsing": fpl.to(dev).eval()}


def invert_rows(net, crit, batches, steps, dev):
    from e4s_amd.invert import WARMUP, LatentOptimizer
    skip = WARMUP + 3                                          # the warm-ups, the first replays
    for prec in ("f32", "bf16x3"):
        K.PRECISION = prec
        for b in batches:
            img = synth.synth_image(b, SIZE, seed=100, tag="bench_t").to(dev)
            mask = synth.onehot(synth.synth_labels_face(b, 512, seed=302)).to(dev)
            events = []

            def on_step(step):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                events.append(e)
            torch.manual_seed(1234)
            res = LatentOptimizer(net, crit, W_steps=skip + steps).invert(img, mask, on_step=on_step)
            torch.cuda.synchronize()
            ms = [events[i].elapsed_time(events[i + 1]) for i in range(skip - 1, skip + steps - 1)]
            hist = res.history.cpu()
            row = {"what": "LatentOptimizer step", "precision": prec, "batch": b, "steps": len(ms), "ms_per_step": round(median(ms), 3),
                   "best_ms": round(min(ms), 3), "ms_per_step_per_image": round(median(ms) / b, 3),
                   "loss_first": round(float(hist[0, 6]), 5), "loss_last": round(float(hist[-1, 6]), 5),
                   "finite": bool(torch.isfinite(hist).all())}
            print(json.dumps(row), flush=True)
            del res, img, mask
            torch.cuda.empty_cache()


def leg_rows(net, steps, dev):
    import bench
    one = bench.build_inputs(1, dev, seed_base=100)
    for prec in ("f32", "bf16x3"):
        K.PRECISION = prec
        ms = bench.optimisation_leg(net, one, steps, "full", graphed=True)
        print(json.dumps({"what": "bench.optimisation_leg (host clock)", "precision": prec, "batch": 1, "steps": steps, "ms_per_step": ms}),
              flush=True)


def kernel_rows(dev):
    spec = [(k, s, kind) for k, s, kind in synth.net3_param_spec() if kind not in ("blur", "blur1", "noisebuf")]
    sets = {"latent [8,12,1280]": [torch.randn(8, 12, 1280, device=dev)],
            f"Net3 ({len(spec)} tensors)": [synth.synth_tensor(k, s, kind, 0).to(dev) for k, s, kind in spec]}
    lr_dev = torch.full((1,), 1e-4, device=dev, dtype=torch.float64)
    for name, ps in sets.items():
        n = sum(p.numel() for p in ps)
        gs = [torch.randn_like(p) * 0.1 for p in ps]
        s1, s2 = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
        flat = torch.ones(len(ps), device=dev, dtype=torch.int64)
        steps = [flat[i:i + 1] for i in range(len(ps))]
        calls = {
            "e4s_sgd_multi_dev_f32 momentum 0": (12, lambda: K.sgd_multi_dev(ps, gs, None, 1e-4, 0.0, 0.0, 0.0, lr_dev=lr_dev)),
            "e4s_sgd_multi_dev_f32 momentum 0.9": (20, lambda: K.sgd_multi_dev(ps, gs, s1, 1e-4, 0.9, 0.0, 0.0, lr_dev=lr_dev)),
            "e4s_adamax_multi_dev_f32": (28, lambda: K.adamax_multi_dev(ps, gs, s1, s2, steps, 1e-4, 0.9, 0.999, 1e-8, 0.0, lr_dev=lr_dev)),
            "e4s_adam_multi_dev_f32": (28, lambda: K.adam_multi_dev(ps, gs, s1, s2, steps, 1e-4, 0.9, 0.999, 1e-8, 0.0, lr_dev=lr_dev)),
        }
        for what, (bpe, fn) in calls.items():
            med, best = timed_calls(fn)
            nbytes = bpe * n
            print(json.dumps({"what": what, "on": name, "elements": n, "launches": -(-len(ps) // 48), "bytes": nbytes, "ms": round(med, 4),
                              "best_ms": round(best, 4), "TBps": round(nbytes / med / 1e9, 3),
                              "of_8TBps": round(nbytes / med / 1e9 / PEAK_HBM_TBPS, 4)}), flush=True)
        del gs, s1, s2
    vals = [torch.zeros(1, device=dev) for _ in range(7)]
    log, step = torch.zeros(200, 7, device=dev), torch.ones(1, device=dev, dtype=torch.int64)
    med, best = timed_calls(lambda: K.scalar_log(vals, step, log))
    print(json.dumps({"what": "e4s_scalar_log_f32", "scalars": 7, "ms": round(med, 4), "best_ms": round(best, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-leg", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("invert_bench: needs the GPU (no CPU timing is meaningful)")
    dev = torch.device("cuda", torch.cuda.current_device())
    net, crit = build_world(dev)
    invert_rows(net, crit, [int(b) for b in a.batches.split(",")], a.steps, dev)
    if not a.no_leg:
        leg_rows(net, a.steps, dev)
    K.PRECISION = os.environ.get("E4S_PRECISION", "auto")
    if not a.no_kernels:
        kernel_rows(dev)


if __name__ == "__main__":
    main()
