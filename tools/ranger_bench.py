"""HIP-event times of the fused Ranger step (e4s_amd/optim.py:Ranger) beside FusedAdam(capturable=True) on Net3's trainable parameters.

    python tools/ranger_bench.py [--rounds 36] [--warmup 6]

The parameter list is synth.net3_param_spec() without its buffers (344 tensors at the defaults), with seeded values and seeded
gradients that stay in place.  One round times, each bracketed by its own pair of events on the current stream after `warmup` untimed
rounds: a Ranger step eager, a FusedAdam step eager, a Ranger step replayed from a captured graph that holds only `opt.step()`, and a
FusedAdam step replayed likewise -- the two optimisers alternate within the run, so they see the same clocks.  The two Ranger
optimisers (eager, replayed) are separate instances over separate copies, so every round is step t of both: the rounds with
t % k == 0 are the Lookahead steps and are reported separately (with k = 6 one round in six).  The warm-up carries every optimiser
past step 6, so all timed Ranger steps take the adaptive branch.

Bytes per step, from the kernels' traffic per element: Adam 28 B (g read; p, m, v read and written); Ranger 32 B for a tensor whose
gradient is centralised (g is read a second time by the row sums) and 28 B otherwise, + 8 B (slow read and written) on a Lookahead
step.  Prints one JSON line per measurement (median, 10th / 90th percentile, bytes, TB/s), then a summary line: the replayed ordinary
Ranger step against the replayed Adam step of the same run and against the ratio of their bytes."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "p10_ms": ms[len(ms) // 10], "p90_ms": ms[(9 * len(ms)) // 10], "calls": len(ms)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def captured(opt):
    """A graph that holds only opt.step() (one eager step first: state, flat step counts and workspace exist before the capture)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        opt.step()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=36)
    ap.add_argument("--warmup", type=int, default=6)
    args = ap.parse_args()
    if args.rounds < 24 or args.warmup < 6:
        raise SystemExit("--rounds: 24 or more (four Lookahead steps), --warmup: 6 or more (past the momentum-only steps)")
    from e4s_amd import synth
    from e4s_amd.optim import FusedAdam, Ranger
    spec = [(k, s, kind) for k, s, kind in synth.net3_param_spec() if kind not in ("blur", "blur1", "noisebuf")]

    def params(seed):
        ps = []
        for key, shape, kind in spec:
            p = synth.synth_tensor(key, shape, kind, seed).cuda().requires_grad_(True)
            p.grad = (synth.synth_tensor(key + ".grad", shape, "randn", seed) * 0.1).cuda()
            ps.append(p)
        return ps

    sets = {"ranger eager": params(0), "ranger replayed": params(0), "adam eager": params(0), "adam replayed": params(0)}
    opts = {name: (Ranger(ps, lr=1e-4) if name.startswith("ranger") else FusedAdam(ps, lr=1e-4, capturable=True)) for name, ps in sets.items()}
    k = opts["ranger eager"].param_groups[0]["k"]
    n_all = sum(p.numel() for p in sets["adam eager"])
    n_gc = sum(p.numel() for p in sets["adam eager"] if Ranger.gc_rows(p.shape) is not None)
    bytes_of = {"adam": 28 * n_all, "ranger ordinary": 28 * n_all + 4 * n_gc, "ranger lookahead": 36 * n_all + 4 * n_gc}
    print(json.dumps({"what": "parameter list", "tensors": len(spec), "elements": n_all, "centralised_elements": n_gc, "bytes_per_step": bytes_of}),
          flush=True)
    opts["ranger eager"].step()                                        # every optimiser is at step 2 after this block
    opts["adam eager"].step()
    graphs = {name: captured(opts[name]) for name in ("ranger replayed", "adam replayed")}
    opts["ranger eager"].step()
    opts["adam eager"].step()
    for name in graphs:
        graphs[name].replay()
    step = 2
    run = {"ranger eager": opts["ranger eager"].step, "adam eager": opts["adam eager"].step,
           "ranger replayed": graphs["ranger replayed"].replay, "adam replayed": graphs["adam replayed"].replay}
    times = {}
    for r in range(args.warmup + args.rounds):
        step += 1
        for name in ("ranger eager", "adam eager", "ranger replayed", "adam replayed"):
            ms = timed(run[name])
            if r >= args.warmup:
                kind = name if name.startswith("adam") else name + (" lookahead" if step % k == 0 else " ordinary")
                times.setdefault(kind, []).append(ms)
    torch.cuda.synchronize()
    for name in ("ranger eager", "ranger replayed"):                   # the host's count of the steps is the device's
        st = opts[name].state[sets[name][0]]["step"]
        assert int(st.item()) == step, (name, int(st.item()), step)
    assert torch.equal(sets["ranger eager"][0].detach(), sets["ranger replayed"][0].detach())
    out = {}
    for kind in sorted(times):
        nbytes = bytes_of["adam"] if kind.startswith("adam") else bytes_of["ranger lookahead" if kind.endswith("lookahead") else "ranger ordinary"]
        r = stats(times[kind])
        r.update(what=kind, bytes=nbytes, tb_per_s=nbytes / r["median_ms"] / 1e9)
        out[kind] = r
        print(json.dumps(r), flush=True)
    want = bytes_of["ranger ordinary"] / bytes_of["adam"]
    got = out["ranger replayed ordinary"]["median_ms"] / out["adam replayed"]["median_ms"]
    print(json.dumps({"what": "ranger replayed ordinary / adam replayed", "time_ratio": got, "bytes_ratio": want,
                      "over_bytes_ratio": got / want, "within_25_percent": got <= 1.25 * want}), flush=True)


if __name__ == "__main__":
    main()
