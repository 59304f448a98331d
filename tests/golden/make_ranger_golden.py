"""Fixture of the Ranger optimiser (e4s_amd/optim.py:Ranger): the REFERENCE's own Ranger (src/training/ranger.py) run on CPU.

The class is imported from the file where it lies (it needs nothing but torch and math).  The reference casts gradient and
parameter with `.float()`, so a float64 parameter alone does not give a float64 run: the fp64 trajectory runs `step()` under
`mock.patch.object(torch.Tensor, "float", lambda s, *a, **k: s.double())`, and the script asserts that `exp_avg` came out float64.

Inputs are recorded as seeds, never as tensors:
    parameters          torch.randn(shape, generator=Generator().manual_seed(1), dtype=float32), drawn in the order of the case's list
    gradients, step t   torch.randn(shape, generator=<one generator, seed 2>, dtype=float32) * (0.1 + 0.3 t) + 0.5, drawn in the order of
                        the case's list on every step (t 0-based; a tensor without a gradient in a step still draws)
    14 steps, lr 1e-2 and the reference's defaults otherwise; group["lr"] = 3e-3 before step 9 (0-based); tensor 2 has grad = None in
    step 3 (0-based), so it ends at 13 steps and its Lookahead syncs fall on other steps than its neighbours'.
    case A  weight_decay 0     SHAPES
    case B  weight_decay 0.01  the tensors of SHAPES with fewer than 5 000 elements
Recorded:
    shapes, steps, lr, lr2, lr2_step, none_step, none_index, param_seed, grad_seed
    A / B: {"index": positions in SHAPES, "weight_decay", "final": the fp64 parameters after the last step (float64), "steps": final step
            counts, "e32": per tensor max |the reference's own fp32 run - its fp64 run|, "e32_all": their maximum, "moved": per tensor
            max |final - initial| of the fp64 run}
    radam: for steps 1..20, betas (0.95, 0.999), threshold 5: [(step, N_sma, step_size, adaptive)] as Python floats from the reference's
           formulas (ranger.py:133-142)
The script asserts e32_all < 1e-3 * lr for both cases (well-conditioned inputs) and that the fp64 run moved every tensor of more than 3
elements by more than 1e-2 -- except (6, 1), whose rows of one element centralise to a gradient of exactly 0 (it stays where it was in
case A and moves by the weight decay alone in case B).

Run in the build container:  python tests/golden/make_ranger_golden.py   (writes tests/golden/ranger.pt)"""
import importlib.util
import math
import os
import sys
from unittest import mock

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SHAPES = [(1, 8, 6, 3, 3), (1, 37, 33, 3, 3), (5, 7), (9, 4099), (3, 4096), (513, 27), (6, 1), (1, 3, 1, 1), (3,), (1,), (4097,),
          (64, 64, 3, 3)]
STEPS, LR, LR2, LR2_STEP, NONE_STEP, NONE_INDEX = 14, 1e-2, 3e-3, 9, 3, 2
PARAM_SEED, GRAD_SEED = 1, 2


def reference_ranger():
    from oracle import ref_shim
    path = os.path.join(ref_shim.REF_ROOT, "src", "training", "ranger.py")
    spec = importlib.util.spec_from_file_location("ref_training_ranger", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Ranger


def params(index, dtype):
    g = torch.Generator().manual_seed(PARAM_SEED)
    return [torch.randn(SHAPES[i], generator=g, dtype=torch.float32).to(dtype).requires_grad_(True) for i in index]


def run(Ranger, index, wd, dtype):
    ps = params(index, dtype)
    opt = Ranger(ps, lr=LR, weight_decay=wd)
    g = torch.Generator().manual_seed(GRAD_SEED)
    for t in range(STEPS):
        if t == LR2_STEP:
            opt.param_groups[0]["lr"] = LR2
        for j, i in enumerate(index):
            gr = torch.randn(SHAPES[i], generator=g, dtype=torch.float32) * (0.1 + 0.3 * t) + 0.5
            ps[j].grad = None if (t == NONE_STEP and i == NONE_INDEX) else gr.to(dtype)
        if dtype == torch.float64:
            with mock.patch.object(torch.Tensor, "float", lambda s, *a, **k: s.double()):
                opt.step()
        else:
            opt.step()
    if dtype == torch.float64:
        assert all(opt.state[p]["exp_avg"].dtype == torch.float64 for p in ps)
    return [p.detach() for p in ps], [int(opt.state[p]["step"]) for p in ps]


def radam_table():
    beta1, beta2, thr = 0.95, 0.999, 5
    rows = []
    for step in range(1, 21):
        beta2_t = beta2 ** step
        N_sma_max = 2 / (1 - beta2) - 1
        N_sma = N_sma_max - 2 * step * beta2_t / (1 - beta2_t)
        if N_sma > thr:
            step_size = math.sqrt((1 - beta2_t) * (N_sma - 4) / (N_sma_max - 4) * (N_sma - 2) / N_sma * N_sma_max / (N_sma_max - 2)) / (
                1 - beta1 ** step)
        else:
            step_size = 1.0 / (1 - beta1 ** step)
        rows.append((step, float(N_sma), float(step_size), bool(N_sma > thr)))
    return rows


def main():
    Ranger = reference_ranger()
    out = {"shapes": SHAPES, "steps": STEPS, "lr": LR, "lr2": LR2, "lr2_step": LR2_STEP, "none_step": NONE_STEP, "none_index": NONE_INDEX,
           "param_seed": PARAM_SEED, "grad_seed": GRAD_SEED, "radam": radam_table()}
    for name, wd, index in (("A", 0.0, list(range(len(SHAPES)))),
                            ("B", 0.01, [i for i, s in enumerate(SHAPES) if math.prod(s) < 5000])):
        p64, st64 = run(Ranger, index, wd, torch.float64)
        p32, st32 = run(Ranger, index, wd, torch.float32)
        assert st64 == st32 and all(p.dtype == torch.float64 for p in p64) and all(p.dtype == torch.float32 for p in p32)
        e32 = [float((a.double() - b).abs().max()) for a, b in zip(p32, p64)]
        start = params(index, torch.float64)
        # How far the fp64 run moved every tensor: more than 1e-2, except where the inputs leave the optimiser nothing to move.  (6, 1): rows
        # of one element centralise to a gradient of exactly 0 (no movement in case A, the weight decay alone in case B).  Tensors of at
        # most 3 elements: the largest of so few updates can stay under 1e-2 ((1, 3, 1, 1) keeps little of a gradient that is mostly its mean).
        moved = [float((a.detach() - b).abs().max()) for a, b in zip(start, p64)]
        assert all(m > 1e-2 for i, m in zip(index, moved) if math.prod(SHAPES[i]) > 3 and SHAPES[i] != (6, 1)), moved
        m61 = moved[index.index(SHAPES.index((6, 1)))]
        assert m61 == 0.0 if wd == 0 else 0 < m61 < 1e-2, m61
        out[name] = {"index": index, "weight_decay": wd, "final": p64, "steps": st64, "e32": e32, "e32_all": max(e32), "moved": moved}
        print(f"case {name}: {len(index)} tensors, steps {st64}, e32_all {max(e32):.2e}, movement {[round(m, 4) for m in moved]}")
        assert max(e32) < 1e-3 * LR, max(e32)
        assert st64[index.index(NONE_INDEX)] == STEPS - 1
    first_adaptive = next(r[0] for r in out["radam"] if r[3])
    print(f"first adaptive step {first_adaptive} (N_sma {out['radam'][first_adaptive - 1][1]:.3f})")
    assert first_adaptive == 6
    path = os.path.join(HERE, "ranger.pt")
    torch.save(out, path)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"wrote {path} ({size / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
