"""Records tests/golden/style.pt: the reference's own StyleLoss (src/criteria/style_loss.py) in fp64 on the CPU, on the seeded synthetic
VGG16 weights, for the three cases of tests/style_cases.py:GOLDEN_CASES.

    python tests/golden/make_style_golden.py            (needs the reference checkout, $E4S_REFERENCE_ROOT)

The reference module is imported in place with the reference's `src` winning over this repo's overlay (the path handling of
oracle/ref_shim.py:reference_criteria, written out here).  torchvision is absent: a stub whose `models.vgg16` returns a module with the
restated `features` Sequential (e4s_amd.criteria.vgg16_features) and an empty `transforms` is put into sys.modules.  Inputs and weights are
regenerated from their seeds by the test; the fixture holds per case the loss, the per-layer terms, dL/dx (fp64), 16 x 16 sampled entries
of each Gram matrix of x, and the relative errors (loss, per-layer terms, L2 of dL/dx, sampled Gram entries) of the reference's own fp32
CPU run against its fp64 run -- the yardstick of the test's tolerances -- with, per layer, the largest Gram entry and the mean of
|G_x - G_xhat|, from which the test derives the tolerance of the per-layer terms."""
import importlib
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import style_cases as sc  # noqa: E402
from e4s_amd import synth  # noqa: E402
from e4s_amd.criteria import vgg16_features  # noqa: E402
from oracle.ref_shim import REF_ROOT  # noqa: E402

OUT = os.path.join(HERE, "style.pt")


def reference_style_loss():
    class _VGG16(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.features = vgg16_features()
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg16 = lambda *a, **k: _VGG16()
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.update({"torchvision": tv, "torchvision.models": tv.models, "torchvision.transforms": tv.transforms})
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [REF_ROOT] + [p for p in saved if not os.path.isfile(os.path.join(p or os.getcwd(), "src", "__init__.py"))]
    try:
        return importlib.import_module("src.criteria.style_loss")
    finally:
        sys.path[:] = saved
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]


def run(mod, case, dtype, grams=False):
    x, x_hat, mask = sc.golden_inputs(case)
    net = mod.StyleLoss(VGG16_ACTIVATIONS_LIST=case["taps"], normalize=case["normalize"], distance="l2")
    net.load_state_dict(synth.synth_vgg16_state_dict(seed=0, prefix="vgg16_act.features."), strict=False)
    keys = list(net.state_dict())
    net = net.to(dtype)
    if case["normalize"]:                     # normalize_img mixes its fp32 constants into the image: keep the run in `dtype`
        mean, std = (torch.from_numpy(v).to(dtype).view(1, 3, 1, 1) for v in (mod.VGG_MEAN, mod.VGG_STD))
        net.normalize_img = lambda t: ((t + 1) / 2 - mean) / std
    xv = x.to(dtype).requires_grad_(True)
    m = None if mask is None else mask.to(dtype)
    loss = net(xv, x_hat.to(dtype), mask_x=m, mask_x_hat=m)
    loss.backward()
    out = dict(loss=loss.detach().double(), grad=xv.grad.detach().double(), keys=keys)
    if grams:
        with torch.no_grad():
            a = torch.nn.functional.interpolate(x.to(dtype), size=(256, 256), mode="bilinear")
            b = torch.nn.functional.interpolate(x_hat.to(dtype), size=(256, 256), mode="bilinear")
            if case["normalize"]:
                a, b = net.normalize_img(a), net.normalize_img(b)
            if m is not None:
                mr = torch.nn.functional.interpolate(m, size=(256, 256), mode="bilinear")
                a, b = a * mr, b * mr
            ga = [net.gram_matrix(f) for f in net.vgg16_act(a)]
            gb = [net.gram_matrix(f) for f in net.vgg16_act(b)]
            out["terms"] = torch.stack([torch.nn.functional.mse_loss(p, q) for p, q in zip(ga, gb)]).double()
            out["grams"] = []
            for p in ga:
                rows, cols = sc.gram_sample_index(p.shape[0])
                out["grams"].append(p[rows][:, cols].double().clone())
            # what the per-layer tolerance of the test is made of: the largest Gram entry and the mean |G_x - G_xhat|
            out["gram_max"] = [float(max(p.abs().max(), q.abs().max())) for p, q in zip(ga, gb)]
            out["d_absmean"] = [float((p - q).abs().mean()) for p, q in zip(ga, gb)]
    return out


def main():
    torch.manual_seed(0)
    mod = reference_style_loss()
    rec = {}
    for case in sc.GOLDEN_CASES:
        r64 = run(mod, case, torch.float64, grams=True)
        r32 = run(mod, case, torch.float32, grams=True)
        rel_loss = abs(float(r32["loss"]) - float(r64["loss"])) / abs(float(r64["loss"]))
        rel_grad = float((r32["grad"] - r64["grad"]).norm() / r64["grad"].norm())
        assert abs(float(r64["terms"].mean()) - float(r64["loss"])) <= 1e-12 * float(r64["loss"])
        rel_terms = ((r32["terms"] - r64["terms"]).abs() / r64["terms"]).tolist()
        rel_grams = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(r32["grams"], r64["grams"])]      # sampled entries, to the largest
        rec[case["name"]] = dict(loss=r64["loss"], terms=r64["terms"], grad=r64["grad"], grams=r64["grams"],
                                 ref_f32_rel_loss=rel_loss, ref_f32_rel_grad=rel_grad, ref_f32_rel_terms=rel_terms, ref_f32_rel_grams=rel_grams,
                                 gram_max=r64["gram_max"], d_absmean=r64["d_absmean"])
        print("   fp32 rel terms", rel_terms, "fp32 rel grams", rel_grams)
        print(case["name"], "loss", float(r64["loss"]), "terms", r64["terms"].tolist(), "fp32 rel loss", rel_loss, "fp32 rel grad", rel_grad,
              "grad norm", float(r64["grad"].norm()), flush=True)
    rec["state_dict_keys"] = r64["keys"]
    torch.save(rec, OUT)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), f"{OUT}: {size} bytes, above the 1 MiB limit for a committed file"
    print(OUT, size, "bytes")


if __name__ == "__main__":
    main()
