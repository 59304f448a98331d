"""Fixture of face-vid2vid's SPADE decoder (e4s_amd/spade.py): the REFERENCE's own SPADEDecoder (modules/generator.py:121-159,
modules/util.py:419-481) run in fp64 and fp32 on the CPU, imported where it lies (oracle/ref_shim stubs the absent third-party
packages).  Nothing of the reference is copied; taps come from forward hooks on the constructed object.

Weights: synth.synth_vid2vid_decoder_state_dict(module, DEC_SEED), the same seeded tensors the tests load into e4s_amd.spade.SPADEDecoder
(chosen by key and shape).  Inputs are recorded as seeds: synth.synth_vid2vid_decoder_feature(n, h, w, seed) of CASES.  The channel
counts are hard-coded in the reference, so only the map is reduced: 'a' N = 1 on 6 x 5 (30 rows: less than one 128-row tile), 'b' N = 2
on 9 x 7 (63 / 252 / 1008 rows per sample at the three resolutions: partial last tiles, and tiles that hold rows of both samples).

Recorded:
    dec.keys / dec.shapes                    the reference decoder's state_dict
    weight.up_1.conv_s                       the fp64 effective weight (the module's .weight after an eval forward), whole [64,256,1,1]
    weight.G_middle_0.conv_0 (+ .rows, .cols) the same of G_middle_0.conv_0 seen as [512, 4608]: rows ::16, columns ::16.  (Whole rows
                                             would be 1.2 MB, more than a committed file may hold; the fold divides the whole tensor by one
                                             scalar, so a grid of its entries pins that scalar as well as whole rows do.)
    sigma_ratio.<block>                      sigma / true 2-norm of the two 1x1 shortcuts
    <case>.tap.<name> (+ .scale)             fp64, channels ::TAP_CSTEP, scale = max |.| of the whole map: fc, every block's output,
                                             G_middle_0.norm_0, G_middle_3.conv_0, up_0.norm_s, up_1.norm_1
    <case>.logits (+ .scale)                 conv_img's output, whole.  prediction == sigmoid(logits) is asserted here to 1e-15, so the
                                             tests rebuild the whole prediction from the logits (it would not fit beside them)
    <case>.e32                               {tap: max |the reference in fp32 - in fp64|}, 'logits' and 'prediction' included
The script asserts while it generates: every tap's scale is in [1e-2, 1e3]; prediction reaches below 0.3 and above 0.7; sigma / true
2-norm is in [0.7, 1) for the two 1x1 shortcuts; e32 <= 1e-5 x scale at every tap.

Run in the build container:  python tests/golden/make_spade_golden.py   (writes tests/golden/spade.pt)"""
import importlib
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

TAP_CSTEP = 16
DEC_SEED = 5
CASES = {"a": dict(n=1, h=6, w=5, seed=11), "b": dict(n=2, h=9, w=7, seed=12)}
TAPS = ["fc"] + [f"G_middle_{i}" for i in range(6)] + ["up_0", "up_1", "G_middle_0.norm_0", "G_middle_3.conv_0", "up_0.norm_s", "up_1.norm_1"]
SIZE_LIMIT = 1 << 20


def reference_generator_module():
    from oracle import ref_shim
    ref_shim.stub_third_party()
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [ref_shim.REF_ROOT] + [p for p in saved if not os.path.isfile(os.path.join(p or os.getcwd(), "src", "__init__.py"))]
    try:
        return importlib.import_module("src.pretrained.face_vid2vid.modules.generator")
    finally:
        sys.path[:] = saved


def build(gm, dtype, sd):
    torch.set_default_dtype(dtype)
    dec = gm.SPADEDecoder().eval().to(dtype)
    dec.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    return dec


def forward(dec, x):
    taps, hooks = {}, []
    mods = dict(dec.named_modules())
    for name in TAPS:
        hooks.append(mods[name].register_forward_hook(lambda mod, i, o, name=name: taps.update({name: o.detach().clone()})))
    hooks.append(dec.conv_img.register_forward_hook(lambda mod, i, o: taps.update({"logits": o.detach().clone()})))
    with torch.no_grad():
        taps["prediction"] = dec(x)
    for h in hooks:
        h.remove()
    return taps


def main():
    from e4s_amd import synth
    gm = reference_generator_module()
    torch.set_default_dtype(torch.float32)
    ref = gm.SPADEDecoder()
    out = {"tap_cstep": TAP_CSTEP, "dec_seed": DEC_SEED, "cases": CASES, "taps": TAPS}
    out["dec.keys"], out["dec.shapes"] = list(ref.state_dict().keys()), [tuple(v.shape) for v in ref.state_dict().values()]
    sd = synth.synth_vid2vid_decoder_state_dict(ref, seed=DEC_SEED)
    dec32, dec64 = build(gm, torch.float32, sd), build(gm, torch.float64, sd)

    for case, c in CASES.items():
        x = synth.synth_vid2vid_decoder_feature(c["n"], c["h"], c["w"], c["seed"])
        torch.set_default_dtype(torch.float64)
        t64 = forward(dec64, x.double())
        torch.set_default_dtype(torch.float32)
        t32 = forward(dec32, x)
        e32 = {}
        for name in TAPS + ["logits"]:
            t = t64[name]
            scale = float(t.abs().max())
            assert math.isfinite(scale) and 1e-2 <= scale <= 1e3, (case, name, scale)
            e32[name] = float((t32[name].double() - t).abs().max())
            print(f"{case} {name}: shape {tuple(t.shape)} max |.| {scale:.4g} e32 {e32[name]:.3g} = {e32[name] / scale:.3g} x scale")
            assert e32[name] <= 1e-5 * scale, (case, name, e32[name], scale)
            if name == "logits":
                out[f"{case}.logits"], out[f"{case}.logits.scale"] = t.clone(), scale
            else:
                out[f"{case}.tap.{name}"], out[f"{case}.tap.{name}.scale"] = t[:, ::TAP_CSTEP].clone(), scale
        pred = t64["prediction"]
        assert tuple(pred.shape) == (c["n"], 3, 4 * c["h"], 4 * c["w"])
        assert float((torch.sigmoid(t64["logits"]) - pred).abs().max()) <= 1e-15
        e32["prediction"] = float((t32["prediction"].double() - pred).abs().max())
        print(f"{case} prediction in [{float(pred.min()):.3f}, {float(pred.max()):.3f}], e32 {e32['prediction']:.3g}")
        assert float(pred.min()) < 0.3 and float(pred.max()) > 0.7 and e32["prediction"] <= 1e-5
        out[f"{case}.e32"] = e32

    # the effective weights: the reference module's .weight after the eval forward above
    out["weight.up_1.conv_s"] = dec64.up_1.conv_s.weight.detach().clone()
    w0 = dec64.G_middle_0.conv_0.weight.detach()
    out["weight.G_middle_0.conv_0"] = w0.reshape(w0.shape[0], -1)[::16, ::16].clone()
    out["weight.G_middle_0.conv_0.rows"], out["weight.G_middle_0.conv_0.cols"] = 16, 16
    for name in ("up_0", "up_1"):
        conv = getattr(dec64, name).conv_s
        wm = conv.weight_orig.detach().reshape(conv.weight_orig.shape[0], -1)
        sigma = float(torch.dot(conv.weight_u, torch.mv(wm, conv.weight_v)))
        ratio = sigma / float(torch.linalg.matrix_norm(wm, 2))
        print(f"{name}.conv_s: sigma / true 2-norm {ratio:.4f}")
        assert 0.7 <= ratio < 1.0, (name, ratio)
        out[f"sigma_ratio.{name}"] = ratio

    path = os.path.join(HERE, "spade.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= SIZE_LIMIT


if __name__ == "__main__":
    main()
