"""Fixture of face-vid2vid's dense motion and 3-D feature warp (e4s_amd/reenact_warp.py): the REFERENCE's own DenseMotionNetwork and
OcclusionAwareSPADEGenerator (modules/dense_motion.py, modules/generator.py, modules/util.py) run in fp64 on the CPU, imported where
they lie (oracle/ref_shim stubs the absent third-party packages).  The SPADE decoder is replaced ON THE CONSTRUCTED OBJECT
(gen.decoder = torch.nn.Identity()), so the generator's 'prediction' is the decoder's input: fourth(third(warped)) * occlusion_map.

Weights: synth.synth_vid2vid_generator_state_dict(module, seed), the same seeded tensors the tests load into e4s_amd.reenact_warp
(chosen by key and shape; the reference's decoder.* entries are loaded too and never used).  Inputs are recorded as seeds: the
source is frame A of reenact.pt (synth.synth_vid2vid_frames(1, 64, 48, 61)); keypoints are synth.synth_vid2vid_keypoints(n, seed, jacobian) of CASES.

Reduced configuration (GEN_CFG): the smallest with every awkward property -- a 4 x 16 x 12 volume, an 80-channel hourglass input, a
112-channel tail, a 7-deep kernel on a 4-deep volume, non-square maps.  Cases: 'a' N = 1 without jacobians, 'b' N = 2 with
jacobians identity + 0.2 randn (|det| >= 0.3 asserted).

Recorded:
    gen.keys / gen.shapes, dm.keys / dm.shapes   the reference's state_dicts at the shipped vox-256.yaml parameters (built on `meta`;
                                                 gen.* includes decoder.*)
    src.tap.<name> (+ .scale)                    the source-only stages first, down0, down1, second, res0, res1, compressed: fp64,
                                                 every TAP_CSTEP-th channel, scale = max |.| of the whole map
    src.lip, comp.lip                            largest |difference| of adjacent voxels of the feature volume / the compressed
                                                 volume along (x, y, z)
    <case>.tap.<name> (+ .scale)                 hg_input, enc<i>, dec<j>, prediction, warped, third per driving sample, channels
                                                 ::TAP_CSTEP
    <case>.logits, .deformation, .occlusion_map  fp64, whole; <case>.mask: channels ::TAP_CSTEP (mask == softmax(logits) is asserted
                                                 here, so the tests rebuild the whole mask from the logits)
    <case>.feature (+ .scale)                    channels ::TAP_CSTEP
    <case>.e32                                   max |the reference in fp32 - in fp64| of logits, deformation, feature
    <case>.motion_max                            max |sparse motion| over the 16 grids
The script asserts while it generates: every tapped stage has max |.| in [1e-2, 1e3]; no voxel's largest mask weight exceeds 0.9 and
the mean largest weight is at least 0.15; between 1 % and 40 % of the final warp's sample points have a coordinate outside [-1, 1];
every sparse grid has an in-range sample; occlusion_map spans at least [0.2, 0.8].

Run in the build container:  python tests/golden/make_reenact_warp_golden.py   (writes tests/golden/reenact_warp.pt)"""
import importlib
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

DM_CFG = dict(block_expansion=32, max_features=128, num_blocks=2, reshape_depth=4, compress=4)
GEN_CFG = dict(image_channel=3, feature_channel=32, num_kp=15, block_expansion=32, max_features=128, num_down_blocks=2, reshape_channel=32,
               reshape_depth=4, num_resblocks=2, estimate_occlusion_map=True, dense_motion_params=DM_CFG)
GEN_SHIPPED = dict(image_channel=3, feature_channel=32, num_kp=15, estimate_jacobian=False, block_expansion=64, max_features=512,
                   num_down_blocks=2, reshape_channel=32, reshape_depth=16, num_resblocks=6, estimate_occlusion_map=True,
                   dense_motion_params=dict(block_expansion=32, max_features=1024, num_blocks=5, reshape_depth=16, compress=4))
FRAME_A = (1, 64, 48, 61)
TAP_CSTEP = 16
GEN_SEED = 21
# seeds: the first that meet every condition asserted below (with jacobians most seeds put more than 40 % of the 4-deep volume's sample
# points outside, or draw an ill-conditioned jacobian)
CASES = {"a": dict(n=1, jacobian=False, seed=31), "b": dict(n=2, jacobian=True, seed=50)}
SIZE_LIMIT = 1 << 20


def keypoints(case, dtype=torch.float32):
    """(kp_source, kp_driving) of a case: synth.synth_vid2vid_keypoints(n, seed, jacobian) in `dtype`"""
    from e4s_amd import synth
    c = CASES[case]
    cast = lambda d: {k: None if v is None else v.to(dtype) for k, v in d.items()}
    ks, kd = synth.synth_vid2vid_keypoints(c["n"], c["seed"], c["jacobian"])
    return cast(ks), cast(kd)


def reference_modules():
    from oracle import ref_shim
    ref_shim.stub_third_party()
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [ref_shim.REF_ROOT] + [p for p in saved if not os.path.isfile(os.path.join(p or os.getcwd(), "src", "__init__.py"))]
    try:
        return (importlib.import_module("src.pretrained.face_vid2vid.modules.generator"),
                importlib.import_module("src.pretrained.face_vid2vid.modules.dense_motion"))
    finally:
        sys.path[:] = saved


def to64(sd):
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def lipschitz(vol):
    """vol [C,D,H,W] -> largest |difference| of adjacent voxels along (x, y, z)"""
    return [float((vol[:, :, :, 1:] - vol[:, :, :, :-1]).abs().max()), float((vol[:, :, 1:] - vol[:, :, :-1]).abs().max()),
            float((vol[:, 1:] - vol[:, :-1]).abs().max())]


def build(gm, dtype, sd):
    torch.set_default_dtype(dtype)
    gen = gm.OcclusionAwareSPADEGenerator(**GEN_CFG).eval().to(dtype)
    gen.load_state_dict(to64(sd) if dtype == torch.float64 else sd, strict=True)
    gen.decoder = torch.nn.Identity()
    return gen


def forward(gen, x, kp_source, kp_driving, taps=None):
    n = kp_driving["value"].shape[0]
    rep = lambda t: None if t is None else t.repeat(n, *([1] * (t.dim() - 1)))
    hooks = []
    if taps is not None:
        dm, hg = gen.dense_motion_network, gen.dense_motion_network.hourglass
        hooks.append(dm.register_forward_hook(lambda mod, i, o: taps.update({"deformation": o["deformation"].clone()})))
        named = [("first", gen.first), ("second", gen.second), ("third", gen.third), ("prediction", hg), ("logits", dm.mask)]
        named += [(f"down{i}", m) for i, m in enumerate(gen.down_blocks)] + [(f"res{i}", m) for i, m in enumerate(gen.resblocks_3d)]
        named += [(f"enc{i}", m) for i, m in enumerate(hg.encoder.down_blocks)] + [(f"dec{j}", m) for j, m in enumerate(hg.decoder.up_blocks)]
        for name, m in named:
            hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: taps.update({name: o.clone()})))
        hooks.append(dm.norm.register_forward_hook(lambda mod, i, o: taps.update({"compressed": torch.relu(o)})))
        hooks.append(hg.register_forward_pre_hook(lambda mod, i: taps.update({"hg_input": i[0].clone()})))
        hooks.append(gen.third.register_forward_pre_hook(lambda mod, i: taps.update({"warped": i[0].clone()})))
    with torch.no_grad():
        out = gen(x.repeat(n, 1, 1, 1), {"value": kp_driving["value"], "jacobian": kp_driving["jacobian"]},
                  {"value": rep(kp_source["value"]), "jacobian": rep(kp_source["jacobian"])})
    for h in hooks:
        h.remove()
    return out


def main():
    from e4s_amd import synth
    gm, dmm = reference_modules()
    out = {"gen_cfg": GEN_CFG, "gen_shipped": GEN_SHIPPED, "frame_A": FRAME_A, "tap_cstep": TAP_CSTEP, "gen_seed": GEN_SEED, "cases": CASES}
    with torch.device("meta"):
        gen_full = gm.OcclusionAwareSPADEGenerator(**GEN_SHIPPED)
    out["gen.keys"], out["gen.shapes"] = list(gen_full.state_dict().keys()), [tuple(v.shape) for v in gen_full.state_dict().values()]
    dsd = gen_full.dense_motion_network.state_dict()
    out["dm.keys"], out["dm.shapes"] = list(dsd.keys()), [tuple(v.shape) for v in dsd.values()]

    frame = synth.synth_vid2vid_frames(*FRAME_A).permute(0, 3, 1, 2).contiguous()
    torch.set_default_dtype(torch.float32)
    sd = synth.synth_vid2vid_generator_state_dict(gm.OcclusionAwareSPADEGenerator(**GEN_CFG), seed=GEN_SEED)
    gen32, gen64 = build(gm, torch.float32, sd), build(gm, torch.float64, sd)
    cs = TAP_CSTEP

    def record(prefix, name, t):
        """t [C, ...] of one sample"""
        scale = float(t.abs().max())
        assert math.isfinite(scale) and 1e-2 <= scale <= 1e3, (prefix, name, scale)
        print(f"{prefix}stage {name}: shape {tuple(t.shape)} max |.| {scale:.4g}")
        out[f"{prefix}tap.{name}"] = t[::cs].clone()
        out[f"{prefix}tap.{name}.scale"] = scale

    for case, c in CASES.items():
        torch.set_default_dtype(torch.float64)
        ks, kd = keypoints(case, torch.float64)
        if c["jacobian"]:
            for j in (ks["jacobian"], kd["jacobian"]):
                assert float(torch.linalg.det(j).abs().min()) >= 0.3, torch.linalg.det(j)
        taps = {}
        res = forward(gen64, frame.double(), ks, kd, taps)
        n = c["n"]
        if case == "a":
            for name in ("first", "down0", "down1", "res0", "res1", "compressed"):
                record("src.", name, taps[name][0])
            record("src.", "second", taps["second"][0].view(32, 4, *taps["second"].shape[2:]))
            out["src.lip"], out["comp.lip"] = lipschitz(taps["res1"][0]), lipschitz(taps["compressed"][0])
            print("lip (x, y, z): volume", out["src.lip"], "compressed", out["comp.lip"])
        d, h, w = taps["res1"].shape[2:]
        logits, mask, deform, occ, feat = taps["logits"], res["mask"], taps["deformation"], res["occlusion_map"], res["prediction"]
        assert tuple(logits.shape) == (n, 16, d, h, w) and tuple(deform.shape) == (n, d, h, w, 3) and tuple(occ.shape) == (n, 1, h, w)
        assert tuple(taps["hg_input"].shape) == (n, 80, d, h, w) and tuple(taps["prediction"].shape) == (n, 112, d, h, w)
        assert float((torch.softmax(logits, 1) - mask).abs().max()) <= 1e-15
        for i in range(n):
            for name in ("hg_input", "enc0", "enc1", "dec0", "dec1", "prediction", "third"):
                record(f"{case}.{i}.", name, taps[name][i])
            record(f"{case}.{i}.", "warped", taps["warped"][i].view(32, d, h, w))
        top = mask.max(1).values
        print(f"{case}: logits max |.| {float(logits.abs().max()):.4g}; largest mask weight max {float(top.max()):.4g} mean {float(top.mean()):.4g}")
        assert float(top.max()) <= 0.9 and float(top.mean()) >= 0.15
        outside = float((deform.abs() > 1).any(-1).double().mean())
        print(f"{case}: {100 * outside:.1f} % of the warp's sample points leave [-1, 1]")
        assert 0.01 <= outside <= 0.40
        dm = gen64.dense_motion_network
        rep = lambda t: None if t is None else t.repeat(n, *([1] * (t.dim() - 1)))
        sparse = dm.create_sparse_motions(taps["compressed"], kd, {"value": rep(ks["value"]), "jacobian": rep(ks["jacobian"])})
        inside = (sparse.abs() <= 1).all(-1).view(n, 16, -1).any(-1)
        assert bool(inside.all()), inside
        out[f"{case}.motion_max"] = float(sparse.abs().max())
        print(f"{case}: occlusion in [{float(occ.min()):.3f}, {float(occ.max()):.3f}]; max |sparse motion| {out[f'{case}.motion_max']:.3f}")
        assert float(occ.min()) <= 0.2 and float(occ.max()) >= 0.8
        fscale = float(feat.abs().max())
        assert 1e-2 <= fscale <= 1e3
        out[f"{case}.logits"], out[f"{case}.deformation"], out[f"{case}.occlusion_map"] = logits.clone(), deform.clone(), occ.clone()
        out[f"{case}.mask"] = mask[:, ::cs].clone()
        out[f"{case}.feature"], out[f"{case}.feature.scale"] = feat[:, ::cs].clone(), fscale
        torch.set_default_dtype(torch.float32)
        ks32, kd32 = keypoints(case, torch.float32)
        t32 = {}
        r32 = forward(gen32, frame, ks32, kd32, t32)
        out[f"{case}.e32"] = [float((t32["logits"].double() - logits).abs().max()), float((t32["deformation"].double() - deform).abs().max()),
                              float((r32["prediction"].double() - feat).abs().max())]
        print(f"{case}: e32 (logits, deformation, feature) {out[f'{case}.e32']}; feature max |.| {fscale:.4g}")
    torch.set_default_dtype(torch.float32)

    path = os.path.join(HERE, "reenact_warp.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= SIZE_LIMIT


if __name__ == "__main__":
    main()
