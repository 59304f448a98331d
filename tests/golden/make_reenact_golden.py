"""Fixture of the face-vid2vid pose front end (e4s_amd/reenact.py): the REFERENCE's own KPDetector, HEEstimator (modules/
keypoint_detector.py, modules/util.py) and headpose_pred_to_degree / get_rotation_matrix / keypoint_transformation (driven_demo.py) run in
fp64 on the CPU, imported where they lie (src/pretrained/face_vid2vid/; yaml, scipy, imageio, skimage and the other absent third-party
packages are stubbed by oracle/ref_shim.stub_third_party).  keypoint_transformation sends its fixed angles to .cuda(); the script makes
Tensor.cuda a no-op while it runs, and sets the default dtype to float64 so that the reference's own torch.tensor / FloatTensor
constants do not pull the fp64 run down to fp32.

Weights: synth.synth_vid2vid_state_dict(module, seed), the same seeded tensors the tests load into e4s_amd.reenact.  Inputs are recorded
as seeds, never as tensors: frames are synth.synth_vid2vid_frames(b, h, w, seed) (float32 [b,h,w,3] in [0,1]).

Recorded:
    kp.keys / kp.shapes, he.keys / he.shapes   the reference's state_dicts at the shipped vox-256.yaml parameters (built on `meta`)
    aa.weight                                  AntiAliasInterpolation2d(3, 0.25).weight[0, 0] (13 x 13, the reference's float32 build)
    kp<j>.* (j = 1: estimate_jacobian, 0: not) the reduced KPDetector (KP_CFG) on frame A (64 x 48): tap.<name> = the fp64 output of each
                                               down / up block at every position and every TAP_CSTEP-th channel with
                                               tap.<name>.scale = max |.| of the whole map; logits (fp64, [15,4,16,8]); jmaps.scale;
                                               value, jacobian (fp64); e32 = max |fp32 forward - fp64 forward| of the reference itself
                                               for logits, value, jacobian
    he.<A|B|C>.*                               HEEstimator(64, num_kp 15, 66 bins) on frame A, on two 64 x 64 frames (B) and on a 75 x 61
                                               frame (C): yaw / pitch / roll / t / exp (fp64), degrees [b,3], and value / jacobian =
                                               keypoint_transformation(kp1's canonical keypoints, these) ; he.e32 on frame C
    kt                                         keypoint_transformation cases on seeded fp64 inputs: plain, without jacobian, free_view
                                               with all, some and no angles fixed
The script asserts while it generates: every tapped stage has max |.| within [1e-2, 1e3]; no heat map puts more than 0.9 of its mass on
one voxel; every angle lies at least 3 degrees inside (-99, 96).

Run in the build container:  python tests/golden/make_reenact_golden.py   (writes tests/golden/reenact.pt)"""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

KP_CFG = dict(block_expansion=32, max_features=128, num_blocks=3, reshape_depth=4, reshape_channel=512, num_kp=15, scale_factor=0.25,
              temperature=0.1, feature_channel=32, image_channel=3)
KP_SHIPPED = dict(temperature=0.1, block_expansion=32, max_features=1024, scale_factor=0.25, num_blocks=5, reshape_channel=16384,
                  reshape_depth=16, num_kp=15, image_channel=3, feature_channel=32, estimate_jacobian=False)
HE_SHIPPED = dict(block_expansion=64, max_features=2048, num_bins=66, num_kp=15, image_channel=3, feature_channel=32, estimate_jacobian=False)
FRAME_A = (1, 64, 48, 61)          # batch, h, w, seed
FRAME_B = (2, 64, 64, 62)
FRAME_C = (1, 75, 61, 63)
TAP_CSTEP = 8
KP_SEED, HE_SEED = 11, 12


def reference_modules():
    """(keypoint_detector module, driven_demo module) of the reference, offline on CPU."""
    from oracle import ref_shim
    ref_shim.stub_third_party()
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [ref_shim.REF_ROOT] + [p for p in saved if not os.path.isfile(os.path.join(p or os.getcwd(), "src", "__init__.py"))]
    try:
        import importlib
        return (importlib.import_module("src.pretrained.face_vid2vid.modules.keypoint_detector"),
                importlib.import_module("src.pretrained.face_vid2vid.driven_demo"))
    finally:
        sys.path[:] = saved


def to64(sd):
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def nchw(frames):
    return frames.permute(0, 3, 1, 2).contiguous()


def transform(dd, kp, he, **kw):
    """The reference's keypoint_transformation with Tensor.cuda a no-op; he is copied, since the reference reshapes he['t'] in place."""
    saved = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        return dd.keypoint_transformation({k: v.clone() for k, v in kp.items()}, {k: v.clone() for k, v in he.items()}, **kw)
    finally:
        torch.Tensor.cuda = saved


def main():
    from e4s_amd import synth
    kd, dd = reference_modules()
    out = {"frame_A": FRAME_A, "frame_B": FRAME_B, "frame_C": FRAME_C, "kp_cfg": KP_CFG, "kp_seed": KP_SEED, "he_seed": HE_SEED,
           "tap_cstep": TAP_CSTEP}
    with torch.device("meta"):
        kp_full, he_full = kd.KPDetector(**KP_SHIPPED), kd.HEEstimator(**HE_SHIPPED)
    for name, net in (("kp", kp_full), ("he", he_full)):
        out[name + ".keys"] = list(net.state_dict().keys())
        out[name + ".shapes"] = [tuple(v.shape) for v in net.state_dict().values()]
    out["kp_shipped"], out["he_shipped"] = KP_SHIPPED, HE_SHIPPED
    out["aa.weight"] = kd.AntiAliasInterpolation2d(3, 0.25).weight[0, 0].clone()

    frames = {tag: nchw(synth.synth_vid2vid_frames(*f)).double() for tag, f in (("A", FRAME_A), ("B", FRAME_B), ("C", FRAME_C))}   # (made under
    xa = frames["A"]                                                         # the float32 default dtype, as the tests make them)
    torch.set_default_dtype(torch.float64)
    canonical = None
    with torch.no_grad():
        for jac in (1, 0):
            torch.set_default_dtype(torch.float32)
            net32 = kd.KPDetector(**KP_CFG, estimate_jacobian=bool(jac)).eval()
            sd = synth.synth_vid2vid_state_dict(net32, seed=KP_SEED)
            net32.load_state_dict(sd, strict=True)
            torch.set_default_dtype(torch.float64)
            net = kd.KPDetector(**KP_CFG, estimate_jacobian=bool(jac)).eval().double()
            net.load_state_dict(to64(sd), strict=True)
            taps, pre = {}, f"kp{jac}."
            for n, m in list(net.predictor.down_blocks.named_children()) + list(net.predictor.up_blocks.named_children()):
                m.register_forward_hook(lambda mod, i, o, n=n: taps.update({n: o}))
            net.kp.register_forward_hook(lambda mod, i, o: taps.update({"logits": o}))
            if jac:
                net.jacobian.register_forward_hook(lambda mod, i, o: taps.update({"jmaps": o}))
            res = net(xa)
            logits = taps.pop("logits")
            jmaps = taps.pop("jmaps", None)
            for n, t in taps.items():
                scale = float(t.abs().max())
                assert math.isfinite(scale) and 1e-2 <= scale <= 1e3, (n, scale)
                print(f"{pre}stage {n}: shape {tuple(t.shape)} max |.| {scale:.4g}")
                out[f"{pre}tap.{n}"] = t[0, ::TAP_CSTEP].clone()
                out[f"{pre}tap.{n}.scale"] = scale
            heat = torch.softmax(logits.view(1, logits.shape[1], -1) / KP_CFG["temperature"], dim=2)
            print(f"{pre}logits {tuple(logits.shape)} max |.| {float(logits.abs().max()):.4g}; largest heat-map voxel {float(heat.max()):.4g}")
            assert tuple(logits.shape) == (1, 15, 4, 16, 8) and float(heat.max()) <= 0.9
            out[pre + "logits"] = logits[0].clone()
            out[pre + "value"] = res["value"].clone()
            saved32 = torch.get_default_dtype()
            torch.set_default_dtype(torch.float32)
            taps32 = {}
            net32.kp.register_forward_hook(lambda mod, i, o: taps32.update({"logits": o}))
            res32 = net32(xa.float())
            torch.set_default_dtype(saved32)
            e32 = [float((taps32["logits"].double() - logits).abs().max()), float((res32["value"].double() - res["value"]).abs().max())]
            if jac:
                out[pre + "jmaps.scale"] = float(jmaps.abs().max())
                out[pre + "jacobian"] = res["jacobian"].clone()
                e32.append(float((res32["jacobian"].double() - res["jacobian"]).abs().max()))
                canonical = {"value": res["value"].clone(), "jacobian": res["jacobian"].clone()}
                print(f"{pre}jacobian maps max |.| {out[pre + 'jmaps.scale']:.4g}")
            out[pre + "e32"] = e32
            print(f"{pre}value max |.| {float(res['value'].abs().max()):.4g}, e32 {e32}")

        torch.set_default_dtype(torch.float32)
        he32 = kd.HEEstimator(block_expansion=64, feature_channel=32, num_kp=15, image_channel=3, max_features=2048, num_bins=66).eval()
        sd = synth.synth_vid2vid_state_dict(he32, seed=HE_SEED)
        he32.load_state_dict(sd, strict=True)
        torch.set_default_dtype(torch.float64)
        he = kd.HEEstimator(block_expansion=64, feature_channel=32, num_kp=15, image_channel=3, max_features=2048, num_bins=66).eval().double()
        he.load_state_dict(to64(sd), strict=True)
        for tag in ("A", "B", "C"):
            x = frames[tag]
            r = he(x)
            deg = torch.stack([dd.headpose_pred_to_degree(r[a]) for a in ("yaw", "pitch", "roll")], 1)
            assert float(deg.min()) >= -96 and float(deg.max()) <= 93, deg
            kt = transform(dd, canonical, r, estimate_jacobian=True)
            for k, v in r.items():
                scale = float(v.abs().max())
                assert 1e-2 <= scale <= 1e3, (k, scale)
                out[f"he.{tag}.{k}"] = v.clone()
            out[f"he.{tag}.degrees"], out[f"he.{tag}.value"], out[f"he.{tag}.jacobian"] = deg.clone(), kt["value"].clone(), kt["jacobian"].clone()
            print(f"he {tag}: degrees {deg.tolist()} raw scales {[round(float(v.abs().max()), 3) for v in r.values()]}")
            if tag == "C":
                torch.set_default_dtype(torch.float32)
                r32 = he32(x.float())
                torch.set_default_dtype(torch.float64)
                out["he.e32"] = [float((r32[k].double() - r[k]).abs().max()) for k in ("yaw", "pitch", "roll", "t", "exp")]
                print("he e32", out["he.e32"])

        # ---- keypoint_transformation on seeded inputs ----
        g = torch.Generator().manual_seed(77)
        cases = []
        for name, b, kw in (("plain", 2, dict(estimate_jacobian=True)), ("no_jacobian", 1, dict(estimate_jacobian=False)),
                            ("free_all", 1, dict(estimate_jacobian=True, free_view=True, yaw=20.0, pitch=-10.0, roll=5.0)),
                            ("free_some", 2, dict(estimate_jacobian=True, free_view=True, yaw=None, pitch=12.5, roll=None)),
                            ("free_default", 1, dict(estimate_jacobian=False, free_view=True)),
                            ("free_none", 2, dict(estimate_jacobian=True, free_view=True, yaw=None, pitch=None, roll=None))):
            kp = {"value": torch.rand(b, 15, 3, generator=g) * 2 - 1, "jacobian": torch.randn(b, 15, 3, 3, generator=g)}
            hd = {"yaw": torch.randn(b, 66, generator=g), "pitch": torch.randn(b, 66, generator=g), "roll": torch.randn(b, 66, generator=g),
                  "t": 0.1 * torch.randn(b, 3, generator=g), "exp": 0.05 * torch.randn(b, 45, generator=g)}
            r = transform(dd, kp, hd, **kw)
            cases.append(dict(name=name, kp=kp, he=hd, kwargs=kw, value=r["value"].clone(),
                              jacobian=None if r["jacobian"] is None else r["jacobian"].clone()))
        out["kt"] = cases
        out["rot"] = dict(yaw=torch.tensor([10.0, -40.0]), pitch=torch.tensor([5.0, 25.0]), roll=torch.tensor([-15.0, 60.0]))
        out["rot"]["mat"] = dd.get_rotation_matrix(out["rot"]["yaw"], out["rot"]["pitch"], out["rot"]["roll"]).clone()
    torch.set_default_dtype(torch.float32)

    path = os.path.join(HERE, "reenact.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "retinaface.pt"))


if __name__ == "__main__":
    main()
