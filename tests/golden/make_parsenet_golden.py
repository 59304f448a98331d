"""Fixture of GPEN's ParseNet (e4s_amd/parsenet.py): the REFERENCE's own ParseNet run on CPU in fp64.

Imports src/pretrained/gpen/face_parse/parse_model.py where it lies (it needs nothing but torch and numpy; absent third-party
packages of the packages above it are stubbed by oracle/ref_shim.stub_third_party).  Weights: synth.synth_parsenet_state_dict(net),
the same seeded tensors the tests load into e4s_amd.parsenet.ParseNet.

Recorded (inputs as seeds, never as tensors; an input is synth.synth_sr_input_u8(b, h, w, seed), RGB, fed to the net as
(x / 255 * 2 - 1 in fp64).float(), face_parsing.py:59-63):
    keys / shapes      the reference's state_dict of the full net ParseNet(512, 512, 32, 64, 19, 'bn', 'LeakyReLU', [32, 256])
    nets               constructor arguments (in_size, out_size, min_feat_size, res_depth) of the three nets
    cases              [(net index, b, seed)]: ParseNet(32, 32, 8, res_depth=2) at B = 2 (2 down / 2 up steps, all three block kinds),
                       ParseNet(64, 64, 32) at B = 1, the full 512^2 net at B = 1
    keys.<i> / shapes.<i>   the state_dict of net i
    rows.<i> / cols.<i>     the recorded rows / columns of case i (all of them for case 0; edges plus a stride otherwise)
    logits.<i>         the fp64 mask logits at those positions, stored as fp32 (the storage rounding, 2^-24 relative, is 3 orders
                       below the tightest bound that reads it)
    scale.<i>          max |logits64| over the whole output
    e32.<i>            max |fp32 forward - fp64 forward| of the reference itself on the recorded positions
    mask.<i>           the whole uint8 mask MASK_COLORMAP[argmax] of the fp64 logits (zlib, as tests/conftest.py:unz reads it)
    margin.<i>         per pixel, the fp64 margin |best logit of classes {0, 14, 18} - best logit of the rest| in units of
                       MARGIN_UNIT x scale, rounded DOWN and clipped to 255 (uint8, zlib): a pixel's mask cannot flip unless two
                       logits move by half its margin each
    mid.<name>         for the full net: the fp64 outputs (stored as fp32, NCHW) of the first down block (enc0), of the trunk
                       feat + body(feat) and of the first up block (dec0) at the rows / columns mid_rc.<name>, with their max |.|
                       in mid.<name>.scale, so that a failure of the whole net can be located
    ref5               get_reference_facial_points((512, 512), 0.25, (0, 0), True) of align_faces.py (float64 [5,2])
    lm.<name>          for four landmark sets (frontal, rotated 30 degrees, small, partly outside a 256 x 320 frame): pts [5,2] and
                       the reference's own _umeyama pair of align_faces.py:258-262 on float64 points, tfm and tfm_inv [2,3]
The script asserts that at most 1 % of the full net's pixels have a margin of 2 x 1e-3 x scale or less (the split-bf16 bound of
tests/test_gpu_parsenet.py) and that both mask values cover at least 5 % of it.

Run in the build container:  python tests/golden/make_parsenet_golden.py   (writes tests/golden/parsenet.pt)"""
import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

NETS = [(32, 32, 8, 2), (64, 64, 32, 10), (512, 512, 32, 10)]
CASES = [(0, 2, 41), (1, 1, 42), (2, 1, 43)]
MARGIN_UNIT = 1e-4
MASK_COLORMAP = [0, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 0, 255, 255, 255, 0]


def sample(n):
    if n <= 32:
        return list(range(n))
    return sorted(set(range(0, 4)) | set(range(n - 4, n)) | set(range(0, n, 37 if n > 64 else 5)) | {15, 16, 17})


def reference_parsenet():
    """The reference's ParseNet class, imported offline on CPU."""
    from oracle import ref_shim
    ref_shim.stub_third_party()
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [ref_shim.REF_ROOT] + [p for p in saved if not os.path.isfile(os.path.join(p or os.getcwd(), "src", "__init__.py"))]
    try:
        import importlib
        mod = importlib.import_module("src.pretrained.gpen.face_parse.parse_model")
    finally:
        sys.path[:] = saved
    return mod.ParseNet


def reference_align():
    """The reference's align_faces module (cv2 and skimage stubbed: only numpy code is called)."""
    from oracle import ref_shim
    ref_shim.stub_third_party()
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [ref_shim.REF_ROOT] + [p for p in saved if not os.path.isfile(os.path.join(p or os.getcwd(), "src", "__init__.py"))]
    try:
        import importlib
        return importlib.import_module("src.pretrained.gpen.align_faces")
    finally:
        sys.path[:] = saved


def landmark_sets(ref5):
    """Four faces in a 256 x 320 (h x w) frame, as similarity images of the reference points plus a seeded jitter."""
    import numpy as np
    rng = np.random.RandomState(7)
    out = {}
    for name, (scale, deg, cx, cy) in {"frontal": (0.30, 0.0, 150.0, 120.0), "rotated30": (0.28, 30.0, 170.0, 130.0),
                                       "small": (0.08, -8.0, 60.0, 200.0), "outside": (0.35, 12.0, 300.0, 40.0)}.items():
        c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
        R = np.array([[c, -s], [s, c]])
        out[name] = (ref5 - 256.0) @ R.T * scale + np.array([cx, cy]) + rng.uniform(-1.5, 1.5, size=(5, 2)) * scale * 3
    return out


def _z(t):
    return (zlib.compress(t.contiguous().numpy().tobytes(), 9), tuple(t.shape))


def main():
    from e4s_amd import synth
    ParseNet = reference_parsenet()
    out = {"nets": NETS, "cases": CASES, "margin_unit": MARGIN_UNIT}
    lut = torch.tensor(MASK_COLORMAP, dtype=torch.uint8)
    with torch.no_grad():
        for i, (ni, b, seed) in enumerate(CASES):
            size, osize, mfs, depth = NETS[ni]
            mk = lambda: ParseNet(size, osize, mfs, 64, 19, res_depth=depth, norm_type="bn", relu_type="LeakyReLU", ch_range=[32, 256]).eval()
            torch.manual_seed(0)
            net = mk()
            sd = synth.synth_parsenet_state_dict(net)
            net.load_state_dict(sd, strict=True)
            net64 = mk()
            net64.load_state_dict(sd, strict=True)
            net64.double()
            out[f"keys.{i}"], out[f"shapes.{i}"] = list(sd.keys()), [tuple(v.shape) for v in sd.values()]
            if size == 512:
                out["keys"], out["shapes"] = out[f"keys.{i}"], out[f"shapes.{i}"]
            u8 = synth.synth_sr_input_u8(b, size, size, seed)
            x = (u8.permute(0, 3, 1, 2).double() / 255.0 * 2 - 1).float()
            mid, hooks = {}, []
            if size == 512:
                hooks = [net64.encoder[1].register_forward_hook(lambda m, a, o: mid.__setitem__("enc0", o)),
                         net64.encoder.register_forward_hook(lambda m, a, o: mid.__setitem__("feat", o)),
                         net64.body.register_forward_hook(lambda m, a, o: mid.__setitem__("body", o)),
                         net64.decoder[0].register_forward_hook(lambda m, a, o: mid.__setitem__("dec0", o))]
            y64 = net64(x.double())[0]
            for hk in hooks:
                hk.remove()
            y32 = net(x)[0].double()
            r, c = torch.tensor(sample(size)), torch.tensor(sample(size))
            rec64, rec32 = y64[:, :, r][:, :, :, c], y32[:, :, r][:, :, :, c]
            scale = float(y64.abs().max())
            out[f"rows.{i}"], out[f"cols.{i}"] = r.tolist(), c.tolist()
            out[f"logits.{i}"] = rec64.float().contiguous()
            out[f"scale.{i}"] = scale
            out[f"e32.{i}"] = float((rec32 - rec64).abs().max())
            mask = lut[y64.argmax(1)]
            zero = torch.tensor([k for k, v in enumerate(MASK_COLORMAP) if v == 0])
            rest = torch.tensor([k for k, v in enumerate(MASK_COLORMAP) if v != 0])
            margin = (y64[:, zero].amax(1) - y64[:, rest].amax(1)).abs()
            out[f"mask.{i}"] = _z(mask)
            out[f"margin.{i}"] = _z(torch.floor(margin / (MARGIN_UNIT * scale)).clamp(max=255).to(torch.uint8))
            close = float((margin <= 2 * 1e-3 * scale).double().mean())
            white = float((mask == 255).double().mean())
            print(f"case {i} net {NETS[ni]} B {b}: scale {scale:.3f}, e32 / scale {out[f'e32.{i}'] / scale:.2e}, mask 255 on {white:.3f}, "
                  f"margin <= 2e-3 x scale on {close:.4f}")
            if size == 512:
                assert close <= 0.01, close
                assert 0.05 <= white <= 0.95, white
                mid["trunk"] = mid["feat"] + mid["body"]
                for name in ("enc0", "trunk", "dec0"):
                    n = mid[name].shape[-1]
                    rc = sorted({0, 1, 15, 16, 17, n - 2, n - 1})
                    t = torch.tensor(rc)
                    out[f"mid_rc.{name}"] = rc
                    out[f"mid.{name}"] = mid[name][:, :, t][:, :, :, t].float().contiguous()
                    out[f"mid.{name}.scale"] = float(mid[name].abs().max())
    import numpy as np
    af = reference_align()
    ref5 = np.asarray(af.get_reference_facial_points((512, 512), 0.25, (0, 0), True), dtype=np.float64)
    out["ref5"] = torch.from_numpy(ref5.copy())
    for name, pts in landmark_sets(ref5).items():
        params, scale = af._umeyama(pts, ref5)
        inv, _ = af._umeyama(ref5, pts, False, scale=1.0 / scale)
        out[f"lm.{name}"] = {"pts": torch.from_numpy(pts.copy()), "tfm": torch.from_numpy(params[:2, :].copy()),
                             "tfm_inv": torch.from_numpy(inv[:2, :].copy())}
        print(f"landmarks {name}: scale {scale:.4f}")
    path = os.path.join(HERE, "parsenet.pt")
    torch.save(out, path)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"wrote {path} ({size / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
