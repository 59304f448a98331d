"""Fixture of the Real-ESRNet x4 super-resolution (e4s_amd/sr.py): the REFERENCE's own RRDBNet run on CPU.

Imports src/pretrained/gpen/sr_model/rrdbnet_arch.py where it lies (it needs nothing but torch; the absent third-party packages
of the packages above it are stubbed by oracle/ref_shim.stub_third_party).  Weights: synth.synth_rrdb_state_dict(net), the same
seeded tensors the tests load into e4s_amd.sr.RRDBNet (dense-block weights x 0.1, conv_last rescaled so that the clamp to [0, 1]
leaves most outputs alone; the script asserts that at least half of every recorded output lies inside (0.02, 0.98)).

Recorded (inputs as seeds, never as tensors; an input is synth.synth_sr_input_u8(b, h, w, seed) / 255 as fp32 NCHW):
    keys / shapes      the reference RRDBNet's state_dict
    cases              [(b, h, w, seed)]: 1x5x7, 2x40x48, 1x256x256
    y.<i>              the fp64 forward before the clamp, stored as fp32 (the storage rounding, 2^-24 relative, is 3 orders below
                       the tightest bound that reads it): all of it for the two small inputs; for 256^2 the rows / columns
                       `sample_out` (edges plus a stride) of the 1024^2 output
    scale.<i>          max |y64| over the whole output
    e32.<i>            max |fp32 forward - fp64 forward| of the reference itself on the recorded positions
    inside.<i>         share of the recorded outputs inside (0.02, 0.98)
    mid.rdb1 / mid.rrdb / mid.trunk   for 2x40x48: the fp64 outputs (stored as fp32, NCHW) of body[0].rdb1, of body[0] and of the
                       trunk feat + conv_body(body(feat)) at the rows `mid_rows` and columns `mid_cols`, with their max |.| in
                       mid.*.scale, so that a failure of the whole net can be located

Run in the build container:  python tests/golden/make_sr_golden.py   (writes tests/golden/sr.pt)"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

CASES = [(1, 5, 7, 21), (2, 40, 48, 22), (1, 256, 256, 23)]
SAMPLE_OUT = sorted(set(range(0, 4)) | set(range(1020, 1024)) | set(range(0, 1024, 37)))
MID_ROWS = sorted(set(range(0, 40, 5)) | {1, 15, 16, 17, 39})
MID_COLS = sorted(set(range(0, 48, 5)) | {1, 15, 16, 17, 31, 32, 47})


def reference_rrdbnet():
    """The reference's RRDBNet class, imported offline on CPU."""
    from oracle import ref_shim
    ref_shim.stub_third_party()
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [ref_shim.REF_ROOT] + [p for p in saved if not os.path.isfile(os.path.join(p or os.getcwd(), "src", "__init__.py"))]
    try:
        import importlib
        arch = importlib.import_module("src.pretrained.gpen.sr_model.rrdbnet_arch")
    finally:
        sys.path[:] = saved
    return arch.RRDBNet


def main():
    from e4s_amd import synth
    RRDBNet = reference_rrdbnet()
    torch.manual_seed(0)
    net = RRDBNet(3, 3, num_feat=32, num_block=23, num_grow_ch=32, scale=4).eval()
    sd = synth.synth_rrdb_state_dict(net)
    net.load_state_dict(sd, strict=True)
    net64 = RRDBNet(3, 3, num_feat=32, num_block=23, num_grow_ch=32, scale=4).eval()
    net64.load_state_dict(sd, strict=True)
    net64.double()
    out = {"keys": list(sd.keys()), "shapes": [tuple(v.shape) for v in sd.values()], "cases": CASES, "sample_out": SAMPLE_OUT,
           "mid_rows": MID_ROWS, "mid_cols": MID_COLS}
    with torch.no_grad():
        for i, (b, h, w, seed) in enumerate(CASES):
            x = synth.synth_sr_input_u8(b, h, w, seed).permute(0, 3, 1, 2).float().div(255)
            mid = {}
            hooks = []
            if (b, h, w) == (2, 40, 48):
                hooks = [net64.body[0].rdb1.register_forward_hook(lambda m, a, o: mid.__setitem__("rdb1", o)),
                         net64.body[0].register_forward_hook(lambda m, a, o: mid.__setitem__("rrdb", o)),
                         net64.conv_first.register_forward_hook(lambda m, a, o: mid.__setitem__("feat", o)),
                         net64.conv_body.register_forward_hook(lambda m, a, o: mid.__setitem__("body", o))]
            y64 = net64(x.double())
            for hk in hooks:
                hk.remove()
            y32 = net(x).double()
            if h * w > 64 * 64:
                s = torch.tensor(SAMPLE_OUT)
                rec64, rec32 = y64[:, :, s][:, :, :, s], y32[:, :, s][:, :, :, s]
            else:
                rec64, rec32 = y64, y32
            inside = float(((rec64 > 0.02) & (rec64 < 0.98)).double().mean())
            assert inside >= 0.5, (i, inside)
            out[f"y.{i}"] = rec64.float().contiguous()
            out[f"scale.{i}"] = float(y64.abs().max())
            out[f"e32.{i}"] = float((rec32 - rec64).abs().max())
            out[f"inside.{i}"] = inside
            print(f"case {i} {b}x{h}x{w}: range {float(y64.min()):.3f} .. {float(y64.max()):.3f}, inside {inside:.3f}, "
                  f"e32 / scale {out[f'e32.{i}'] / out[f'scale.{i}']:.2e}")
            if mid:
                r, c = torch.tensor(MID_ROWS), torch.tensor(MID_COLS)
                mid["trunk"] = mid["feat"] + mid["body"]
                for name in ("rdb1", "rrdb", "trunk"):
                    out[f"mid.{name}"] = mid[name][:, :, r][:, :, :, c].float().contiguous()
                    out[f"mid.{name}.scale"] = float(mid[name].abs().max())
    path = os.path.join(HERE, "sr.pt")
    torch.save(out, path)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"wrote {path} ({size / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
