"""Seeded cases of the gather-GEMM conv tile (csrc/gather_gemm.h; e4s_rconv_f32 of csrc/retinaface.hip and e4s_conv3dx_f32 of
csrc/vid2vid.hip) for the bits test: tests/test_gather_conv_cases_host.py and tests/test_gpu_gather_conv_bits.py.  Building a case is
CPU only; the native library is imported by run() alone.

Every case is the smallest shape that reaches a path of its own and runs in both precisions.  The fixture
tests/golden/gather_conv_bits.json holds, per case, the sha256 of every input tensor, of the packed weight image and of the WHOLE
output buffer (pre-filled with SENTINEL, so a store outside the conv's channels changes the hash too).  It is written by

    python tests/gather_conv_cases.py --record tests/golden/gather_conv_bits.json

on an MI355X, from these same cases."""
import hashlib
import json
import os
import sys

import torch

SENTINEL = 12345.0
PRECISIONS = ("f32", "bf16x3")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gather_conv_bits.json")


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def _w(cout, cin, *k, seed):
    fan = cin
    for e in k:
        fan *= e
    return _rand(cout, cin, *k, seed=seed) / fan ** 0.5


def _depth_of_nhwc(t):
    """[B,h,w,depth * 64] -> the volume [B,depth,h,w,64] it holds, as a view (the 1x1 conv in front of the keypoint detector's decoder)"""
    b, h, w, dc = t.shape
    return t.view(b, h, w, dc // 64, 64).permute(0, 3, 1, 2, 4)


# name -> (kind, inputs, options).  2-D options are K.rconv's keywords plus the output buffer's width; 3-D options are K.conv3dx's plus
# the output buffer's shape and the views x and res are read through.
def _cases():
    c = {}
    c["2d_k3_s2_ragged_last_tile_bn64"] = ("2d", dict(x=_rand(3, 19, 28, 64, seed=1), w=_w(64, 64, 3, 3, seed=2)),
                                           dict(k=3, stride=2))
    c["2d_k1_sub_tile_bn128"] = ("2d", dict(x=_rand(2, 5, 7, 64, seed=3), w=_w(128, 64, 1, 1, seed=4), bias=_rand(128, seed=5)),
                                 dict(k=1, act=True))
    c["2d_k3_lrelu_nearest_r0_at_y_coff"] = ("2d", dict(x=_rand(2, 5, 7, 256, seed=6), w=_w(128, 256, 3, 3, seed=7), bias=_rand(128, seed=8),
                                                      r0=_rand(2, 3, 4, 128, seed=9)),
                                             dict(k=3, act=True, slope=0.1, r0_after=True, y_width=264, y_coff=128))
    c["2d_k3_r0_before_act_one_tile"] = ("2d", dict(x=_rand(1, 8, 16, 64, seed=10), w=_w(64, 64, 3, 3, seed=11), r0=_rand(1, 8, 16, 64, seed=12)),
                                         dict(k=3, act=True))
    c["3d_k3_cout15_guarded_stores_bn32"] = ("3d", dict(x=_rand(2, 3, 9, 7, 32, seed=13), w=_w(15, 32, 3, 3, 3, seed=14), bias=_rand(15, seed=15)),
                                             dict(relu=True, y_shape=(2, 3, 9, 7, 16)))
    c["3d_k3_up2_strided_view"] = ("3d", dict(x=_rand(2, 3, 5, 4 * 64, seed=16), w=_w(32, 64, 3, 3, 3, seed=17)),
                                   dict(up2=True, y_shape=(2, 4, 6, 10, 32), x_view=_depth_of_nhwc))
    c["3d_k1_strided_res_channel_slice"] = ("3d", dict(x=_rand(2, 2, 3, 5, 64, seed=18), w=_w(64, 64, 1, 1, 1, seed=19),
                                                       res=_rand(2, 2, 3, 5, 80, seed=20)),
                                            dict(y_shape=(2, 2, 3, 5, 96), y_coff=32, res_view=lambda t: t[..., 8:72]))
    c["3d_k3_broadcast_batch_bn128"] = ("3d", dict(x=_rand(1, 2, 5, 6, 128, seed=21), w=_w(128, 128, 3, 3, 3, seed=22)),
                                        dict(y_shape=(2, 2, 5, 6, 128)))
    c["3d_k7_two_planes_per_tile_skips_kd"] = ("3d", dict(x=_rand(2, 4, 8, 8, 32, seed=23), w=_w(16, 32, 7, 7, 7, seed=24)),
                                               dict(y_shape=(2, 4, 8, 8, 16)))
    c["3d_k7_tile_spans_samples"] = ("3d", dict(x=_rand(3, 2, 4, 4, 32, seed=25), w=_w(16, 32, 7, 7, 7, seed=26)),
                                     dict(y_shape=(3, 2, 4, 4, 16)))
    return c


_CACHE = {}


def cases():
    """name -> (kind, inputs, options), built once; nobody writes to the tensors"""
    if not _CACHE:
        _CACHE.update(_cases())
    return _CACHE


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def input_hashes(name):
    return {k: sha(v) for k, v in cases()[name][1].items()}


def skipped_kd_planes(d, h, w, m0, m_total, ks=7, bm=128):
    """The kd planes that the tile of output voxels m0 .. m0 + bm - 1 leaves out (the plane skip of the k = 7 conv, restated for the
    host test that the two k = 7 cases are what their names say)"""
    per, pad = h * w, ks // 2
    v0, v1 = m0 // per, min(m0 + bm - 1, m_total - 1) // per
    one = v0 // d == v1 // d
    dlo, dhi = (v0 % d, v1 % d) if one else (0, d - 1)
    lo, hi = max(pad - dhi, 0), min(d - 1 + pad - dlo, ks - 1)
    return [kd for kd in range(ks) if kd < lo or kd > hi]


def run(name, precision, dev="cuda"):
    """One case on the device -> (the packed weight image, the whole output buffer)"""
    from e4s_amd import kernels as K
    kind, inp, opt = cases()[name]
    f32 = precision == "f32"
    t = {k: v.to(dev) for k, v in inp.items()}
    opt = dict(opt)
    cout, cin = inp["w"].shape[:2]
    if kind == "2d":
        k, stride = opt.pop("k"), opt.get("stride", 1)
        b, h, w, _ = inp["x"].shape
        y = torch.full((b, K.rconv_out_size(h, k, stride), K.rconv_out_size(w, k, stride), opt.pop("y_width", cout)), SENTINEL, device=dev)
        pack = K.rconv_pack(t["w"], f32)
        K.rconv(t["x"], cin, pack, cout, k, y, bias=t.get("bias"), r0=t.get("r0"), f32=f32, **opt)
    else:
        y = torch.full(opt.pop("y_shape"), SENTINEL, device=dev)
        x = opt.pop("x_view", lambda v: v)(t["x"])
        res = opt.pop("res_view")(t["res"]) if "res" in t else None
        pack = K.conv3dx_pack(t["w"], f32)
        K.conv3dx(x, pack, cout, y, bias=t.get("bias"), res=res, f32=f32, **opt)
    torch.cuda.synchronize()
    return pack, y


def record(path):
    out = {}
    for name in cases():
        out[name] = dict(inputs=input_hashes(name))
        for precision in PRECISIONS:
            pack, y = run(name, precision)
            out[name][precision] = dict(pack=sha(pack), out=sha(y))
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(out)} cases x {len(PRECISIONS)} precisions to {path}")


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: gather_conv_cases.py --record <fixture.json>")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record(sys.argv[2])
