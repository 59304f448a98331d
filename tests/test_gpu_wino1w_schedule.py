"""conv_wino1w_kernel (csrc/conv_wino1w.hip): the re-planned slot table of its K loop moves instructions between MFMA gaps and changes no
arithmetic and no order of addition.  Two checks per seeded case, on the smallest shapes the one-wave-per-SIMD kernel takes (E4S_WINO_1W=1,
no K split):
  (a) against F.conv2d in fp64 with the bounds of test_winograd_f23_conv_vs_fp64 (3e-5 of the output scale; statistics 3e-5 of the
      scale for the mean, 1e-4 relative for 1 / sqrt(var + eps)),
  (b) bit-identical to the commit before the re-plan: SHA-256 of every output tensor's bytes == tests/golden/wino1w_parent_digests.json
      (tools/parent_digests.py wrote it from that commit's library: tools/build_prev_lib.sh + E4S_LIB_PATH).
Cases: both forms (InstanceNorm folded into the input transform + PReLU; output statistics); 320 tiles on 256 CUs (a block walks two tiles
across a sample boundary, the statistics table switches parity); 16-wide maps of four tile rows (a tile is the left AND the right edge; top,
inner and bottom rows); Cin = 128 = eight chunks, the fewest the policy sends to this kernel."""
import ctypes
import functools
import hashlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino1w_parent_digests.json")

# (batch, H, W, Cin, Cout): 160 tiles (one per CU) x 16 chunks; 320 tiles x 8 chunks; 144 tiles x 8 chunks, every tile on two or three edges.
# (8, 64, 16, 128 -> 512) would be 128 tiles, which the policy splits along K: nine samples keep it whole
SHAPES = [(5, 64, 64, 256, 256), (5, 128, 128, 128, 128), (9, 64, 16, 128, 512)]
MODES = ["in_prelu", "stats"]
GOLDEN_ENV = {"E4S_WINO_1W": "1"}          # tools/parent_digests.py: the environment of the cases


def case_id(shape, mode):
    return "x".join(str(s) for s in shape) + "_" + mode


def golden_cases():
    return {case_id(shape, mode): (shape, mode) for shape in SHAPES for mode in MODES}


@functools.lru_cache(maxsize=None)
def operands(shape):
    b, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(1000 + h * 7 + w * 3 + cin + cout)
    x = torch.randn(b, cin, h, w, generator=g) * 1.3 + 0.4
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    slope = torch.rand(cout, generator=g) * 0.5
    return x, wt, slope


@functools.lru_cache(maxsize=None)
def reference(shape, mode):
    """fp64 on the CPU, once per case."""
    x, wt, slope = operands(shape)
    x64, w64 = x.double(), wt.double()
    if mode == "in_prelu":
        xn = (x64 - x64.mean((2, 3), keepdim=True)) / torch.sqrt(x64.var((2, 3), unbiased=False, keepdim=True) + 1e-5)
        ref = F.conv2d(xn, w64, padding=1)
        return torch.where(ref > 0, ref, ref * slope.double().view(1, -1, 1, 1))
    return F.conv2d(x64, w64, padding=1)


def run_case(shape, mode):
    """The launch under test -> {name: tensor} of everything it wrote.  The caller has set E4S_WINO_1W=1."""
    from e4s_amd import kernels as K
    from e4s_amd import lib
    b, h, w, cin, cout = shape
    x, wt, slope = operands(shape)
    xd = K.nchw_to_nhwc(x.to(DEV))
    u = K.wino_weights(K.pack_taps(wt.to(DEV)))
    p = lib.ConvParams()
    p.B, p.Ha, p.Wa, p.Hi, p.Wi, p.Ho, p.Wo, p.Cin, p.Cout = b, h, w, h, w, h, w, cin, cout
    p.istride, p.ostride, p.ntaps, p.ncls, p.groups_per_batch = 1, 1, 9, 1, 1
    assert lib.load().e4s_conv_wino_covers(ctypes.byref(p)) == 1
    assert lib.load().e4s_conv_wino_ws_floats(ctypes.byref(p)) == 0          # no K split: the launch goes to conv_wino1w_kernel
    if mode == "in_prelu":
        st, _ = K.instnorm_stats(xd)
        return {"y": K.conv_wino(xd, u, cout, in_stats=st, act=2, slope=slope.to(DEV))}
    y, (stats, pooled) = K.conv_wino(xd, u, cout, want_stats=True)
    return {"y": y, "stats": stats, "pooled": pooled}


def digests(out):
    torch.cuda.synchronize()
    return {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, v in sorted(out.items())}


def maxabs(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_wino1w_matches_fp64_and_the_parent_bit_for_bit(shape, mode, monkeypatch):
    from e4s_amd import kernels as K
    monkeypatch.setenv("E4S_WINO_1W", "1")
    out = run_case(shape, mode)
    ref = reference(shape, mode)
    scale = float(ref.abs().max())
    err = maxabs(K.nhwc_to_nchw(out["y"]), ref) / scale
    print("%s: max |y - fp64| = %.3e of the output scale" % (case_id(shape, mode), err))
    got = digests(out)
    with open(GOLDEN) as fh:
        want = json.load(fh)["cases"][case_id(shape, mode)]
    print("digests", got, "parent", want)
    assert err < 3e-5, err
    if mode == "stats":
        mean, var = ref.mean((2, 3)), ref.var((2, 3), unbiased=False)
        rstd = 1 / torch.sqrt(var + 1e-5)
        e_mean, e_rstd = maxabs(out["stats"][..., 0], mean) / scale, maxabs(out["stats"][..., 1], rstd) / float(rstd.max())
        print("statistics: mean %.3e of the scale, rstd %.3e relative" % (e_mean, e_rstd))
        assert e_mean < 3e-5 and e_rstd < 1e-4
    assert got == want
