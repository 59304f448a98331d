"""GPU parity tests: the HIP path (through the C-ABI of libe4s_hip.so) against the CPU oracle and the
golden fixtures produced by the real reference.  Tolerance: BASELINE.json north_star states 1e-3
max-abs on the 1024^2 outputs.  With E4S_PRECISION=f32 (pinned by a fixture for every test that does not ask
otherwise) the kernels compute in exact fp32 (v_mfma_f32_32x32x2_f32), so the op/layer tests use much tighter
bounds (written next to each assert); the split-bf16 kernels (E4S_PRECISION=bf16x3/auto) have their own tests
against 1e-4 of the output scale per layer and the 1e-3 bound end to end."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from e4s_amd import synth
from oracle import e4s_oracle as orc
from region_cases import region_case as _region_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def maxabs(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


@pytest.fixture(autouse=True)
def _exact_fp32_unless_a_test_asks_otherwise(monkeypatch):
    """The tight (<= 1e-4) bounds in this file are statements about the exact-fp32 kernels; the split-bf16 encoder
    path (E4S_PRECISION=auto/bf16x3, the runtime default at batch >= 8) has its own tests against the 1e-3 bound."""
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", "f32")


# ---------------------------------------------------------------------------------------------
# operators (1:1 with the reference's native ops)
# ---------------------------------------------------------------------------------------------
def test_ops_golden(golden):
    from e4s_amd.op import fused_leaky_relu, upfirdn2d
    g = golden("ops.pt")
    for case in g["kat"] + g["rand"]:
        if case["op"] == "upfirdn2d":
            y = upfirdn2d(case["x"].to(DEV), case["k"].to(DEV), up=case["up"], down=case["down"], pad=case["pad"])
        else:
            y = fused_leaky_relu(case["x"].to(DEV), case["b"].to(DEV))
        assert y.shape == case["y"].shape
        assert maxabs(y, case["y"]) < 2e-6, case["op"]


def test_fused_bias_act_all_modes():
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(0)
    for shape in [(2, 5, 7, 3), (3, 8, 16, 16), (4, 6), (1, 32, 64, 64)]:
        x = torch.randn(*shape, generator=g)
        b = torch.randn(shape[1], generator=g)
        ref = torch.randn(*shape, generator=g)
        for act, grad in [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2)]:
            want = orc.fused_bias_act(x, b, ref, act, grad, 0.2, 1.5)
            got = K.fused_bias_act(x.to(DEV), b.to(DEV), ref.to(DEV), act, grad, 0.2, 1.5)
            assert maxabs(got, want) < 1e-6, (shape, act, grad)
        want = orc.fused_bias_act(x, None, ref, 3, 1, 0.2, 2 ** 0.5)
        got = K.fused_bias_act(x.to(DEV), None, ref.to(DEV), 3, 1, 0.2, 2 ** 0.5)
        assert maxabs(got, want) < 1e-6


def test_ops_backward_matches_oracle_autograd():
    from e4s_amd.op import fused_leaky_relu, upfirdn2d
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 6, 9, 11, generator=g)
    b = torch.randn(6, generator=g)
    k = orc.make_blur_kernel() * 4
    for fn_dev, fn_ref in [
        (lambda t, bb: fused_leaky_relu(t, bb), lambda t, bb: orc.fused_leaky_relu(t, bb)),
        (lambda t, bb: upfirdn2d(t, k.to(DEV), up=2, pad=(2, 1)) * bb.view(1, -1, 1, 1),
         lambda t, bb: orc.upfirdn2d(t, k, up=2, pad=(2, 1)) * bb.view(1, -1, 1, 1)),
        (lambda t, bb: upfirdn2d(t, k.to(DEV), down=2, pad=(1, 1)) * bb.view(1, -1, 1, 1),
         lambda t, bb: orc.upfirdn2d(t, k, down=2, pad=(1, 1)) * bb.view(1, -1, 1, 1)),
    ]:
        xd, bd = x.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        xr, br = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
        yd, yr = fn_dev(xd, bd), fn_ref(xr, br)
        w = torch.randn(yr.shape, generator=g)
        (yd * w.to(DEV)).sum().backward()
        (yr * w).sum().backward()
        assert maxabs(yd, yr) < 1e-5
        assert maxabs(xd.grad, xr.grad) < 1e-5
        assert maxabs(bd.grad, br.grad) < 1e-4


def test_upfirdn2d_large_matches_oracle():
    from e4s_amd.op import upfirdn2d
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 4, 257, 257, generator=g)
    k = orc.make_blur_kernel() * 4
    assert maxabs(upfirdn2d(x.to(DEV), k.to(DEV), pad=(1, 1)), orc.upfirdn2d(x, k, pad=(1, 1))) < 1e-5
    x = torch.randn(2, 3, 128, 128, generator=g)
    assert maxabs(upfirdn2d(x.to(DEV), k.to(DEV), up=2, pad=(2, 1)), orc.upfirdn2d(x, k, up=2, pad=(2, 1))) < 1e-5


@pytest.mark.parametrize("b,c,h,w,pad,asym", [(2, 32, 40, 56, (2, 2), False), (1, 64, 33, 17, (2, 1), False), (3, 8, 16, 16, (1, 1), False),
                                               (1, 544, 8, 8, (1, 2), True), (2, 128, 64, 64, (-1, 0), True)])
def test_fir_on_channels_last_activations_vs_oracle(b, c, h, w, pad, asym):
    """The Blur of the ConvLayers (model.py:683-689: up = down = 1) on NHWC activations: e4s_upfirdn2d_f32's coalesced
    channels-last path (4 channels per lane) == the reference's fallback upfirdn2d on the NCHW tensor; the 4x4 blur and an
    ASYMMETRIC kernel (flip convention, KAT4), negative pads (crop), the 544-channel padded map, odd sizes."""
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(21)
    x = torch.randn(b, c, h, w, generator=g)
    k = torch.randn(4, 4, generator=g) if asym else orc.make_blur_kernel()
    want = orc.upfirdn2d(x, k, pad=pad)
    got = K.nhwc_to_nchw(K.upfirdn2d_nhwc(K.nchw_to_nhwc(x.to(DEV)), k.to(DEV), pad=pad))
    assert got.shape == want.shape
    assert maxabs(got, want) < 1e-5 * max(1.0, float(want.abs().max()))


# ---------------------------------------------------------------------------------------------
# the MFMA conv kernel against plain fp32 convolution
# ---------------------------------------------------------------------------------------------
def _pack(w):
    cout, cin, kh, kw = w.shape
    return w.permute(2, 3, 0, 1).reshape(1, kh * kw, cout, cin).contiguous()


def test_plain_c_host_reproduces_kats_through_the_abi(tmp_path):
    """examples/c_abi_demo.c (C99, no Python, no torch) built with gcc against libe4s_hip.so runs SURVEY.md 8(c)'s KAT5
    and KAT2 on the GPU and checks them itself."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "c_abi_demo"
    libdir = os.path.join(root, "e4s_amd")
    build = subprocess.run(["gcc", "-std=c99", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "c_abi_demo.c"),
                            "-L" + libdir, "-le4s_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
                            "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    assert "KAT5 and KAT2 reproduced" in run.stdout


@pytest.mark.parametrize("b,h,w,cin,cout,stride,spatial", [
    (2, 16, 16, 64, 128, 1, True), (2, 16, 16, 64, 128, 1, False), (1, 32, 32, 32, 64, 1, True),
    (1, 32, 32, 64, 32, 1, True), (1, 32, 32, 64, 32, 1, False), (2, 32, 32, 64, 64, 2, False),
    (1, 16, 32, 96, 160, 1, True), (1, 64, 64, 128, 256, 2, False),
    (2, 12, 20, 64, 64, 1, True), (3, 4, 4, 64, 128, 1, True), (1, 8, 8, 32, 32, 1, True),   # partial halo tiles
])
def test_conv_mfma_vs_conv2d(b, h, w, cin, cout, stride, spatial):
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(3)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    want = F.conv2d(x, wt, stride=stride, padding=1)
    y = K.conv_mfma(K.nchw_to_nhwc(x.to(DEV)), _pack(wt).to(DEV), cout, istride=stride, spatial=spatial)
    assert maxabs(K.nhwc_to_nchw(y), want) < 2e-5


def test_conv_mfma_1x1_stride2_and_prelu():
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 64, 32, 32, generator=g)
    wt = torch.randn(128, 64, 1, 1, generator=g) / 8
    y = K.conv_mfma(K.nchw_to_nhwc(x.to(DEV)), _pack(wt).to(DEV), 128, istride=2, ntaps=1)
    assert maxabs(K.nhwc_to_nchw(y), F.conv2d(x, wt, stride=2)) < 2e-5
    w3 = torch.randn(64, 64, 3, 3, generator=g) / 24
    slope = torch.rand(64, generator=g)
    y = K.conv_mfma(K.nchw_to_nhwc(x.to(DEV)), _pack(w3).to(DEV), 64, act=2, slope=slope.to(DEV))
    assert maxabs(K.nhwc_to_nchw(y), F.prelu(F.conv2d(x, w3, padding=1), slope)) < 2e-5


@pytest.mark.parametrize("b,h,w,cin,cout,full", [
    (2, 32, 32, 64, 128, False), (1, 16, 16, 512, 512, True), (2, 8, 8, 128, 256, False),     # 8x8: partial 16x16 tile
    (1, 20, 40, 96, 128, True), (3, 4, 4, 32, 128, False),                                    # ragged tiles
    (2, 32, 32, 64, 64, True), (1, 24, 40, 32, 32, True), (2, 16, 16, 128, 64, False), (1, 12, 20, 64, 32, False),
    (1, 8, 16, 96, 96, True),                                      # 64- / 32-wide column tiles, 128-pixel tiles
])
def test_conv_bf16x3_vs_conv2d_f64(b, h, w, cin, cout, full):
    """Split-bf16 contraction (3 bf16 MFMAs per product, fp32 accumulate) against an fp64 convolution.  Error model:
    <= ~2^-16 per product, random sign -> ~1e-5 of the output scale; bound 1e-4 of max|y| (the exact fp32-MFMA kernel
    measures ~1e-6 on the same inputs).  `full` adds the whole epilogue: per-sample style on the input, demodulation,
    noise, bias and leaky-ReLU."""
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(31)
    x = torch.randn(b, cin, h, w, generator=g, dtype=torch.float64) * 1.3 + 0.2
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / math.sqrt(cin * 9)
    wp = _pack(wt.float()).to(DEV)
    ws = K.split_bf16x2(wp)
    xd = K.nchw_to_nhwc(x.float().to(DEV))
    if not full:
        want = F.conv2d(x.float().double(), wt.float().double(), padding=1)
        y = K.conv_mfma(xd, wp, cout, w_split=ws)
    else:
        s = torch.rand(b, cin, generator=g) + 0.5
        d = torch.rand(b, cout, generator=g) + 0.5
        nz = torch.randn(b, 1, h, w, generator=g)
        nw = torch.tensor([0.3])
        bias = torch.randn(cout, generator=g) * 0.1
        pre = F.conv2d(x.float().double() * s.double()[:, :, None, None], wt.float().double(), padding=1)
        pre = pre * d.double()[:, :, None, None] + 0.3 * nz.double() + bias.double()[None, :, None, None]
        want = F.leaky_relu(pre, 0.2) * math.sqrt(2.0)
        y = K.conv_mfma(xd, wp, cout, w_split=ws, in_scale=s.to(DEV), out_scale=d.to(DEV), noise=nz.to(DEV),
                        noise_w=nw.to(DEV), bias=bias.to(DEV), act=1)
    err = maxabs(K.nhwc_to_nchw(y), want)
    assert err < 1e-4 * float(want.abs().max()), (err, float(want.abs().max()))


@pytest.mark.parametrize("b,h,w,cin,cout,ntaps", [(2, 32, 32, 128, 128, 9), (1, 16, 48, 256, 256, 9), (3, 8, 8, 64, 128, 1),
                                                   (1, 20, 12, 128, 256, 1), (2, 6, 10, 512, 512, 9), (2, 64, 64, 64, 64, 9), (1, 18, 26, 64, 64, 9),
                                                   (3, 10, 14, 32, 64, 1)])
def test_conv_bf16x3_gather_stride2_vs_conv2d_f64(b, h, w, cin, cout, ntaps):
    """The encoder's stride-2 3x3 convs and 1x1 stride-2 shortcut convs on the per-tap gather split-bf16 kernel (ragged
    pixel counts: tiles straddle rows and samples) against an fp64 convolution, 1e-4 of the output scale.  Cout = 64 (the first
    stride-2 unit, helpers.py:125-137 with depth 64): one half-used 128-column tile whose upper waves issue no MFMAs and store nothing."""
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(35)
    k = 3 if ntaps == 9 else 1
    x = torch.randn(b, cin, h, w, generator=g, dtype=torch.float64) * 1.1 - 0.1
    wt = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / math.sqrt(cin * k * k)
    wp = _pack(wt.float()).to(DEV)
    xd = K.nchw_to_nhwc(x.float().to(DEV))
    want = F.conv2d(x.float().double(), wt.float().double(), stride=2, padding=k // 2)
    y = K.conv_mfma(xd, wp, cout, istride=2, ntaps=ntaps, w_split=K.split_bf16x2(wp))
    y32 = K.conv_mfma(xd, wp, cout, istride=2, ntaps=ntaps)
    assert tuple(y.shape) == (b, h // 2, w // 2, cout)
    assert 0.0 < maxabs(y, y32)
    err = maxabs(K.nhwc_to_nchw(y), want)
    assert err < 1e-4 * float(want.abs().max()), (err, float(want.abs().max()))


@pytest.mark.parametrize("b,h,w,cin,cout,kind", [(2, 32, 32, 512, 512, "in"), (1, 16, 16, 256, 128, "style"), (1, 16, 32, 128, 64, "plain"),
                                                 (1, 8, 8, 256, 64, "up")])
def test_conv_bf16x3_split_k_vs_unsplit_path(b, h, w, cin, cout, kind):
    """Few-tile launches (batch-1 latency runs) split the input channels over blocks and add the slabs in a second kernel:
    against the fp64 convolution, with every epilogue flavour (fused InstanceNorm + PReLU, style/demod/noise/bias/lrelu,
    none, pixel-shuffled up-conv), and bit-reproducible."""
    from e4s_amd import kernels as K, lib
    g = torch.Generator().manual_seed(37)
    x = (torch.randn(b, h, w, cin, generator=g) * 1.2 + 0.1).to(DEV)
    ncls = 4 if kind == "up" else 1
    wt = torch.randn(ncls, 9, cout, cin, generator=g).to(DEV) / math.sqrt(cin * 9)
    ws = K.split_bf16x2(wt)
    ho = h * 2 if kind == "up" else h
    kw = {}
    if kind == "in":
        st, _ = K.instnorm_stats(x)
        kw = dict(in_stats=st, act=2, slope=(torch.rand(cout, generator=g) * 0.5).to(DEV))
    elif kind in ("style", "up"):
        kw = dict(in_scale=(torch.rand(b, cin, generator=g) + 0.5).to(DEV), out_scale=(torch.rand(b, cout, generator=g) + 0.5).to(DEV),
                  noise=torch.randn(b, 1, ho, ho * w // h, generator=g).to(DEV), noise_w=torch.tensor([0.3], device=DEV),
                  bias=(torch.randn(cout, generator=g) * 0.1).to(DEV), act=1)
    if kind == "up":
        kw.update(ncls=4, ostride=2)
    y = K.conv_mfma(x, wt, cout, w_split=ws, **kw)
    y2 = K.conv_mfma(x, wt, cout, w_split=ws, **kw)
    assert torch.equal(y, y2)
    if kind == "in":
        ref = K.conv_mfma(K.instnorm_apply(x, kw["in_stats"]), wt, cout, act=2, slope=kw["slope"])
    else:
        ref = K.conv_mfma(x, wt, cout, **kw)                             # exact fp32 kernel, same epilogue
    assert 0 < maxabs(y, ref) < 1e-4 * float(ref.abs().max())


@pytest.mark.parametrize("res,cin,cout,up", [(32, 512, 512, False), (16, 512, 256, True), (64, 256, 128, False)])
def test_region_kernel_split_k_vs_fp32(res, cin, cout, up, monkeypatch):
    """Masked StyledConv contractions at batch 1 (few tiles): the region-select split-bf16 kernel with the input channels
    split over blocks (slabs carry d[region]; the second stage adds them in order + noise / bias / lrelu) vs the exact fp32
    region-select kernel, and bit-reproducible."""
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", "auto")
    g = torch.Generator().manual_seed(39)
    b, R = 1, 12
    ncls = 4 if up else 1
    x = torch.randn(b, res, res, cin, generator=g).to(DEV)
    wt = torch.randn(ncls, 9, cout, cin, generator=g).to(DEV) / math.sqrt(cin * 9)
    labels = synth.synth_labels_blocks(b, 512, 32, seed=5).to(torch.uint8).view(b, 512, 512).to(DEV)
    ro = res * 2 if up else res
    kw = dict(labels=labels, num_regions=R, ncls=ncls, ostride=2 if up else 1, in_scale=(torch.rand(b * R, cin, generator=g) + 0.5).to(DEV),
              out_scale=(torch.rand(b * R, cout, generator=g) + 0.5).to(DEV), noise=torch.randn(b, 1, ro, ro, generator=g).to(DEV),
              noise_w=torch.tensor([0.2], device=DEV), bias=(torch.randn(cout, generator=g) * 0.1).to(DEV), act=1)
    assert K.want_bf16x3(b, res, res, cin, cout, ncls, masked=True)
    ws = K.split_bf16x2(wt)
    y = K.conv_mfma(x, wt, cout, w_split=ws, **kw)
    assert torch.equal(y, K.conv_mfma(x, wt, cout, w_split=ws, **kw))
    ref = K.conv_mfma(x, wt, cout, **kw)
    assert 0 < maxabs(y, ref) < 1e-4 * float(ref.abs().max())


@pytest.mark.parametrize("b,h,w,cin,cout,up,kind,R", [
    (2, 48, 40, 64, 128, False, "face", 12), (2, 64, 64, 96, 256, False, "blocks", 12), (9, 64, 64, 512, 128, False, "face", 12),
    (2, 32, 32, 64, 128, True, "face", 12), (2, 24, 40, 64, 256, True, "blocks", 12), (1, 33, 17, 64, 128, False, "face", 12),
    (2, 64, 64, 64, 128, False, "noise", 12), (2, 64, 64, 64, 128, False, "half-noise", 12), (2, 32, 48, 64, 128, False, "blocks", 16),
    (3, 128, 128, 128, 128, False, "face", 12),
    # launches of <= 128 tiles: the input channels split over blocks (slabs + second stage), variant rows inside each split
    (1, 32, 32, 512, 512, False, "face", 12), (1, 16, 16, 512, 256, True, "blocks", 12), (2, 64, 64, 256, 128, False, "half-noise", 12),
    # Cout % 256 == 0 and > 128 tiles without a K split: the one-wave-per-SIMD kernel (csrc/conv_region1w.hip; "1w" = asserted below):
    # one and two column tiles, polyphase with partial tiles, 16 regions, a map that overflows the variant rows on one side
    (8, 64, 64, 64, 256, False, "face", 12), (5, 64, 64, 96, 512, False, "blocks", 12), (3, 48, 40, 64, 256, True, "face", 12),
    (11, 32, 48, 64, 256, False, "blocks", 16), (8, 64, 64, 64, 256, False, "half-noise", 12), (5, 33, 49, 32, 256, False, "face", 12)])
def test_region_rows_kernel_vs_fp32_and_region_select(b, h, w, cin, cout, up, kind, R):
    """e4s_conv_region_bf16x3_f32 (variant rows: the halo scaled with each pixel's own region's style once, boundary pairs read extra
    rows) on masked StyledConv contractions, plain and polyphase, ragged maps, 16 regions: == the exact fp32 region kernel to 1e-4
    of the output scale, == the region-select split-bf16 kernel to a few 1e-6 (same products, another summation order), bitwise
    reproducible; per-pixel random regions (every tile overflows the variant rows) fall back to the region-select kernel bit for bit,
    and a map that overflows only on one side mixes both kernels in one launch."""
    from e4s_amd import kernels as K
    x, wt, kw = _region_case(b, h, w, cin, cout, up, kind, R)
    ws, ws16 = K.split_bf16x2(wt), K.split16_bf16x2(wt)
    y = K.conv_mfma(x, wt, cout, w_split=ws, w_split16=ws16, **kw)
    # the kernel this case is here for (the K-split policy of csrc/conv_bf16x3.hip:few_tiles_split restated)
    tiles, nchunk = b * ((h + 15) // 16) * ((w + 15) // 16) * (4 if up else 1) * (cout // 128), cin // 32
    ksplit = tiles <= 128 and nchunk >= 4 and min(-(-256 // tiles), nchunk // 2) >= 2
    assert K.LAST_REGION_PATH == (2 if (cout % 256 == 0 and not ksplit and K.REGION_1W) else 1)
    assert torch.equal(y, K.conv_mfma(x, wt, cout, w_split=ws, w_split16=ws16, **kw))
    ref = K.conv_mfma(x, wt, cout, **kw)
    sel = K.conv_mfma(x, wt, cout, w_split=ws, **kw)
    scale = float(ref.abs().max())
    assert 0 < maxabs(y, ref) < 1e-4 * scale
    assert maxabs(y, sel) < 5e-6 * scale
    if kind == "noise":
        assert torch.equal(y, sel)
    else:
        assert maxabs(y, sel) > 0                                        # the variant-rows kernel really produced these tiles
    if kind == "half-noise":                                             # left-most tiles: fallback (bit-equal); right-most: rows kernel
        assert torch.equal(y[:, :, :16], sel[:, :, :16]) and not torch.equal(y[:, :, -16:], sel[:, :, -16:])


def test_region_rows_kernel_replays_in_a_graph_with_another_mask():
    """The tile analysis (variant rows, overflow flags) happens inside the launch from the label map it is handed: a captured launch
    replayed after the labels changed == the eager launch on the new labels."""
    from e4s_amd import kernels as K
    x, wt, kw = _region_case(2, 64, 64, 64, 128, False, "face")
    _, _, kw2 = _region_case(2, 64, 64, 64, 128, False, "half-noise", seed=43)
    ws, ws16 = K.split_bf16x2(wt), K.split16_bf16x2(wt)
    lab = kw["labels"][:, ::8, ::8].contiguous()                        # [2,64,64] static label buffer
    kw["labels"] = lab
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        K.conv_mfma(x, wt, 128, w_split=ws, w_split16=ws16, **kw)
    torch.cuda.current_stream().wait_stream(st)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        y = K.conv_mfma(x, wt, 128, w_split=ws, w_split16=ws16, **kw)
    lab.copy_(kw2["labels"])
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, K.conv_mfma(x, wt, 128, w_split=ws, w_split16=ws16, **kw))
    lab.copy_(torch.zeros_like(lab))
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, K.conv_mfma(x, wt, 128, w_split=ws, w_split16=ws16, **kw))


def test_bf16x3_rejects_shapes_it_does_not_cover():
    from e4s_amd import kernels as K
    x = torch.zeros(1, 16, 16, 64, device=DEV)
    w = torch.zeros(1, 9, 48, 64, device=DEV)
    with pytest.raises(RuntimeError):
        K.conv_mfma(x, w, 48, w_split=K.split_bf16x2(w))                 # Cout % 32 != 0
    w = torch.zeros(1, 9, 64, 64, device=DEV)
    labels = torch.zeros(1, 16, 16, device=DEV, dtype=torch.uint8)
    s = torch.ones(12, 64, device=DEV)
    with pytest.raises(RuntimeError):                                    # region-select needs 128-wide column tiles
        K.conv_mfma(x, w, 64, w_split=K.split_bf16x2(w), labels=labels, num_regions=12, in_scale=s, out_scale=s)


@pytest.mark.parametrize("b,h,w,cin,cout", [(2, 32, 32, 64, 128), (1, 16, 48, 128, 128), (2, 8, 8, 256, 512)])
def test_conv_bf16x3_fused_instnorm_equals_unfused_bitwise(b, h, w, cin, cout):
    """in_stats: InstanceNorm folded into the halo staging == e4s_instnorm_apply_f32 followed by the same kernel, bit
    for bit (the same (x - mean) * rstd in fp32 before the hi/lo split), incl. the zero padding of the NORMALISED map."""
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(33)
    x = (torch.randn(b, h, w, cin, generator=g) * 2.0 + 0.7).to(DEV)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    slope = (torch.rand(cout, generator=g) * 0.5).to(DEV)
    wp = _pack(wt).to(DEV)
    ws = K.split_bf16x2(wp)
    st, _ = K.instnorm_stats(x)
    fused = K.conv_mfma(x, wp, cout, w_split=ws, in_stats=st, act=2, slope=slope)
    unfused = K.conv_mfma(K.instnorm_apply(x, st), wp, cout, w_split=ws, act=2, slope=slope)
    assert torch.equal(fused, unfused)
    xn = F.instance_norm(x.permute(0, 3, 1, 2).double().cpu(), eps=1e-5)
    want = F.prelu(F.conv2d(xn, wt.double(), padding=1), slope.double().cpu())
    assert maxabs(K.nhwc_to_nchw(fused), want) < 1e-4 * float(want.abs().max())


@pytest.mark.parametrize("cin,cout,res", [(128, 64, 32), (64, 32, 48), (256, 128, 16)])
def test_unmasked_polyphase_upconv_bf16x3_vs_oracle(cin, cout, res, monkeypatch):
    """Unmasked up-sampling StyledConv (the 512^2 / 1024^2 layers, model.py:655-657) on the plain split-bf16 kernel in
    polyphase form (ncls = 4) with 128- / 64- / 32-wide column tiles, against the oracle's conv_transpose2d + blur."""
    from e4s_amd import kernels as K
    from e4s_amd import stylegan2
    from e4s_amd.stylegan2 import StyledConv
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    monkeypatch.setattr(stylegan2, "UPCONV_BF16X3_EXACT", False)       # the polyphase statement (E4S_UPCONV_BF16X3=polyphase)
    sd = _styled_sd(cin, cout, True, 14)
    m = StyledConv(cin, cout, 3, 512, upsample=True, mask_op=False)
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(2, cin, res, res, generator=g)
    style = torch.randn(2, 512, generator=g)
    noise = torch.randn(2, 1, 2 * res, 2 * res, generator=g)
    want = orc.styled_conv(sd, "", x, style, None, noise, True, False)
    got = m(x.to(DEV), style.to(DEV), None, noise=noise.to(DEV))
    monkeypatch.setattr(K, "PRECISION", "f32")
    got32 = m(x.to(DEV), style.to(DEV), None, noise=noise.to(DEV))
    assert 0.0 < maxabs(got, got32)
    assert maxabs(got, want) < 1e-4 * float(want.abs().max())


@pytest.mark.parametrize("b,cin,cout,h,w", [(2, 128, 64, 32, 32), (3, 64, 32, 24, 40), (2, 256, 128, 16, 16), (1, 64, 32, 15, 33), (2, 192, 96, 9, 20),
                                            (1, 128, 64, 256, 256), (1, 64, 32, 512, 512)])
def test_unmasked_exact_upconv_bf16x3_vs_oracle(b, cin, cout, h, w, monkeypatch):
    """the unmasked up-sampling StyledConvs (model.py:287-300 + Blur :206-213; the 128 -> 64 -> 512^2 and
    64 -> 32 -> 1024^2 layers of a face swap, run here at their FULL sizes too) on the exact split-bf16 sub-pixel GEMM
    (e4s_upconv_bf16x3_f32: 9 Cin Cout MACs per input pixel) + FIR epilogue, against the oracle's conv_transpose2d + blur;
    odd, non-square and partial-tile geometries; per-sample and shared noise maps; <= 5e-5 of the output scale.  (The blur kernel of
    the reference is an outer product: this is the kernel's row pass + column pass FIR; the generic 16-tap pass has its own test below.)"""
    from e4s_amd import kernels as K
    from e4s_amd import stylegan2
    from e4s_amd.stylegan2 import StyledConv
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    assert stylegan2.UPCONV_BF16X3_EXACT
    sd = _styled_sd(cin, cout, True, 15)
    m = StyledConv(cin, cout, 3, 512, upsample=True, mask_op=False)
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(b, cin, h, w, generator=g)
    style = torch.randn(b, 512, generator=g)
    noise = torch.randn(b if b > 1 else 1, 1, 2 * h, 2 * w, generator=g)
    want = orc.styled_conv(sd, "", x, style, None, noise, True, False)
    calls = []
    real = K.upconv_bf16x3
    monkeypatch.setattr(K, "upconv_bf16x3", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = m(x.to(DEV), style.to(DEV), None, noise=noise.to(DEV))
    assert calls, "the exact split-bf16 up-conv kernel was not the one that ran"
    assert got.shape == want.shape
    scale = float(want.abs().max())
    assert maxabs(got, want) < 5e-5 * scale, (maxabs(got, want), scale)
    got2 = m(x.to(DEV), style.to(DEV), None, noise=noise.to(DEV))
    assert torch.equal(got, got2)                                  # no atomics anywhere: bit-reproducible


@pytest.mark.parametrize("separable", [False, True])
def test_exact_upconv_kernel_with_an_arbitrary_4x4_blur_kernel_vs_fp64(separable):
    """e4s_upconv_bf16x3_f32 called directly: the FIR epilogue factors the blur kernel into a row pass and a column pass when it is an
    outer product (checked in the kernel, on the values) and runs the generic 16-tap pass otherwise.  Both against fp64
    conv_transpose2d + upfirdn2d (model.py:287-300, 206-213) with a kernel that is NOT symmetric (the flip matters), partial tiles, two
    samples with their own style."""
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(71)
    b, cin, cout, h, w = 2, 64, 32, 21, 30
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    s = torch.rand(b, cin, generator=g) + 0.5
    d = torch.rand(b, cout, generator=g) + 0.5
    k4 = torch.outer(torch.tensor([0.7, 2.0, 3.1, 0.4]), torch.tensor([1.0, 2.5, 3.0, 1.5])) / 16 if separable else \
        torch.randn(4, 4, generator=g) / 4
    f64 = torch.float64
    want = torch.stack([orc.upfirdn2d(F.conv_transpose2d((x[i] * s[i][:, None, None])[None].to(f64), wt.to(f64).transpose(0, 1), stride=2),
                                      k4.to(f64), pad=(1, 1))[0] * d[i].to(f64)[:, None, None] for i in range(b)])
    got = K.nhwc_to_nchw(K.upconv_bf16x3(K.nchw_to_nhwc(x.to(DEV)), K.subpixel_weights(wt.to(DEV)), cout, k4.to(DEV).contiguous(),
                                         in_scale=s.to(DEV), out_scale=d.to(DEV)))
    assert got.shape == want.shape
    scale = float(want.abs().max())
    assert maxabs(got, want) < 5e-5 * scale, (maxabs(got, want), scale)


@pytest.mark.parametrize("b,cout,h,w", [(2, 32, 48, 48), (1, 32, 37, 70), (3, 64, 16, 33), (1, 32, 256, 256)])
def test_conv_c32_resident_weights_and_fused_torgb_vs_oracle(b, cout, h, w, monkeypatch):
    """the Cin == 32 StyledConv (the generator's 32 -> 32 layer at 1024^2) on e4s_conv_c32_bf16x3_f32 -- weights
    resident in LDS, halos fetched two tiles ahead, partial edge tiles -- against the oracle's modulated conv + noise + bias +
    activation (<= 5e-5 of the output scale); and the ToRGB contraction fused into its epilogue + e4s_torgb_finish_f32 against
    the standalone e4s_torgb_f32 pass over the same activation (model.py:422-448) and against the oracle."""
    from e4s_amd import kernels as K
    from e4s_amd import stylegan2
    from e4s_amd.stylegan2 import StyledConv, ToRGB
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    assert stylegan2.CONV_C32
    sd = _styled_sd(32, cout, False, 16)
    m = StyledConv(32, cout, 3, 512, upsample=False, mask_op=False)
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(b, 32, h, w, generator=g)
    style = torch.randn(b, 512, generator=g)
    noise = torch.randn(b if b > 1 else 1, 1, h, w, generator=g)
    want = orc.styled_conv(sd, "", x, style, None, noise, False, False)
    calls = []
    real = K.conv_c32
    monkeypatch.setattr(K, "conv_c32", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = m(x.to(DEV), style.to(DEV), None, noise=noise.to(DEV))
    assert calls, "the Cin == 32 kernel was not the one that ran"
    scale = float(want.abs().max())
    assert maxabs(got, want) < 5e-5 * scale, (maxabs(got, want), scale)
    assert torch.equal(got, m(x.to(DEV), style.to(DEV), None, noise=noise.to(DEV)))
    if cout != 32:
        return
    # ---- fused ToRGB ----
    rgb_sd = {"conv.weight": synth.synth_tensor("rgb.w", (1, 3, 32, 1, 1), "randn", 3),
              "conv.modulation.weight": synth.synth_tensor("rgb.mw", (32, 512), "randn", 3),
              "conv.modulation.bias": synth.synth_tensor("rgb.mb", (32,), "modbias", 3),
              "bias": synth.synth_tensor("rgb.b", (1, 3, 1, 1), "bias", 3), "upsample.kernel": orc.make_blur_kernel() * 4}
    t = ToRGB(32, 512, mask_op=False)
    t.load_state_dict(rgb_sd)
    t = t.to(DEV)
    style_rgb = torch.randn(b, 512, generator=g)
    skip = torch.randn(b, 3, h // 2, w // 2, generator=g) if (h % 2 == 0 and w % 2 == 0) else None
    s_c = K.modulate_vec(style.to(DEV), m.conv.modulation.weight, m.conv.modulation.bias)
    d = K.demod_coefs(s_c, m.conv.packed()["wsq"], m.conv.scale)
    s_r = K.modulate_vec(style_rgb.to(DEV), t.conv.modulation.weight, t.conv.modulation.bias)
    ws = K.rgb_weights(t.conv.packed()["w"].view(3, -1), s_r, t.conv.scale)
    xn = K.nchw_to_nhwc(x.to(DEV))
    nzd = noise.to(DEV)
    y, partial = K.conv_c32(xn, m.conv.split_weights(), 32, in_scale=s_c, out_scale=d, noise=nzd, noise_w=m.noise.weight,
                            bias=m.activate.bias, act=1, alpha=m.activate.negative_slope, gain=m.activate.scale, rgb_ws=ws)
    assert torch.equal(K.nhwc_to_nchw(y), got)                         # the rgb epilogue does not disturb y
    skd = skip.to(DEV) if skip is not None else None
    fused = K.torgb_finish(partial, t.bias, skd, t.upsample.kernel if skd is not None else None)
    separate = K.torgb(y, ws, t.bias, skd, t.upsample.kernel if skd is not None else None, None, 1)
    rscale = float(separate.abs().max())
    assert maxabs(fused, separate) < 2e-6 * rscale
    want_rgb = orc.to_rgb(rgb_sd, "", want, style_rgb, None, skip, False)
    assert maxabs(fused, want_rgb) < 1e-4 * float(want_rgb.abs().max())


# ---------------------------------------------------------------------------------------------
# generator layers against the oracle
# ---------------------------------------------------------------------------------------------
def _styled_sd(cin, cout, up, seed):
    spec = [("conv.weight", (1, cout, cin, 3, 3), "randn"), ("conv.modulation.weight", (cin, 512), "randn"),
            ("conv.modulation.bias", (cin,), "modbias"), ("noise.weight", (1,), "noisew"),
            ("activate.bias", (cout,), "bias")]
    sd = {k: synth.synth_tensor(k, s, kind, seed) for k, s, kind in spec}
    if up:
        sd["conv.blur.kernel"] = orc.make_blur_kernel() * 4
    return sd


@pytest.mark.parametrize("cin,cout,res,up", [(512, 512, 16, False), (512, 512, 8, True), (256, 128, 16, True),
                                              (64, 32, 32, False), (128, 64, 16, True)])
def test_modulated_conv_vs_oracle(cin, cout, res, up):
    from e4s_amd.stylegan2 import ModulatedConv2d
    sd = _styled_sd(cin, cout, up, 11)
    m = ModulatedConv2d(cin, cout, 3, 512, upsample=up)
    m.load_state_dict({k[5:]: v for k, v in sd.items() if k.startswith("conv.")})
    m = m.to(DEV)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, cin, res, res, generator=g)
    style = torch.randn(2, 512, generator=g)
    want = orc.modulated_conv2d(x, style, sd["conv.weight"], sd["conv.modulation.weight"],
                                sd["conv.modulation.bias"], True, up)
    got = m(x.to(DEV), style.to(DEV))
    assert got.shape == want.shape
    assert maxabs(got, want) < 5e-5          # fp32 both sides, different summation order


@pytest.mark.parametrize("use_plan", [False, True])
@pytest.mark.parametrize("cin,cout,res,up,cells", [(512, 512, 16, False, 16), (512, 512, 8, True, 4),
                                                    (256, 256, 32, False, 8), (512, 256, 16, True, 32),
                                                    (512, 512, 4, False, 64), (512, 512, 4, True, 64)])
def test_styled_conv_masked_vs_oracle(cin, cout, res, up, cells, use_plan):
    """Region-select (in-GEMM per-pixel style, or the gathered row plan) == the reference's 12 passes x
    one-hot mask."""
    from e4s_amd.stylegan2 import StyledConv
    sd = _styled_sd(cin, cout, up, 12)
    m = StyledConv(cin, cout, 3, 512, upsample=up, mask_op=True)
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(6)
    b = 2
    x = torch.randn(b, cin, res, res, generator=g)
    style = torch.randn(b, 12, 512, generator=g)
    mask = synth.onehot(synth.synth_labels_blocks(b, 512, cells, seed=7))
    out_res = res * 2 if up else res
    noise = torch.randn(b, 1, out_res, out_res, generator=g)
    want = orc.styled_conv(sd, "", x, style, mask, noise, up, True)
    got = m(x.to(DEV), style.to(DEV), mask.to(DEV), noise=noise.to(DEV), use_plan=use_plan)
    assert maxabs(got, want) < 5e-5


@pytest.mark.parametrize("cin,cout,res,up,cells,masked", [
    (512, 512, 16, False, 16, True), (512, 512, 8, True, 4, True), (256, 256, 32, False, 8, True),
    (512, 256, 16, True, 32, True), (512, 512, 4, False, 64, True), (512, 512, 4, True, 64, True),
    (128, 128, 32, False, 64, True), (256, 128, 16, True, 8, False), (128, 128, 16, False, 8, False)])
def test_styled_conv_bf16x3_vs_oracle(cin, cout, res, up, cells, masked, monkeypatch):
    """The region-select split-bf16 kernel (per-pixel style applied to the A fragment before the hi/lo split; polyphase
    form for up-convs) == the reference's 12 passes x one-hot mask, to 1e-4 of the output scale (error model in
    test_conv_bf16x3_vs_conv2d_f64); the fp32 kernels measure ~1e-6 here."""
    from e4s_amd import kernels as K
    from e4s_amd.stylegan2 import StyledConv
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    sd = _styled_sd(cin, cout, up, 12)
    m = StyledConv(cin, cout, 3, 512, upsample=up, mask_op=masked)
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(6)
    b = 2
    x = torch.randn(b, cin, res, res, generator=g)
    style = torch.randn(b, 12, 512, generator=g) if masked else torch.randn(b, 512, generator=g)
    mask = synth.onehot(synth.synth_labels_blocks(b, 512, cells, seed=7))
    out_res = res * 2 if up else res
    noise = torch.randn(b, 1, out_res, out_res, generator=g)
    want = orc.styled_conv(sd, "", x, style, mask if masked else None, noise, up, masked)
    got = m(x.to(DEV), style.to(DEV), mask.to(DEV) if masked else None, noise=noise.to(DEV))
    monkeypatch.setattr(K, "PRECISION", "f32")
    got32 = m(x.to(DEV), style.to(DEV), mask.to(DEV) if masked else None, noise=noise.to(DEV))
    scale = float(want.abs().max())
    assert 0.0 < maxabs(got, got32)                                  # the split-bf16 kernel really ran
    assert maxabs(got, want) < 1e-4 * scale, (maxabs(got, want), scale)


def test_styled_conv_per_channel_noise_and_unmasked():
    from e4s_amd.stylegan2 import StyledConv
    sd = _styled_sd(64, 64, False, 13)
    m = StyledConv(64, 64, 3, 512, mask_op=False)
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 64, 32, 32, generator=g)
    style = torch.randn(2, 512, generator=g)
    noise = torch.randn(1, 64, 32, 32, generator=g)             # scripts/face_edit.py:49-52
    want = orc.styled_conv(sd, "", x, style, None, noise, False, False)
    got = m(x.to(DEV), style.to(DEV), None, noise=noise.to(DEV))
    assert maxabs(got, want) < 5e-5


@pytest.mark.parametrize("cin,res,masked,with_skip", [(512, 8, True, True), (128, 32, False, True),
                                                       (32, 64, False, True), (512, 4, True, False)])
def test_torgb_vs_oracle(cin, res, masked, with_skip):
    from e4s_amd.stylegan2 import ToRGB
    spec = [("bias", (1, 3, 1, 1), "bias"), ("conv.weight", (1, 3, cin, 1, 1), "randn"),
            ("conv.modulation.weight", (cin, 512), "randn"), ("conv.modulation.bias", (cin,), "modbias")]
    sd = {k: synth.synth_tensor(k, s, kind, 3) for k, s, kind in spec}
    m = ToRGB(cin, 512, upsample=with_skip, mask_op=masked)
    if with_skip:
        sd["upsample.kernel"] = orc.make_blur_kernel() * 4
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, cin, res, res, generator=g)
    style = torch.randn(2, 12, 512, generator=g) if masked else torch.randn(2, 512, generator=g)
    mask = synth.onehot(synth.synth_labels_blocks(2, 512, 8, seed=4))
    skip = torch.randn(2, 3, res // 2, res // 2, generator=g) if with_skip else None
    want = orc.to_rgb(sd, "", x, style, mask, skip, masked)
    got = m(x.to(DEV), style.to(DEV), mask.to(DEV), None if skip is None else skip.to(DEV))
    assert maxabs(got, want) < 5e-5


# ---------------------------------------------------------------------------------------------
# encoder pieces against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h,w,cin,cout,stride", [(2, 32, 32, 64, 128, 1), (3, 32, 48, 128, 256, 2), (2, 16, 16, 512, 512, 1)])
def test_se_gate_fused_with_the_statistics_finalisation(b, h, w, cin, cout, stride, monkeypatch):
    """conv -> InstanceNorm statistics -> SE gate: with `se` the gate leaves the launch that adds the epilogue's partial sums
    (e4s_instnorm_finalize_se_f32) -- same statistics bit for bit, gate == e4s_se_gate_f32 on the pooled vector bit for bit, and
    == sigmoid(fc2 relu(fc1 pooled)) in fp64."""
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    g = torch.Generator().manual_seed(71)
    x = torch.randn(b, h, w, cin, generator=g).to(DEV)
    wt = (torch.randn(1, 9, cout, cin, generator=g) / math.sqrt(9 * cin)).to(DEV)
    ws = K.split_bf16x2(wt)
    cr = cout // 16
    fc1 = (torch.randn(cr, cout, generator=g) * 50).to(DEV)          # pooled is a rounding residue (~1e-8 .. 1e-7): make the gate move
    fc2 = (torch.randn(cout, cr, generator=g) * 1e6).to(DEV)
    kw = dict(w_split=ws, want_stats=True, istride=stride)
    y0, (st0, pooled) = K.conv_mfma(x, wt, cout, **kw)
    y1, (st1, gate) = K.conv_mfma(x, wt, cout, se=(fc1, fc2), **kw)
    assert torch.equal(y0, y1) and torch.equal(st0, st1)
    assert torch.equal(gate, K.se_gate(pooled, fc1, fc2))
    ref = torch.sigmoid(torch.relu(pooled.double() @ fc1.double().t()) @ fc2.double().t())
    assert float((gate.double() - ref).abs().max()) < 1e-5 and float((gate - 0.5).abs().max()) > 1e-4


@pytest.mark.parametrize("cin,depth,stride,res", [(64, 128, 2, 64), (128, 128, 1, 32), (512, 512, 2, 32)])
def test_encoder_unit_vs_oracle(cin, depth, stride, res):
    from e4s_amd.encoders import bottleneck_IR_SE_Ours
    spec = [("res_layer.1.weight", (depth, cin, 3, 3), "conv"), ("res_layer.2.weight", (depth,), "prelu"),
            ("res_layer.3.weight", (depth, depth, 3, 3), "conv"),
            ("res_layer.5.fc1.weight", (depth // 16, depth, 1, 1), "conv"),
            ("res_layer.5.fc2.weight", (depth, depth // 16, 1, 1), "conv")]
    if cin != depth:
        spec.append(("shortcut_layer.0.weight", (depth, cin, 1, 1), "conv"))
    sd = {k: synth.synth_tensor(k, s, kind, 5) for k, s, kind in spec}
    m = bottleneck_IR_SE_Ours(cin, depth, stride)
    m.load_state_dict(sd)
    m = m.to(DEV)
    x = torch.randn(2, cin, res, res, generator=torch.Generator().manual_seed(10)) * 1.7 + 0.3
    want = orc.encoder_unit(sd, "", x, cin, depth, stride)
    assert maxabs(m(x.to(DEV)), want) < 5e-5


def test_region_mean_exact_zero_for_empty_regions():
    from e4s_amd.encoders import FSEncoder_PSP
    with torch.device("meta"):
        enc = FSEncoder_PSP()
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(2, 256, 64, 64, generator=g)
    lab = synth.synth_labels_face(2, 512, seed=5)
    lab[lab == 9] = 1                                           # region 9 (teeth) empty
    mask = synth.onehot(lab)
    want = orc.region_mean(feats, mask)
    got = enc.get_per_comp_styleCode(feats.to(DEV), mask.to(DEV))
    assert maxabs(got, want) < 1e-5
    assert float(got[:, 9].abs().max()) == 0.0                  # face_swap.py:132,136 test `sum == 0`


# ---------------------------------------------------------------------------------------------
# Net3 end-to-end against the golden fixtures of the REAL reference
# ---------------------------------------------------------------------------------------------
def _net(out_size):
    from e4s_amd.networks import Net3
    from e4s_amd.options import make_opts
    net = Net3(make_opts(out_size=out_size))
    net.load_state_dict(synth.synth_state_dict(out_size, 13), strict=True)
    net.latent_avg = synth.synth_latent_avg(out_size).to(DEV)
    return net.to(DEV).eval()


def _swap_inputs(mask_kind):
    driven = synth.synth_image(1, 1024, tag="driven")
    target = synth.synth_image(1, 1024, tag="target")
    mk = synth.synth_labels_face if mask_kind == "face" else (lambda b, s, seed: synth.synth_labels_blocks(b, s, 64, seed=seed))
    dm, tm, sm = (synth.onehot(mk(1, 512, seed=s)) for s in (1, 2, 3))
    return driven, target, dm, tm, sm


@torch.no_grad()
def test_net256_swap_vs_golden(golden):
    from e4s_amd.networks import swap_comp_style_vector
    g = golden("net256.pt")
    net = _net(256)
    driven, target, dm, tm, sm = _swap_inputs("blocks")
    d_sv, struct = net.get_style_vectors(driven.to(DEV), dm.to(DEV))
    t_sv, _ = net.get_style_vectors(target.to(DEV), tm.to(DEV))
    assert tuple(struct.shape) == (1, 512, 16, 16) and float(struct.abs().max()) == 0.0
    assert maxabs(d_sv, g["driven_sv"]) < 1e-4
    assert maxabs(t_sv, g["target_sv"]) < 1e-4
    sv = swap_comp_style_vector(t_sv, d_sv, set(range(12)) - {0, 4, 11, 10})
    assert maxabs(sv, g["swapped_sv"]) < 1e-4
    codes = net.cal_style_codes(g["swapped_sv"].to(DEV))
    assert tuple(codes.shape) == (1, 12, 14, 512)
    assert maxabs(codes[:, :, :, ::8], g["codes_stride"]) < 1e-4
    noise = [n.to(DEV) for n in synth.synth_noise(256)]
    img, minus1, feats = net.gen_img(torch.zeros(1, 512, 32, 32, device=DEV), codes, sm.to(DEV), noise=noise)
    assert minus1 == -1 and tuple(img.shape) == (1, 3, 256, 256) and tuple(feats.shape) == (1, 512, 16, 16)
    assert maxabs(feats[:, ::4], g["feats_stride"]) < 1e-3
    assert maxabs(img, g["img"]) < 1e-3                          # north_star tolerance


@torch.no_grad()
def test_net1024_swap_vs_golden(golden):
    """BASELINE.json configs[1]: single 1024^2 face swap, against the real reference's output."""
    from e4s_amd.networks import face_swap_core
    g = golden("net1024.pt")
    net = _net(1024)
    driven, target, dm, tm, sm = _swap_inputs("face")
    noise = [n.to(DEV) for n in synth.synth_noise(1024)]
    img = face_swap_core(net, driven.to(DEV), dm.to(DEV), target.to(DEV), tm.to(DEV), sm.to(DEV), noise=noise)
    assert tuple(img.shape) == (1, 3, 1024, 1024)
    assert maxabs(img[:, :, ::8, ::8], g["img_stride8"]) < 1e-3
    c0 = 512 - 64
    assert maxabs(img[:, :, c0:c0 + 128, c0:c0 + 128], g["img_crop"]) < 1e-3
    assert maxabs(img.mean((2, 3)), g["img_mean"]) < 1e-4
    assert maxabs(img.abs().mean((2, 3)), g["img_absmean"]) < 1e-4


@torch.no_grad()
def test_net1024_swap_vs_golden_bf16x3(golden, monkeypatch):
    """The same 1024^2 swap with the encoder's stride-1 convs on the split-bf16 kernel (E4S_PRECISION=bf16x3): the
    north-star bound of 1e-3 against the real reference's output must still hold."""
    from e4s_amd import kernels as K
    from e4s_amd.networks import face_swap_core
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    g = golden("net1024.pt")
    net = _net(1024)
    driven, target, dm, tm, sm = _swap_inputs("face")
    noise = [n.to(DEV) for n in synth.synth_noise(1024)]
    sv, _ = net.get_style_vectors(driven.to(DEV), dm.to(DEV))
    monkeypatch.setattr(K, "PRECISION", "f32")
    sv32, _ = net.get_style_vectors(driven.to(DEV), dm.to(DEV))
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    sv_err = maxabs(sv, sv32)
    assert 0.0 < sv_err < 2e-4, sv_err                      # > 0: the split-bf16 kernel really ran
    img = face_swap_core(net, driven.to(DEV), dm.to(DEV), target.to(DEV), tm.to(DEV), sm.to(DEV), noise=noise)
    e1 = maxabs(img[:, :, ::8, ::8], g["img_stride8"])
    c0 = 512 - 64
    e2 = maxabs(img[:, :, c0:c0 + 128, c0:c0 + 128], g["img_crop"])
    print(f"bf16x3: style-vector delta vs fp32 path {sv_err:.3e}; image max-abs vs reference {max(e1, e2):.3e}")
    assert e1 < 1e-3 and e2 < 1e-3, (e1, e2)


@torch.no_grad()
def test_net256_swap_vs_golden_bf16x3(golden, monkeypatch):
    """BASELINE.json configs[0] plumbing with the split-bf16 encoder: style vectors within 3e-4 of the real
    reference's, image within the 1e-3 north-star bound."""
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    g = golden("net256.pt")
    net = _net(256)
    driven, target, dm, tm, sm = _swap_inputs("blocks")
    d_sv, _ = net.get_style_vectors(driven.to(DEV), dm.to(DEV))
    assert 0.0 < maxabs(d_sv, g["driven_sv"]) < 3e-4
    codes = net.cal_style_codes(g["swapped_sv"].to(DEV))
    noise = [n.to(DEV) for n in synth.synth_noise(256)]
    img, _, _ = net.gen_img(torch.zeros(1, 512, 32, 32, device=DEV), codes, sm.to(DEV), noise=noise)
    assert maxabs(img, g["img"]) < 1e-3


@torch.no_grad()
def test_discriminator_vs_golden(golden):
    """Discriminator(64) -- HIP blur (upfirdn2d pad modes of model.py:683-689) and fused
    bias+leaky-ReLU inside the ResBlock stack -- against the REAL reference's logits and 4x4 feature map."""
    from e4s_amd.stylegan2 import Discriminator
    g = golden("disc64.pt")
    d = Discriminator(64)
    d.load_state_dict(synth.synth_disc_state_dict(64), strict=True)
    d = d.to(DEV).eval()
    x = synth.synth_image(4, 64, tag="disc").to(DEV)
    feats = d.convs(x)
    assert maxabs(feats, g["feats"]) < 1e-4 * float(g["feats"].abs().max())
    assert maxabs(d(x), g["logits"]) < 1e-4


@torch.no_grad()
def test_gen1024_properties_batch_and_region_relabel():
    """Size-independent properties at the full 1024^2 size (no oracle needed):
    (1) a batch of 2 equals two batches of 1 bit-for-bit per sample (row order inside the gathered GEMM
        must not matter); (2) relabelling regions (permute mask channels and the style rows the same
        way) leaves the image unchanged -- region-select depends on the label only through its style."""
    net = _net(1024)
    g = torch.Generator().manual_seed(21)
    codes = (torch.randn(2, 12, 18, 512, generator=g) * 0.3).to(DEV)
    codes[:, :, 13:] = codes[:, :1, 13:]                         # layers >= K share one code (networks.py:152-154)
    lab = torch.cat([synth.synth_labels_face(1, 512, seed=8), synth.synth_labels_blocks(1, 512, 32, seed=9)], 0)
    mask = synth.onehot(lab).to(DEV)
    noise = [n.to(DEV) for n in synth.synth_noise(1024, batch=2)]
    img, _, _ = net.gen_img(None, codes, mask, noise=noise)
    for i in range(2):
        one, _, _ = net.gen_img(None, codes[i:i + 1], mask[i:i + 1], noise=[n[i:i + 1] for n in noise])
        assert torch.equal(one[0], img[i])
    perm = torch.randperm(11, generator=g) + 1                  # keep region 0 (used by unmasked layers) fixed
    perm = torch.cat([torch.zeros(1, dtype=torch.long), perm])
    img2, _, _ = net.gen_img(None, codes[:, perm].contiguous(), mask[:, perm].contiguous(), noise=noise)
    assert torch.equal(img2, img)
    assert bool(torch.isfinite(img).all())


def test_weight_repacking_kernels():
    """e4s_polyphase_weights_f32 / e4s_pack_taps_f32 against their CPU-tested torch statements."""
    from e4s_amd import kernels as K
    from e4s_amd.stylegan2 import polyphase_upconv_weights
    g = torch.Generator().manual_seed(31)
    w = torch.randn(40, 24, 3, 3, generator=g)
    blur = orc.make_blur_kernel() * 4
    assert maxabs(K.polyphase_weights(w.to(DEV), blur.to(DEV)), polyphase_upconv_weights(w, blur)) < 1e-6
    assert torch.equal(K.pack_taps(w.to(DEV)).cpu(), _pack(w))
    # the two split-bf16 images of tap-packed weights: [rows][Cin/32][32 hi | 32 lo] and [rows][Cin/16][Cout][16 hi | 16 lo]
    wt = torch.randn(2, 9, 8, 64, generator=g)
    hi = wt.bfloat16()
    lo = (wt - hi.float()).bfloat16()
    bits = lambda t: t.view(torch.int16)
    s32 = K.split_bf16x2(wt.to(DEV)).cpu().view(torch.int16).view(18, 8, 2, 2, 32)            # [row][co][chunk][hi|lo][32]
    assert torch.equal(s32[:, :, :, 0], bits(hi).view(18, 8, 2, 32)) and torch.equal(s32[:, :, :, 1], bits(lo).view(18, 8, 2, 32))
    s16 = K.split16_bf16x2(wt.to(DEV)).cpu().view(torch.int16).view(18, 4, 8, 2, 16)           # [row][chunk][co][hi|lo][16]
    want_hi = bits(hi).view(18, 8, 4, 16).permute(0, 2, 1, 3)
    want_lo = bits(lo).view(18, 8, 4, 16).permute(0, 2, 1, 3)
    assert torch.equal(s16[:, :, :, 0], want_hi) and torch.equal(s16[:, :, :, 1], want_lo)


# ---------------------------------------------------------------------------------------------
# backward: the fused generator / MLP gradients against the oracle's autograd
# ---------------------------------------------------------------------------------------------
def _gen_sd(size, seed=0):
    full = synth.synth_state_dict(size, 13, seed=seed)
    return {k[2:]: v for k, v in full.items() if k.startswith("G.")}


@pytest.mark.parametrize("size,K,cells", [(16, 13, 4), (64, 5, 16)])
def test_generator_backward_vs_oracle_autograd(size, K, cells):
    from e4s_amd.stylegan2 import Generator
    sd = _gen_sd(size)
    gen = Generator(size, 512, 8, split_layer_idx=5, remaining_layer_idx=K)
    gen.load_state_dict(sd, strict=True)
    gen = gen.to(DEV).eval()
    for p in gen.parameters():
        p.requires_grad = False
    g = torch.Generator().manual_seed(40)
    b, nl = 2, gen.n_latent
    lat = torch.randn(b, 12, nl, 512, generator=g) * 0.5
    mask = synth.onehot(synth.synth_labels_blocks(b, 512, cells, seed=3))
    noise = synth.synth_noise(size, seed=2, batch=b)
    w_img = torch.randn(b, 3, size, size, generator=g)
    w_ft = torch.randn(b, 512, 16, 16, generator=g)

    lat_d = lat.to(DEV).requires_grad_(True)
    img, _, feats = gen([lat_d], None, mask.to(DEV), input_is_latent=True, noise=[n.to(DEV) for n in noise])
    ((img * w_img.to(DEV)).sum() + (feats * w_ft.to(DEV)).sum()).backward()

    # Oracle autograd twice: fp32 (what the reference computes) and fp64 (ground truth).  The latent gradient is a
    # sum over all pixels/channels with heavy cancellation, so fp32 implementations differ by accumulation noise that
    # grows with resolution; the HIP path must be as close to the fp64 truth as the fp32 reference itself is
    # (within 3x), and within 2e-4 of the gradient scale where that noise is negligible.
    grads = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        lat_r = lat.detach().clone().to(dt).requires_grad_(True)
        sd_g = {"G." + k: v.to(dt) for k, v in sd.items()}
        img_r, feats_r = orc.generator_forward(sd_g, lat_r, mask.to(dt), [n.to(dt) for n in noise], size, K)
        ((img_r * w_img.to(dt)).sum() + (feats_r * w_ft.to(dt)).sum()).backward()
        grads[name] = lat_r.grad
        if name == "f32":
            assert maxabs(img, img_r) < 1e-4
    scale = float(grads["f64"].abs().max())
    ref_noise = maxabs(grads["f32"], grads["f64"])
    err = maxabs(lat_d.grad, grads["f64"])
    # measured: 16^2 -> err/scale 7e-7 ... 64^2 -> 7.4e-4 (4x the fp32 reference's own distance to fp64); every
    # component is checked tightly against fp64 in test_styled_conv_backward_vs_oracle_f64 / test_torgb_backward_*.
    assert err < max(3.0 * ref_noise, 1e-3 * scale), (err, ref_noise, scale)
    # unmasked layers only read region 0 (model.py:655-657): no gradient may leak to the other regions' rows
    if K < gen.n_latent:
        assert float(lat_d.grad[:, 1:, K + 1:].abs().max()) == 0.0


def test_style_codes_backward_vs_oracle_autograd():
    """cal_style_codes: gradients w.r.t. the style vectors (config 3) and the LocalMLP weights/biases (config 5)."""
    net = _net(256)
    sd = synth.synth_state_dict(256, 13)
    g = torch.Generator().manual_seed(41)
    sv = torch.randn(2, 12, 1280, generator=g)
    w = torch.randn(2, 12, 14, 512, generator=g)
    sv_d = sv.to(DEV).requires_grad_(True)
    codes = net.cal_style_codes(sv_d)
    (codes * w.to(DEV)).sum().backward()
    sd_r = {k: (v.clone().requires_grad_(True) if k.startswith("MLPs.") else v) for k, v in sd.items()}
    sv_r = sv.clone().requires_grad_(True)
    codes_r = orc.cal_style_codes(sd_r, sv_r, synth.synth_latent_avg(256), 13)
    (codes_r * w).sum().backward()
    assert maxabs(codes, codes_r) < 1e-4
    assert maxabs(sv_d.grad, sv_r.grad) < 1e-4 * float(sv_r.grad.abs().max())
    for i in (0, 5, 11):
        for j, nm in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias")):
            ref = sd_r[f"MLPs.{i}.mlp.{j}.{nm}"].grad
            got = getattr(net.MLPs[i].mlp[j], nm).grad
            assert maxabs(got, ref) < 2e-4 * float(ref.abs().max()), (i, j, nm)


def test_optimization_step_runs_and_descends():
    """scripts/optimization.py:209-232 in miniature at 256^2: Adam on the style vectors through
    cal_style_codes -> gen_img with an MSE loss; the loss must go down and gradients must be finite."""
    import warnings
    net = _net(256)
    for p in net.parameters():
        p.requires_grad = False
    target = synth.synth_image(1, 256, tag="opt_target").to(DEV)
    mask = synth.onehot(synth.synth_labels_face(1, 512, seed=6)).to(DEV)
    noise = [n.to(DEV) for n in synth.synth_noise(256)]
    g = torch.Generator().manual_seed(42)
    latent = (torch.randn(1, 12, 1280, generator=g) * 0.1).to(DEV).requires_grad_(True)
    opt = torch.optim.Adam([latent], lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        codes = net.cal_style_codes(latent)
        img, _, _ = net.gen_img(None, codes, mask, noise=noise)
        loss = torch.nn.functional.mse_loss(img, target)
        loss.backward()
        assert bool(torch.isfinite(latent.grad).all())
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("cin,cout,res,up,masked", [(64, 64, 16, False, True), (64, 64, 16, True, True),
                                                     (128, 64, 32, False, False), (64, 64, 24, True, False),
                                                     (512, 512, 8, False, True), (32, 32, 32, False, False),
                                                     (64, 32, 16, True, False), (512, 512, 32, False, False)])
def test_styled_conv_backward_vs_oracle_f64(cin, cout, res, up, masked):
    """One fused StyledConv: dL/dx (per-pixel, tight) and dL/dstyle against the oracle's fp64 autograd."""
    from e4s_amd import kernels as K
    from e4s_amd.autograd import styled_conv_backward
    from e4s_amd.stylegan2 import StyledConv
    sd = _styled_sd(cin, cout, up, 21)
    m = StyledConv(cin, cout, 3, 512, upsample=up, mask_op=masked)
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(50)
    b, r = 2, 12
    x = torch.randn(b, cin, res, res, generator=g)
    style = torch.randn(b, r, 512, generator=g) if masked else torch.randn(b, 512, generator=g)
    mask = synth.onehot(synth.synth_labels_blocks(b, 512, 16, seed=5))
    ores = res * 2 if up else res
    noise = torch.randn(b, 1, ores, ores, generator=g)
    wgt = torch.randn(b, cout, ores, ores, generator=g)

    xd = K.nchw_to_nhwc(x.to(DEV))
    mod = m.conv.modulation
    s = K.modulate_vec(style.reshape(-1, 512).to(DEV), mod.weight, mod.bias)
    labels = K.mask_labels(mask.to(DEV))[0] if masked else None
    rec = {}
    y = m.run_nhwc(xd, s, noise.to(DEV), labels, r, rec=rec)
    rec.update(layer=m, x=xd, y=y, s=s, labels=labels)
    extras = {}
    dx, ds = styled_conv_backward(rec, K.nchw_to_nhwc(wgt.to(DEV)), r, extras)
    dstyle = (ds @ mod.weight.detach()) * mod.scale
    from e4s_amd.autograd import styled_conv_weight_grad
    dweight = styled_conv_weight_grad(rec, extras, r)

    f64 = torch.float64
    sd64 = {k: v.to(f64) for k, v in sd.items()}
    sd64["conv.weight"].requires_grad_(True)
    xr = x.to(f64).requires_grad_(True)
    sr = style.to(f64).requires_grad_(True)
    yr = orc.styled_conv(sd64, "", xr, sr, mask.to(f64), noise.to(f64), up, masked)
    (yr * wgt.to(f64)).sum().backward()
    assert maxabs(K.nhwc_to_nchw(y), yr) < 5e-5
    assert maxabs(K.nhwc_to_nchw(dx), xr.grad) < 1e-4 * float(xr.grad.abs().max())
    assert maxabs(dstyle.view_as(sr), sr.grad) < 2e-4 * float(sr.grad.abs().max())
    wref = sd64["conv.weight"].grad
    assert maxabs(dweight, wref) < 2e-4 * float(wref.abs().max()), (maxabs(dweight, wref), float(wref.abs().max()))


@pytest.mark.parametrize("cin,cout,res", [(64, 64, 32), (32, 32, 48), (128, 64, 24), (64, 32, 40)])
def test_unmasked_styled_conv_dgrad_on_the_forward_kernels_vs_oracle_f64(cin, cout, res, monkeypatch):
    """Unmasked same-resolution StyledConv under the split-bf16 policy: dL/dx = s * conv(gz * d, flipped W^T) runs on the forward
    kernels (plain split-bf16 kernel; the resident-weights kernel when gz has 32 channels) + e4s_scale_dot_f32 (applies s, reduces
    dL/ds) instead of the exact-fp32 dx + ds kernel: both against the oracle's fp64 autograd, and close to the fp32 path."""
    from e4s_amd import kernels as K
    from e4s_amd.autograd import styled_conv_backward
    from e4s_amd.stylegan2 import StyledConv
    sd = _styled_sd(cin, cout, False, 23)
    m = StyledConv(cin, cout, 3, 512, upsample=False, mask_op=False)
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(52)
    b = 2
    x = torch.randn(b, cin, res, res, generator=g)
    style = torch.randn(b, 512, generator=g)
    noise = torch.randn(b, 1, res, res, generator=g)
    wgt = torch.randn(b, cout, res, res, generator=g)
    xd = K.nchw_to_nhwc(x.to(DEV))
    mod = m.conv.modulation
    s = K.modulate_vec(style.to(DEV), mod.weight, mod.bias)

    # ONE forward (exact fp32) for both backward paths: lrelu'(y) flips where a pre-activation is within the split-bf16 error of zero,
    # which would show up as isolated O(|dy|) differences in dx that have nothing to do with the dgrad kernels
    monkeypatch.setattr(K, "PRECISION", "f32")
    rec = {}
    y = m.run_nhwc(xd, s, noise.to(DEV), None, 1, rec=rec)
    rec.update(layer=m, x=xd, y=y, s=s, labels=None)

    def run(prec):
        monkeypatch.setattr(K, "PRECISION", prec)
        dx, ds = styled_conv_backward(rec, K.nchw_to_nhwc(wgt.to(DEV)), 1, {})
        return K.nhwc_to_nchw(dx), (ds @ mod.weight.detach()) * mod.scale

    dx, dstyle = run("bf16x3")
    dx32, dstyle32 = run("f32")
    f64 = torch.float64
    sd64 = {k: v.to(f64) for k, v in sd.items()}
    xr = x.to(f64).requires_grad_(True)
    sr = style.to(f64).requires_grad_(True)
    yr = orc.styled_conv(sd64, "", xr, sr, None, noise.to(f64), False, False)
    (yr * wgt.to(f64)).sum().backward()
    gs, ss = float(xr.grad.abs().max()), float(sr.grad.abs().max())
    assert maxabs(dx, xr.grad) < 1e-4 * gs, ("split-bf16 forward-kernel dgrad", maxabs(dx, xr.grad), gs)
    assert maxabs(dx32, xr.grad) < 1e-4 * gs, ("exact fp32 dx + ds kernel", maxabs(dx32, xr.grad), gs)
    assert 0 < maxabs(dx, dx32)                                   # another kernel, the same gradient
    assert maxabs(dstyle.view_as(sr), sr.grad) < 3e-4 * ss and maxabs(dstyle, dstyle32) < 3e-4 * ss


@pytest.mark.parametrize("cin,cout,res", [(128, 64, 32), (64, 32, 48), (64, 64, 16)])
def test_unmasked_upconv_dgrad_on_the_forward_kernel_vs_oracle_f64(cin, cout, res, monkeypatch):
    """Unmasked UP-SAMPLING StyledConv (model.py:287-300) under the split-bf16 policy: the four output phases of gz laid side by side in
    the channel dimension (e4s_pixel_unshuffle2_f32), then dL/dx = s * conv3x3(that * d, flipped polyphase W^T) on the forward kernel +
    e4s_scale_dot_f32 -- against the oracle's fp64 autograd of conv_transpose2d + blur, and against the exact-fp32 dx + ds kernel."""
    from e4s_amd import kernels as K
    from e4s_amd.autograd import styled_conv_backward
    from e4s_amd.stylegan2 import StyledConv
    sd = _styled_sd(cin, cout, True, 29)
    m = StyledConv(cin, cout, 3, 512, upsample=True, mask_op=False)
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(53)
    b = 2
    x = torch.randn(b, cin, res, res, generator=g)
    style = torch.randn(b, 512, generator=g)
    noise = torch.randn(b, 1, 2 * res, 2 * res, generator=g)
    wgt = torch.randn(b, cout, 2 * res, 2 * res, generator=g)
    xd = K.nchw_to_nhwc(x.to(DEV))
    mod = m.conv.modulation
    s = K.modulate_vec(style.to(DEV), mod.weight, mod.bias)
    # pixel unshuffle by itself, bit for bit against the torch view
    t = torch.randn(2, 6, 10, 8, generator=g).to(DEV)
    assert torch.equal(K.pixel_unshuffle2(t), t.view(2, 3, 2, 5, 2, 8).permute(0, 1, 3, 2, 4, 5).reshape(2, 3, 5, 32))
    monkeypatch.setattr(K, "PRECISION", "f32")           # one forward for both backward paths (see the same-resolution test)
    rec = {}
    y = m.run_nhwc(xd, s, noise.to(DEV), None, 1, rec=rec)
    rec.update(layer=m, x=xd, y=y, s=s, labels=None)

    def run(prec):
        monkeypatch.setattr(K, "PRECISION", prec)
        dx, ds = styled_conv_backward(rec, K.nchw_to_nhwc(wgt.to(DEV)), 1, {})
        return K.nhwc_to_nchw(dx), (ds @ mod.weight.detach()) * mod.scale

    dx, dstyle = run("bf16x3")
    dx32, dstyle32 = run("f32")
    f64 = torch.float64
    sd64 = {k: v.to(f64) for k, v in sd.items()}
    xr = x.to(f64).requires_grad_(True)
    sr = style.to(f64).requires_grad_(True)
    yr = orc.styled_conv(sd64, "", xr, sr, None, noise.to(f64), True, False)
    (yr * wgt.to(f64)).sum().backward()
    gs, ss = float(xr.grad.abs().max()), float(sr.grad.abs().max())
    assert maxabs(dx, xr.grad) < 1e-4 * gs, ("split-bf16 forward-kernel up-conv dgrad", maxabs(dx, xr.grad), gs)
    assert maxabs(dx32, xr.grad) < 1e-4 * gs, ("exact fp32 dx + ds kernel", maxabs(dx32, xr.grad), gs)
    assert 0 < maxabs(dx, dx32)                                   # another kernel, the same gradient
    assert maxabs(dstyle.view_as(sr), sr.grad) < 3e-4 * ss and maxabs(dstyle, dstyle32) < 3e-4 * ss


@pytest.mark.parametrize("cin,res,masked,with_skip", [(512, 8, True, True), (128, 32, False, True), (512, 4, True, False),
                                                       (32, 32, False, True)])
def test_torgb_backward_vs_oracle_f64(cin, res, masked, with_skip):
    """ToRGB inside the fused generator: gradients w.r.t. activation, style and skip against fp64 autograd."""
    from e4s_amd import kernels as K
    from e4s_amd.stylegan2 import ToRGB
    spec = [("bias", (1, 3, 1, 1), "bias"), ("conv.weight", (1, 3, cin, 1, 1), "randn"),
            ("conv.modulation.weight", (cin, 512), "randn"), ("conv.modulation.bias", (cin,), "modbias")]
    sd = {k: synth.synth_tensor(k, s, kind, 3) for k, s, kind in spec}
    m = ToRGB(cin, 512, upsample=with_skip, mask_op=masked)
    if with_skip:
        sd["upsample.kernel"] = orc.make_blur_kernel() * 4
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(51)
    b, r = 2, 12
    x = torch.randn(b, cin, res, res, generator=g)
    style = torch.randn(b, r, 512, generator=g) if masked else torch.randn(b, 512, generator=g)
    mask = synth.onehot(synth.synth_labels_blocks(b, 512, 8, seed=6))
    skip = torch.randn(b, 3, res // 2, res // 2, generator=g) if with_skip else None
    wgt = torch.randn(b, 3, res, res, generator=g)

    xd = K.nchw_to_nhwc(x.to(DEV))
    mod = m.conv.modulation
    s = K.modulate_vec(style.reshape(-1, 512).to(DEV), mod.weight, mod.bias)
    labels = K.mask_labels(mask.to(DEV))[0] if masked else None
    rec = {}
    out = m.run_nhwc(xd, s, labels, r, None if skip is None else skip.to(DEV), rec=rec)
    dx, dws = K.torgb_bwd(wgt.to(DEV), xd, rec["ws"], labels, r)
    ds = m.conv.scale * (dws * m.conv.weight.detach()[0, :, :, 0, 0].unsqueeze(0)).sum(1)
    dstyle = (ds @ mod.weight.detach()) * mod.scale

    f64 = torch.float64
    sd64 = {k: v.to(f64) for k, v in sd.items()}
    xr, sr = x.to(f64).requires_grad_(True), style.to(f64).requires_grad_(True)
    kr = None if skip is None else skip.to(f64).requires_grad_(True)
    outr = orc.to_rgb(sd64, "", xr, sr, mask.to(f64), kr, masked)
    (outr * wgt.to(f64)).sum().backward()
    assert maxabs(out, outr) < 5e-5
    assert maxabs(K.nhwc_to_nchw(dx), xr.grad) < 1e-4 * float(xr.grad.abs().max())
    assert maxabs(dstyle.view_as(sr), sr.grad) < 2e-4 * float(sr.grad.abs().max())
    if with_skip:
        n, c, h, w = wgt.shape
        dsk = K.upfirdn2d_raw(wgt.to(DEV).reshape(n * c, h, w, 1), torch.flip(m.upsample.kernel, [0, 1]), 1, 1, 2, 2,
                              1, 1, 1, 1).view(n, c, h // 2, w // 2)
        assert maxabs(dsk, kr.grad) < 1e-4 * float(kr.grad.abs().max())


@torch.no_grad()
def test_soft_mask_fallback_and_net3_forward():
    """(1) a soft (non one-hot) mask takes the reference's R-pass formulation and still matches the oracle;
    (2) Net3.forward == get_style_vectors -> cal_style_codes -> gen_img (networks.py:85-119)."""
    from e4s_amd.stylegan2 import Generator
    size, K_ = 32, 13
    sd = _gen_sd(size)
    gen = Generator(size, 512, 8, split_layer_idx=5, remaining_layer_idx=K_)
    gen.load_state_dict(sd, strict=True)
    gen = gen.to(DEV).eval()
    g = torch.Generator().manual_seed(60)
    lat = torch.randn(2, 12, gen.n_latent, 512, generator=g) * 0.5
    soft = torch.softmax(torch.randn(2, 12, 64, 64, generator=g) * 3, dim=1)
    noise = synth.synth_noise(size, seed=3, batch=2)
    img, _, feats = gen([lat.to(DEV)], None, soft.to(DEV), input_is_latent=True, noise=[n.to(DEV) for n in noise])
    img_r, feats_r = orc.generator_forward({"G." + k: v for k, v in sd.items()}, lat, soft, noise, size, K_)
    assert maxabs(img, img_r) < 1e-4 and maxabs(feats, feats_r) < 1e-4

    net = _net(256)
    x = synth.synth_image(1, 1024, tag="fwd").to(DEV)
    mask = synth.onehot(synth.synth_labels_face(1, 512, seed=7)).to(DEV)
    imgs, feats16, latent = net(x, mask, randomize_noise=False, return_latents=True)
    sv, _ = net.get_style_vectors(x, mask)
    codes = net.cal_style_codes(sv)
    stored = [getattr(net.G.noises, f"noise_{i}") for i in range(net.G.num_layers)]
    img2, _, feats2 = net.gen_img(None, codes, mask, noise=stored)
    assert torch.equal(imgs, img2) and torch.equal(latent, codes) and torch.equal(feats16, feats2)
    with pytest.raises(NotImplementedError):
        net.get_style_vectors(x, torch.softmax(torch.randn(1, 12, 512, 512, device=DEV), 1))


def test_ops_double_backward_matches_oracle():
    """Second-order path used by the R1 / path-length regularisers (op/fused_act.py:41-47, op/upfirdn2d.py:59-82)."""
    from e4s_amd.op import fused_leaky_relu, upfirdn2d
    g = torch.Generator().manual_seed(70)
    x = torch.randn(2, 4, 8, 8, generator=g)
    b = torch.randn(4, generator=g)
    k = orc.make_blur_kernel() * 4
    w = torch.randn(2, 4, 16, 16, generator=g)

    def second_order(xt, bt, kt, wt, lrelu, up):
        y = up(lrelu(xt, bt), kt)
        (gx,) = torch.autograd.grad((y * wt).sum(), xt, create_graph=True)
        return (gx ** 2).sum() + (y ** 2).sum()

    xd, bd = x.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    ld = second_order(xd, bd, k.to(DEV), w.to(DEV), fused_leaky_relu, lambda t, kk: upfirdn2d(t, kk, up=2, pad=(2, 1)))
    ld.backward()
    xr, br = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lr_ = second_order(xr, br, k, w, orc.fused_leaky_relu, lambda t, kk: orc.upfirdn2d(t, kk, up=2, pad=(2, 1)))
    lr_.backward()
    assert abs(float(ld) - float(lr_)) < 1e-3 * abs(float(lr_))
    assert maxabs(xd.grad, xr.grad) < 1e-4 * float(xr.grad.abs().max())
    assert maxabs(bd.grad, br.grad) < 1e-4 * float(br.grad.abs().max())


@pytest.mark.parametrize("size,K,cells", [(16, 13, 4), (32, 5, 8)])
def test_generator_weight_grads_vs_oracle_f64(size, K, cells):
    """Config 5 (train_G=True): gradients w.r.t. every generator parameter the fused path uses -- conv weights
    (3x3, polyphase up-convs, ToRGB), modulation weights/biases, noise strengths, activation/RGB biases and the
    constant input -- against the oracle's fp64 autograd."""
    from e4s_amd.stylegan2 import Generator
    sd = _gen_sd(size)
    gen = Generator(size, 512, 8, split_layer_idx=5, remaining_layer_idx=K)
    gen.load_state_dict(sd, strict=True)
    gen = gen.to(DEV).eval()
    for n_, p in gen.named_parameters():
        p.requires_grad = not n_.startswith("style.")
    g = torch.Generator().manual_seed(80)
    b = 2
    lat = torch.randn(b, 12, gen.n_latent, 512, generator=g) * 0.5
    mask = synth.onehot(synth.synth_labels_blocks(b, 512, cells, seed=4))
    noise = synth.synth_noise(size, seed=5, batch=b)
    w_img = torch.randn(b, 3, size, size, generator=g)
    img, _, _ = gen([lat.to(DEV)], None, mask.to(DEV), input_is_latent=True, noise=[n.to(DEV) for n in noise])
    (img * w_img.to(DEV)).sum().backward()

    f64 = torch.float64
    sd64 = {"G." + k: v.to(f64).requires_grad_(not k.startswith("style.") and v.is_floating_point()
                                               and not k.endswith("kernel") and not k.startswith("noises."))
            for k, v in sd.items()}
    img_r, _ = orc.generator_forward(sd64, lat.to(f64), mask.to(f64), [n.to(f64) for n in noise], size, K)
    (img_r * w_img.to(f64)).sum().backward()
    checked, bad = 0, []
    for name, p in gen.named_parameters():
        ref = sd64["G." + name].grad
        if name.startswith("style."):
            continue
        if ref is None or float(ref.abs().max()) == 0.0:          # parameter not on the path of this configuration
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, name
        scale = float(ref.abs().max())
        got = p.grad.detach().cpu().double()
        rel_l2 = float((got - ref).norm() / ref.norm())
        # Two error sources, bounded separately.
        # (1) fp32 accumulation through the whole backward chain (atomics make the order vary run to run): measured
        #     <= 3e-4 on most parameters, 6e-4..7e-4 on the deepest ones (conv1, the constant input) at 32^2 -> the
        #     relative L2 error stays under 2e-3.
        # (2) LeakyReLU gate flips: the fp32 forward and the fp64 oracle disagree on sign(y) for the handful of
        #     activations with |y| < ~1e-5 (about one in the 1M of a 32^2 layer).  A flipped element changes that pixel's
        #     contribution by a factor 5, and with only b*H*W = 2048 pixels in the weight-gradient sum one pixel is
        #     worth up to ~1e-2 of max|dW| (tools/debug_wgrad.py: same x and dy -> HIP dW equals fp64 dW to 2e-6,
        #     while fp64 dW from the fp64 forward differs by 4.3e-3 of 0.80 on convs.5.conv.weight).  So the max-abs
        #     bound is looser than the L2 bound, which averages the flips out.
        tol_l2, tol_max = 2e-3, 1e-2
        if ref.numel() == 1:
            # NoiseInjection.weight: one scalar = a sum of ~1e5 signed terms that cancels to ~1e-4 of sum|terms|, so the
            # fp32 round-off of the incoming gradient shows up amplified (measured 1.1e-2 on convs.0.noise.weight)
            tol_l2 = tol_max = 5e-2
        err = maxabs(p.grad, ref)
        if not (rel_l2 < tol_l2 and err < tol_max * scale):
            bad.append((name, rel_l2, err, scale))
        checked += 1
    assert not bad, bad
    assert checked >= 20


@pytest.mark.parametrize("b,h,w,cin,cout,stride,ntaps", [(2, 32, 32, 128, 128, 1, 9), (3, 16, 48, 64, 256, 1, 9), (2, 32, 32, 128, 128, 2, 9),
                                                         (2, 64, 32, 64, 128, 2, 1)])
def test_fused_output_statistics_equal_the_separate_pass(b, h, w, cin, cout, stride, ntaps, monkeypatch):
    """InstanceNorm statistics emitted by the conv epilogues / by the apply pass == e4s_instnorm_stats_f32 on the tensor
    they describe (same fp64 sums, different summation order: 1e-6 relative), and the encoder with them == without."""
    from e4s_amd import kernels as K
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    g = torch.Generator().manual_seed(41)
    x = (torch.randn(b, h, w, cin, generator=g) * 1.3 + 0.4).to(DEV)
    k = 3 if ntaps == 9 else 1
    wp = _pack(torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)).to(DEV)
    ws = K.split_bf16x2(wp)
    y, (st, pooled) = K.conv_mfma(x, wp, cout, istride=stride, ntaps=ntaps, w_split=ws, want_stats=True)
    st_ref, pooled_ref = K.instnorm_stats(y, want_pooled=True)
    assert torch.equal(y, K.conv_mfma(x, wp, cout, istride=stride, ntaps=ntaps, w_split=ws))
    assert maxabs(st, st_ref) < 2e-6 * float(st_ref.abs().max())
    assert maxabs(pooled, pooled_ref) < 1e-6
    gate = torch.rand(b, cout, generator=g).to(DEV)
    res = torch.randn(y.shape, generator=g).to(DEV)
    slope = (torch.rand(cout, generator=g) * 0.4).to(DEV)
    out, st_out = K.instnorm_apply(y, st_ref, gate=gate, res=res, slope=slope, want_stats=True)
    assert torch.equal(out, K.instnorm_apply(y, st_ref, gate=gate, res=res, slope=slope))
    assert maxabs(st_out, K.instnorm_stats(out)[0]) < 2e-6 * float(st_out.abs().max())


@pytest.mark.parametrize("cin,cout,h,w,stride", [(256, 256, 14, 14, 1), (512, 512, 7, 7, 1), (512, 512, 14, 14, 2), (128, 128, 16, 16, 1),
                                                 (512, 64, 8, 8, 1)])
def test_f32_conv_split_k_small_maps(cin, cout, h, w, stride):
    """e4s_conv_mfma_f32 on maps of <= 2 pixel tiles per sample (IR-SE50's 14x14 / 7x7 layers, the generator's 4^2-16^2
    layers): the input channels are split over blockIdx.y and added in order -- same values as the fp64 reference, and a
    sample's result does not depend on the batch it is computed in (the split policy never looks at the batch)."""
    from e4s_amd import kernels as K
    from e4s_amd import lib
    g = torch.Generator().manual_seed(17)
    x = torch.randn(3, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    bias = torch.randn(cout, generator=g)
    ref = F.leaky_relu(F.conv2d(x.double(), wt.double(), bias.double(), stride=stride, padding=1), 0.2) * (2 ** 0.5)
    wp = K.pack_taps(wt.to(DEV))
    xd = K.nchw_to_nhwc(x.to(DEV))
    kw = dict(bias=bias.to(DEV), act=1) if stride == 1 else dict(bias=bias.to(DEV), act=1, istride=2, ntaps=9)
    y3 = K.conv_mfma(xd, wp, cout, **kw)
    assert maxabs(K.nhwc_to_nchw(y3), ref) < 5e-5
    y1 = K.conv_mfma(xd[1:2].contiguous(), wp, cout, **kw)
    assert torch.equal(y1[0], y3[1])
    # the launch really split (otherwise this test pins nothing)
    p = lib.ConvParams()
    p.B, p.Ha, p.Wa, p.Ho, p.Wo, p.Cin, p.Cout, p.ncls, p.ntaps = 3, h // stride, w // stride, h // stride, w // stride, cin, cout, 1, 9
    assert lib.load().e4s_conv_mfma_ws_floats(ctypes.byref(p), 1 if stride == 1 else 0) > 0


@pytest.mark.parametrize("b,h,w,cin,cout,mode", [(2, 32, 32, 512, 512, "in_prelu"), (2, 32, 32, 512, 512, "stats"), (1, 16, 48, 64, 128, "plain"),
                                                 (3, 64, 32, 64, 256, "in_prelu"), (1, 128, 128, 128, 128, "stats"),
                                                 (2, 16, 16, 96, 128, "bias_lrelu"),
                                                 # more tiles than CUs: the persistent blocks walk 2-3 tiles each, across samples
                                                 (3, 256, 256, 64, 128, "in_prelu"), (5, 128, 128, 128, 128, "stats"), (9, 96, 96, 32, 256, "plain"),
                                                 # > 128 tiles of >= 16 chunks: what the policy gives the one-wave-per-SIMD kernel
                                                 (5, 64, 64, 256, 256, "in_prelu"), (5, 64, 64, 256, 256, "stats"), (3, 96, 96, 512, 128, "bias_lrelu")])
@pytest.mark.parametrize("wave_tile", [0, 1, "1w"])
def test_winograd_f23_conv_vs_fp64(b, h, w, cin, cout, mode, wave_tile, monkeypatch):
    """wave_tile: every form of the kernel on every shape (0: a wave owns 64 x 32 of all four positions; 1, round 5: 64 x 64 of two positions,
    one position exchanged between the waves of a pair in the epilogue -- the policy picks it for the 512-channel layers only; "1w", round 6:
    csrc/conv_wino1w.hip, four waves of 64 x 64 x four positions, one per SIMD -- launches without a K split; split launches stay on 0 / 1).
    e4s_conv_wino_bf16x3_f32 (Winograd F(2,3) along the rows, split-bf16 MFMAs) vs F.conv2d in fp64 on the same operands: plain,
    with the InstanceNorm folded into the input transform + PReLU epilogue (the encoder unit's first conv, helpers.py:128-133), with the
    fused output statistics + SE gate (its second conv), with bias + leaky ReLU (the loss networks' convs).  Bound 3e-5 of the output
    scale (measured ~8e-6: 1.7x the direct split-bf16 kernel), statistics 2e-6 relative; bit-reproducible."""
    import torch.nn.functional as F
    from e4s_amd import kernels as K
    if wave_tile == "1w":
        monkeypatch.setenv("E4S_WINO_1W", "1")
    else:
        monkeypatch.setenv("E4S_WINO_1W", "0")
        monkeypatch.setenv("E4S_WINO_WT", str(wave_tile))
    g = torch.Generator().manual_seed(h * 7 + cin)
    x = torch.randn(b, cin, h, w, generator=g) * 1.3 + 0.4
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    xd = K.nchw_to_nhwc(x.to(DEV))
    u = K.wino_weights(K.pack_taps(wt.to(DEV)))
    x64, w64 = x.double(), wt.double()
    kw = {}
    if mode == "in_prelu":
        st, _ = K.instnorm_stats(xd)
        slope = (torch.rand(cout, generator=g) * 0.5).to(DEV)
        kw = dict(in_stats=st, act=2, slope=slope)
        xn = (x64 - x64.mean((2, 3), keepdim=True)) / torch.sqrt(x64.var((2, 3), unbiased=False, keepdim=True) + 1e-5)
        ref = F.conv2d(xn, w64, padding=1)
        ref = torch.where(ref > 0, ref, ref * slope.cpu().double().view(1, -1, 1, 1))
    elif mode == "bias_lrelu":
        bias = torch.randn(cout, generator=g).to(DEV)
        kw = dict(bias=bias, act=1, alpha=0.2, gain=2 ** 0.5)
        ref = F.leaky_relu(F.conv2d(x64, w64, bias.cpu().double(), padding=1), 0.2) * 2 ** 0.5
    else:
        ref = F.conv2d(x64, w64, padding=1)
    if mode == "stats":
        cr = cout // 16
        fc1, fc2 = (torch.randn(cr, cout, generator=g) / cout ** 0.5).to(DEV), (torch.randn(cout, cr, generator=g) / cr ** 0.5).to(DEV)
        y, (stats, gate) = K.conv_wino(xd, u, cout, want_stats=True, se=(fc1, fc2))
        mean, var = ref.mean((2, 3)), ref.var((2, 3), unbiased=False)
        assert maxabs(stats[..., 0], mean) < 3e-5 * float(ref.abs().max())
        assert maxabs(stats[..., 1], 1 / torch.sqrt(var + 1e-5)) < 1e-4 * float((1 / torch.sqrt(var + 1e-5)).max())
        y2, (stats2, pooled) = K.conv_wino(xd, u, cout, want_stats=True)
        assert torch.equal(y, y2) and torch.equal(stats, stats2)
    else:
        y = K.conv_wino(xd, u, cout, **kw)
    err = maxabs(K.nhwc_to_nchw(y), ref) / float(ref.abs().max())
    assert err < 3e-5, err
    assert torch.equal(y, K.conv_wino(xd, u, cout, **kw) if mode != "stats" else y2)


def test_encoder_forward_with_and_without_winograd_vs_oracle(monkeypatch):
    """FSEncoder_PSP at 256^2 on the Winograd F(2,3) kernel (default) and on the direct split-bf16 kernel (E4S_WINO off): both within the
    style-vector bound against the CPU oracle (VERDICT r3 go / no-go: style vectors <= 3e-4)."""
    from e4s_amd import kernels as K
    from e4s_amd.networks import Net3
    from e4s_amd.options import make_opts
    from oracle import e4s_oracle as orc
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    sd = synth.synth_state_dict(256, 13)
    net = Net3(make_opts(out_size=256))
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    img = synth.synth_image(2, 1024, tag="wino_enc")
    mask = synth.onehot(synth.synth_labels_face(2, 512, seed=5))
    with torch.no_grad():
        ref, _ = orc.get_style_vectors({k: v.double() for k, v in sd.items()}, img.double(), mask.double())
        out = {}
        for wino in (True, False):
            monkeypatch.setattr(K, "WINO", wino)
            sv, _ = net.get_style_vectors(img.to(DEV), mask.to(DEV))
            out[wino] = maxabs(sv, ref)
    print("style vectors vs fp64 oracle: winograd %.3e, direct %.3e (scale %.2f)" % (out[True], out[False], float(ref.abs().max())))
    assert out[True] < 3e-4 and out[False] < 3e-4


def test_mapping_network_native_vs_module_chain():
    """Generator.get_latent / mean_latent (model.py:489-497, 570-574: PixelNorm + 8 x EqualLinear(lr_mul 0.01, fused_lrelu)) on the
    native kernels == the reference module chain evaluated in fp64 on the CPU; under autograd (z requires grad) the ATen chain is kept."""
    from e4s_amd.stylegan2 import Generator
    g = Generator(256, 512, 8)
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for lin in list(g.style)[1:]:
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=gen) / 0.01)        # EqualLinear init: randn / lr_mul
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=gen))
    z = torch.randn(5, 512, generator=gen)
    x = (z.double() * torch.rsqrt((z.double() ** 2).mean(1, keepdim=True) + 1e-8))
    for lin in list(g.style)[1:]:
        x = torch.nn.functional.leaky_relu(x @ (lin.weight.double() * lin.scale).t() + lin.bias.double() * lin.lr_mul, 0.2) * 2 ** 0.5
    g = g.to(DEV)
    w = g.get_latent(z.to(DEV))
    assert maxabs(w, x) < 2e-5 * float(x.abs().max()), maxabs(w, x)
    zg = z.to(DEV).requires_grad_(True)
    wg = g.get_latent(zg)                                          # differentiable path: the module chain
    assert wg.requires_grad and maxabs(wg, x) < 1e-4 * float(x.abs().max())
    assert tuple(g.mean_latent(64).shape) == (1, 512)


@pytest.mark.parametrize("b,h,w", [(2, 256, 256), (3, 112, 112), (1, 16, 48)])
def test_tiled_stem_conv_and_its_fused_statistics(b, h, w):
    """e4s_conv3x3_stem_f32 (Cin 3 -> Cout 64 on 16x16 tiles, weights in registers) vs F.conv2d in fp64, its fused InstanceNorm statistics
    vs the separate statistics pass, and == the grid-stride kernel e4s_conv3x3_small_f32 to rounding (same products, another order)."""
    import torch.nn.functional as F
    from e4s_amd import kernels as K
    from e4s_amd import lib
    g = torch.Generator().manual_seed(h + b)
    x = torch.randn(b, 3, h, w, generator=g)
    wt = torch.randn(64, 3, 3, 3, generator=g) * 0.3
    xd = K.nchw_to_nhwc(x.to(DEV))
    y, st = K.conv3x3_small(xd, wt.to(DEV), want_stats=True)
    ref = F.conv2d(x.double(), wt.double(), padding=1)
    assert maxabs(K.nhwc_to_nchw(y), ref) < 2e-6 * float(ref.abs().max())
    st_sep, _ = K.instnorm_stats(y)
    assert maxabs(st[..., 0], st_sep[..., 0]) < 1e-6 and maxabs(st[..., 1], st_sep[..., 1]) < 1e-5 * float(st_sep[..., 1].max())
    assert maxabs(st[..., 0], ref.mean((2, 3))) < 1e-5
    y_old = torch.empty_like(y)
    lib.call("e4s_conv3x3_small_f32", lib.fptr(xd), lib.fptr(wt.to(DEV)), lib.fptr(y_old), b, h, w, 3, 64, lib.stream())
    assert maxabs(y, y_old) < 2e-6 * float(ref.abs().max())
    assert torch.equal(y, K.conv3x3_small(xd, wt.to(DEV)))


@pytest.mark.parametrize("b,h,w,c,masked", [(2, 64, 64, 128, True), (1, 128, 96, 32, False), (2, 16, 16, 512, True), (1, 32, 32, 64, True)])
def test_fused_activation_backward_and_demod_gradient(b, h, w, c, masked):
    """e4s_act_bwd_demod_f32 == e4s_fused_bias_act_f32(grad) followed by e4s_demod_grad_f32 (the two passes it replaces): gz bit for bit,
    dd to summation-order rounding, and dd bit-reproducible."""
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(c + h)
    dy = torch.randn(b, h, w, c, generator=g).to(DEV)
    y = torch.randn(b, h, w, c, generator=g).to(DEV)
    noise = torch.randn(b, 1, h, w, generator=g).to(DEV)
    nw = torch.tensor([0.3], device=DEV)
    bias = torch.randn(c, generator=g).to(DEV)
    labels = None
    if masked:
        labels, _ = K.mask_labels(synth.onehot(synth.synth_labels_face(b, 512, seed=3)).to(DEV))
    gz0 = K.fused_bias_act(dy, None, y, 3, 1, 0.2, 2 ** 0.5)
    dd0 = K.demod_grad(gz0, y, noise, nw, bias, 0.2, 2 ** 0.5, labels, 12)
    gz1, dd1 = K.act_bwd_demod(dy, y, noise, nw, bias, 0.2, 2 ** 0.5, labels, 12)
    assert torch.equal(gz0, gz1)
    assert maxabs(dd0, dd1) < 2e-5 * float(dd0.abs().max()), maxabs(dd0, dd1)
    assert torch.equal(dd1, K.act_bwd_demod(dy, y, noise, nw, bias, 0.2, 2 ** 0.5, labels, 12)[1])


def test_polyphase_fold_is_the_transpose_of_polyphase_weights():
    """e4s_polyphase_fold_f32 (weight gradient of an up-sampling StyledConv: the gradients of the 4 x 9 polyphase kernels folded back onto
    the 3x3 weight) vs the fp64 transpose of stylegan2.polyphase_upconv_weights (the CPU-tested statement of the polyphase map), and the
    adjoint identity <P(w), g> == <w, P^T(g)> against the forward kernel."""
    from e4s_amd import kernels as K
    from e4s_amd.stylegan2 import make_kernel, polyphase_upconv_weights
    g = torch.Generator().manual_seed(21)
    cout, cin = 12, 20
    k4 = make_kernel([1, 3, 3, 1]) * 4
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    deff = torch.randn(4, 9, cout, cin, generator=g, dtype=torch.float64)
    (polyphase_upconv_weights(w, k4.double()) * deff).sum().backward()
    got = K.polyphase_fold(deff.float().to(DEV), k4.to(DEV), cout, cin)
    assert got.shape == (cout, cin, 3, 3)
    assert maxabs(got, w.grad) < 1e-5 * float(w.grad.abs().max())
    pw = K.polyphase_weights(w.detach().float().to(DEV), k4.to(DEV))
    lhs = float((pw.double().cpu() * deff).sum())
    rhs = float((w.detach() * got.double().cpu()).sum())
    assert abs(lhs - rhs) < 1e-4 * max(1.0, abs(lhs))


@pytest.mark.parametrize("cin,cout,res,up,lab", [(128, 64, 32, False, "blocks"), (128, 128, 16, True, "blocks"), (512, 512, 16, False, "face"),
                                                 (256, 128, 32, True, "face"), (128, 64, 24, False, "face")])
def test_masked_styled_conv_dgrad_in_scatter_form_vs_exact_fp32_and_oracle_f64(cin, cout, res, up, lab, monkeypatch):
    """Masked StyledConv (per-pixel region styles, model.py:386-400; plain and polyphase up-conv) under the split-bf16 policy: dL/dx and
    dL/dstyle from the SCATTER form (csrc/dgrad_scatter.hip: e4s_region_scale_f32 -> one 1x1 split-bf16 contraction per phase with the
    nine taps in its columns -> e4s_col2im_region_f32) against the exact-fp32 dx + ds kernel it replaces and the oracle's fp64 autograd.
    'blocks' = one region per 16x16 block of the 512^2 map (every pixel of a 32^2 layer is a boundary pixel), 'face' = the synthetic
    face map; 24^2: partial 256-row tiles.  The gradients are bit-reproducible (ordered dL/ds sums)."""
    from e4s_amd import kernels as K
    from e4s_amd.autograd import styled_conv_backward
    from e4s_amd.stylegan2 import StyledConv
    sd = _styled_sd(cin, cout, up, 31)
    m = StyledConv(cin, cout, 3, 512, upsample=up, mask_op=True)
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(60)
    b, r = 2, 12
    x = torch.randn(b, cin, res, res, generator=g)
    style = torch.randn(b, r, 512, generator=g)
    mask = synth.onehot(synth.synth_labels_blocks(b, 512, 16, seed=7) if lab == "blocks" else synth.synth_labels_face(b, 512, seed=70))
    ores = res * 2 if up else res
    noise = torch.randn(b, 1, ores, ores, generator=g)
    wgt = torch.randn(b, cout, ores, ores, generator=g)
    xd = K.nchw_to_nhwc(x.to(DEV))
    mod = m.conv.modulation
    s = K.modulate_vec(style.reshape(-1, 512).to(DEV), mod.weight, mod.bias)
    labels = K.mask_labels(mask.to(DEV))[0]
    monkeypatch.setattr(K, "PRECISION", "f32")          # ONE exact forward for both backward paths (no activation-kink flips between them)
    rec = {}
    y = m.run_nhwc(xd, s, noise.to(DEV), labels, r, rec=rec)
    rec.update(layer=m, x=xd, y=y, s=s, labels=labels)

    def run(prec):
        monkeypatch.setattr(K, "PRECISION", prec)
        dx, ds = styled_conv_backward(rec, K.nchw_to_nhwc(wgt.to(DEV)), r, {})
        return K.nhwc_to_nchw(dx), (ds @ mod.weight.detach()) * mod.scale, ds

    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    used = K.scatter_dgrad_wanted(b, res, res, cout, cin)
    dx, dstyle, ds = run("bf16x3")
    dx2, _, ds2 = run("bf16x3")
    dx32, dstyle32, _ = run("f32")
    assert torch.equal(dx, dx2) and torch.equal(ds, ds2)
    f64 = torch.float64
    sd64 = {k: v.to(f64) for k, v in sd.items()}
    xr = x.to(f64).requires_grad_(True)
    sr = style.to(f64).requires_grad_(True)
    yr = orc.styled_conv(sd64, "", xr, sr, mask.to(f64), noise.to(f64), up, True)
    (yr * wgt.to(f64)).sum().backward()
    gs, ss = float(xr.grad.abs().max()), float(sr.grad.abs().max())
    assert maxabs(dx32, xr.grad) < 1e-4 * gs
    assert maxabs(dx, xr.grad) < 1e-4 * gs, ("scatter-form dgrad", used, maxabs(dx, xr.grad), gs)
    assert maxabs(dstyle.view_as(sr), sr.grad) < 3e-4 * ss and maxabs(dstyle, dstyle32) < 3e-4 * ss
    assert used and 0 < maxabs(dx, dx32)                # really another kernel, the same gradient
