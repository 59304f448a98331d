"""The one-wave-per-SIMD strided gather conv (csrc/conv_gather1w.hip) against the 8-wave kernel it replaces where a launch is eligible.

Every case runs the same call twice in one process -- E4S_GATHER_1W=0 (the library reads it per launch) and the default -- and asserts that the
conv outputs are the same bits and that the default call really took the new kernel (K.LAST_GATHER_PATH, the library's own answer).  The shapes
are the smallest at which the re-cut can go wrong: a single stage per tap, two column tiles, 1x1, tiles that straddle samples and end in a
partial tile, the padding-0 geometry, a K split, the fused statistics; and the launches that must stay on the 8-wave kernel."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import enc_fwd_cases as ef
from guarded_alloc import _GuardedTorch, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture
def guard(monkeypatch):
    from e4s_amd import kernels as K
    g = _GuardedTorch()
    monkeypatch.setattr(K, "torch", g)
    return g


def _pack(w):
    cout, cin, kh, kw = w.shape
    return w.permute(2, 3, 0, 1).reshape(1, kh * kw, cout, cin).contiguous()


def _operands(b, h, w, cin, cout, k, seed):
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, cin, h, w, generator=g) * 1.1 - 0.1
    wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    wp = _pack(wt).to(DEV)
    return x, wt, K.nchw_to_nhwc(x.to(DEV)), wp, K.split_bf16x2(wp), K.gather_frag_bf16x2(wp)


def _both(monkeypatch, call, expect_new=True):
    """call() on the 8-wave kernel, then by default: (old result, new result); the paths are the library's own answers"""
    from e4s_amd import kernels as K
    monkeypatch.setenv("E4S_GATHER_1W", "0")
    old = call()
    assert K.LAST_GATHER_PATH == 1
    monkeypatch.delenv("E4S_GATHER_1W")
    new = call()
    assert K.LAST_GATHER_PATH == (2 if expect_new else 1)
    return old, new


# (b, h, w, cin, cout, ntaps): stride 2, padding 1 (3x3) / 0 (1x1)
PLAIN = [(1, 32, 32, 32, 128, 9),        # one full tile, a single stage per tap
         (1, 32, 32, 64, 256, 9),        # two column tiles, two chunks
         (1, 32, 32, 64, 256, 1)]        # the 1x1 shortcut: two stages in all


@pytest.mark.parametrize("b,h,w,cin,cout,ntaps", PLAIN)
def test_same_bits_as_8wave(b, h, w, cin, cout, ntaps, monkeypatch):
    from e4s_amd import kernels as K
    k = 3 if ntaps == 9 else 1
    x, wt, xd, wp, ws, wf = _operands(b, h, w, cin, cout, k, 7)
    old, new = _both(monkeypatch, lambda: K.conv_mfma(xd, wp, cout, istride=2, ntaps=ntaps, w_split=ws, w_frag=wf))
    assert torch.equal(old, new)
    want = F.conv2d(x.double(), wt.double(), stride=2, padding=k // 2)
    assert float((K.nhwc_to_nchw(new).cpu().double() - want).abs().max()) < 1e-4 * float(want.abs().max())
    # bias + PReLU in the epilogue
    g = torch.Generator().manual_seed(8)
    bias, slope = (torch.randn(cout, generator=g) * 0.1).to(DEV), (torch.rand(cout, generator=g) * 0.5).to(DEV)
    old, new = _both(monkeypatch, lambda: K.conv_mfma(xd, wp, cout, istride=2, ntaps=ntaps, w_split=ws, w_frag=wf, bias=bias, slope=slope, act=2))
    assert torch.equal(old, new)


def test_straddling_and_partial_tiles(monkeypatch, guard):
    """B = 3, 24 x 40 -> 12 x 20: 720 pixels = two full tiles and one of 208, tiles straddle the samples; into guarded buffers"""
    from e4s_amd import kernels as K
    b, h, w, cin, cout = 3, 24, 40, 64, 128
    x, wt, xd, wp, ws, wf = _operands(b, h, w, cin, cout, 3, 9)
    guard.check()
    old, new = _both(monkeypatch, lambda: K.conv_mfma(xd, wp, cout, istride=2, ntaps=9, w_split=ws, w_frag=wf))
    assert unwritten(new) == 0
    guard.check()                        # nothing written next to y
    assert torch.equal(old, new)
    alone = K.conv_mfma(xd[1:2].contiguous(), wp, cout, istride=2, ntaps=9, w_split=ws, w_frag=wf)
    assert K.LAST_GATHER_PATH == 2
    assert torch.equal(new[1, 0], alone[0, 0]) and torch.equal(new[1], alone[0])


def test_padding0_convlayer_geometry(monkeypatch):
    """Blur + stride-2 padding-0 3x3 conv (ConvLayer): anchors, tap_shift = 1, 35 x 35 -> 17 x 17 (289 pixels: a partial second tile)"""
    from e4s_amd import kernels as K
    x, wt, xd, wp, ws, wf = _operands(1, 35, 35, 32, 128, 3, 10)
    bias = (torch.randn(128, generator=torch.Generator().manual_seed(11)) * 0.1).to(DEV)
    kw = dict(istride=2, ntaps=9, anchors=(17, 17), tap_shift=1, bias=bias, act=1, alpha=0.2, gain=math.sqrt(2))
    old, new = _both(monkeypatch, lambda: K.conv_mfma(xd, wp, 128, w_split=ws, w_frag=wf, **kw))
    assert torch.equal(old, new)
    want = F.leaky_relu(F.conv2d(x.double(), wt.double(), bias.cpu().double(), stride=2), 0.2) * math.sqrt(2)
    assert float((K.nhwc_to_nchw(new).cpu().double() - want).abs().max()) < 1e-4 * float(want.abs().max())


def test_k_split(monkeypatch, guard):
    """B = 1, Cin 256, 32 x 32 -> 16 x 16, Cout 128: one tile split over its input channels; raw slabs + the second stage with bias and PReLU"""
    from e4s_amd import kernels as K
    if K.gather_split(1, 256, 9) <= 1:
        pytest.skip("gather_split does not split one tile of Cin 256")
    x, wt, xd, wp, ws, wf = _operands(1, 32, 32, 256, 128, 3, 12)
    g = torch.Generator().manual_seed(13)
    bias, slope = (torch.randn(128, generator=g) * 0.1).to(DEV), (torch.rand(128, generator=g) * 0.5).to(DEV)
    guard.check()
    old, new = _both(monkeypatch, lambda: K.conv_mfma(xd, wp, 128, istride=2, ntaps=9, w_split=ws, w_frag=wf, bias=bias, slope=slope, act=2))
    slabs = [t for t in guard.insides(torch.float32) if t.numel() > new.numel()]
    assert len(slabs) == 2 and all(unwritten(t) == 0 for t in slabs)       # the split really ran, both times, and filled its slabs
    guard.check()
    assert unwritten(new) == 0 and torch.equal(old, new)
    want = F.prelu(F.conv2d(x.double(), wt.double(), bias.cpu().double(), stride=2, padding=1), slope.cpu().double())
    assert float((K.nhwc_to_nchw(new).cpu().double() - want).abs().max()) < 1e-4 * float(want.abs().max())


def test_fused_statistics_and_gate(monkeypatch):
    """B = 2, 32 x 32 -> 16 x 16, Cin 64, Cout 128 with want_stats + se: the output is the same bits; a statistics slot adds two wave rows
    where the 8-wave kernel adds four, an fp64 re-association (~1e-13 relative), so (mean, rstd) may cross one float rounding boundary"""
    from e4s_amd import kernels as K
    x, wt, xd, wp, ws, wf = _operands(2, 32, 32, 64, 128, 3, 14)
    g = torch.Generator().manual_seed(15)
    fc1, fc2 = (torch.randn(8, 128, generator=g) * 0.3).to(DEV), (torch.randn(128, 8, generator=g) * 0.3).to(DEV)
    (yo, (so, go)), (yn, (sn, gn)) = _both(
        monkeypatch, lambda: K.conv_mfma(xd, wp, 128, istride=2, ntaps=9, w_split=ws, w_frag=wf, want_stats=True, se=(fc1, fc2)))
    assert torch.equal(yo, yn)
    assert bool(((so == sn) | (torch.nextafter(so, sn) == sn)).all())          # within one float ulp
    r = ef.stats_ref(yn.cpu())                                                 # fp64, from the kernel's own output
    for name, s in (("8-wave", so), ("1-wave", sn)):
        s = s.cpu().double()
        assert bool(((s[..., 0] - r["mean"]).abs() <= r["mean_bound_sum"]).all()), name + " mean"
        assert bool(((s[..., 1] - r["rstd"]).abs() <= r["rstd_bound"]).all()), name + " rstd"
    dev = float((go - gn).abs().max())
    print(f"\n[gather1w] gate deviation from the 8-wave kernel: {dev:.3e}; statistics differing: {int((so != sn).sum())} of {so.numel()}")
    assert dev <= 1e-6


def test_stays_on_8wave(monkeypatch):
    """Cout = 64 (the half-used tile) and a launch without the image keep the 8-wave kernel"""
    from e4s_amd import kernels as K
    x, wt, xd, wp, ws, wf = _operands(1, 32, 32, 32, 64, 3, 16)
    old, new = _both(monkeypatch, lambda: K.conv_mfma(xd, wp, 64, istride=2, ntaps=9, w_split=ws, w_frag=wf), expect_new=False)
    assert torch.equal(old, new)
    x, wt, xd, wp, ws, wf = _operands(1, 32, 32, 32, 128, 3, 17)
    old, new = _both(monkeypatch, lambda: K.conv_mfma(xd, wp, 128, istride=2, ntaps=9, w_split=ws), expect_new=False)
    assert torch.equal(old, new)
    assert os.environ.get("E4S_GATHER_1W") is None
