"""The launches that used to leave the chip mostly idle (csrc/conv_bf16x3.hip):

* masked StyledConv contractions on 4^2 / 8^2 maps -- several whole images per 256-row tile of the region-select kernel (path 3,
  csrc/few_tile_geom.h) with a K split down to one 32-channel chunk per block;
* deep stride-2 3x3 convs of few tiles -- the gather kernel with its input channels split over blocks (raw slabs + the ordered second stage).

Bounds: 1e-4 of the output's max-abs against exact fp32 / fp64 (the split-bf16 error model of test_conv_bf16x3_vs_conv2d_f64), 5e-6 against
the unpacked path (same products, another summation order: the bound of test_region_rows_kernel_vs_fp32_and_region_select).  Outputs and
workspaces are allocated between sentinel bands (tests/guarded_alloc.py).  The unpacked path exists only with E4S_REGION_PACK=0, which the
library reads once: one child process computes all its outputs."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from e4s_amd import synth
from guarded_alloc import DEV, _GuardedTorch, unwritten
from oracle import e4s_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (b, h, w, cin, cout, up, labels, R)
PACKED = [(8, 4, 4, 128, 128, False, "face", 12),      # the workload's own layer shape at reduced channels
          (9, 4, 4, 64, 128, False, "noise", 12),      # exactly one full tile
          (10, 4, 4, 64, 256, True, "noise", 12),      # second tile holds one image
          (3, 8, 8, 128, 128, False, "blocks", 16),    # one full tile, 16 regions
          (4, 8, 8, 64, 128, True, "face", 12),        # second tile holds one image, polyphase
          (5, 4, 8, 64, 128, False, "noise", 12),      # rectangular map
          (2, 5, 7, 32, 128, True, "blocks", 12),      # odd sizes
          (1, 8, 8, 512, 512, False, "face", 12)]      # one image, deepest K split


def maxabs(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


@pytest.fixture
def guard(monkeypatch):
    from e4s_amd import kernels as K
    g = _GuardedTorch()
    monkeypatch.setattr(K, "torch", g)
    return g


def _labels(b, ho, wo, kind, R, g, seed):
    if kind == "face":                      # 512^2 face-like map, legacy-nearest lookup inside the kernel
        return synth.synth_labels_face(b, 512, seed=seed).view(b, 512, 512).to(torch.uint8).contiguous()
    if kind == "blocks":                    # 2x2-pixel blocks at output resolution: boundaries inside every image
        return torch.randint(0, R, (b, (ho + 1) // 2, (wo + 1) // 2), generator=g).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :ho, :wo].to(torch.uint8).contiguous()
    return torch.randint(0, R, (b, ho, wo), generator=g).to(torch.uint8)        # "noise": per-pixel random regions


def _packed_case(case, seed=41):
    """CPU tensors of a masked contraction (the same in the child process): x, tap-packed weights, keyword operands of K.conv_mfma."""
    b, h, w, cin, cout, up, kind, R = case
    g = torch.Generator().manual_seed(seed)
    ncls = 4 if up else 1
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    x = torch.randn(b, h, w, cin, generator=g)
    wt = torch.randn(ncls, 9, cout, cin, generator=g) / math.sqrt(cin * 9)
    kw = dict(labels=_labels(b, ho, wo, kind, R, g, seed), num_regions=R, ncls=ncls, ostride=2 if up else 1,
              in_scale=torch.rand(b * R, cin, generator=g) + 0.5, out_scale=torch.rand(b * R, cout, generator=g) + 0.5,
              noise=torch.randn(b, 1, ho, wo, generator=g), noise_w=torch.tensor([0.2]), bias=torch.randn(cout, generator=g) * 0.1, act=1)
    return x, wt, kw


def _dev(kw):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}


def _dump_unpacked(path):
    """Child process (E4S_REGION_PACK=0): every PACKED case on the routing the small maps had before, with the path it took."""
    from e4s_amd import kernels as K
    out = []
    for case in PACKED:
        x, wt, kw = _packed_case(case)
        x, wt, kw = x.to(DEV), wt.to(DEV), _dev(kw)
        y = K.conv_mfma(x, wt, case[4], w_split=K.split_bf16x2(wt), w_split16=K.split16_bf16x2(wt), **kw)
        out.append((y.cpu(), K.LAST_REGION_PATH, K.REGION_PACK))
    torch.save(out, path)


@pytest.fixture(scope="module")
def unpacked(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("few_tile") / "unpacked.pt")
    env = dict(os.environ, E4S_REGION_PACK="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, "-c", f"import test_gpu_few_tile_launches as t; t._dump_unpacked({path!r})"], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-4000:]
    return torch.load(path, map_location="cpu", weights_only=False)


@pytest.mark.parametrize("ci", range(len(PACKED)), ids=[f"b{c[0]}-{c[1]}x{c[2]}-{c[3]}to{c[4]}{'-up' if c[5] else ''}-{c[6]}" for c in PACKED])
def test_packed_masked_conv(ci, unpacked, guard):
    """A masked contraction on a map that packs: path 3 (not with the switch off), == the exact fp32 region kernel to 1e-4 and == the unpacked
    routing to 5e-6 of the output's max-abs, every output element written and nothing beside it, bit-reproducible, the same launch with and
    without the 16-channel weight image, no sample's output depends on its tile neighbours, and a captured launch follows the label buffer."""
    from e4s_amd import kernels as K
    case = PACKED[ci]
    b, h, w, cin, cout, up, kind, R = case
    x, wt, kw = _packed_case(case)
    x, wt, kw = x.to(DEV), wt.to(DEV), _dev(kw)
    ws, ws16 = K.split_bf16x2(wt), K.split16_bf16x2(wt)
    guard.check()

    def run(x=x, kw=kw, w16=True):
        return K.conv_mfma(x, wt, cout, w_split=ws, w_split16=ws16 if w16 else None, **kw)

    y = run()
    assert K.LAST_REGION_PATH == 3 if K.REGION_PACK else K.LAST_REGION_PATH in (1, 2)
    y_off, path_off, pack_off = unpacked[ci]
    assert not pack_off and path_off in (1, 2)                           # not 3 with the switch off
    assert unwritten(y) == 0
    guard.check()                                                        # nothing written beside the output or the slabs
    assert torch.equal(y, run())                                         # two calls are bit-equal
    assert torch.equal(y, run(w16=False))                                # the same launch whether or not the 16-channel image is given
    ref = K.conv_mfma(x, wt, cout, **kw)                                 # exact fp32 region kernel
    scale = float(ref.abs().max())
    err32, err_off = maxabs(y, ref), maxabs(y, y_off)
    print(f"\n[few-tile] {case}: vs fp32 {err32 / scale:.3e}, vs unpacked {err_off / scale:.3e} of max-abs {scale:.3f}")
    assert 0 < err32 < 1e-4 * scale
    assert err_off < 5e-6 * scale
    guard.check()

    # nothing leaks between the images of a tile: another x, label map and styles for every OTHER sample leave sample i bit-equal
    x2, _, kw2 = _packed_case(case, seed=43)
    x2, kw2 = x2.to(DEV), dict(_dev(kw2), bias=kw["bias"])               # (the bias belongs to the layer, not to a sample)
    for i in range(b):
        xi, kwi = x2.clone(), dict(kw2)
        xi[i] = x[i]
        for k in ("labels", "noise"):
            kwi[k] = kw2[k].clone()
            kwi[k][i] = kw[k][i]
        for k in ("in_scale", "out_scale"):
            kwi[k] = kw2[k].clone()
            kwi[k][i * R:(i + 1) * R] = kw[k][i * R:(i + 1) * R]
        yi = run(x=xi, kw=kwi)
        assert torch.equal(yi[i], y[i]), i
        if b > 1:
            assert not torch.equal(yi, y)
    guard.check()

    # the tiles are cut from the label map inside the launch: a captured launch replayed on other labels == the eager launch on them
    lab = kw["labels"].clone()
    kwg = dict(kw, labels=lab)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run(kw=kwg)
    torch.cuda.current_stream().wait_stream(st)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        yg = run(kw=kwg)
    lab.copy_(kw2["labels"])
    gr.replay()
    torch.cuda.synchronize()
    want = run(kw=kwg)
    assert torch.equal(yg, want) and not torch.equal(want, y)
    guard.check()


def _styled_sd(cin, cout, up, seed):
    spec = [("conv.weight", (1, cout, cin, 3, 3), "randn"), ("conv.modulation.weight", (cin, 512), "randn"),
            ("conv.modulation.bias", (cin,), "modbias"), ("noise.weight", (1,), "noisew"), ("activate.bias", (cout,), "bias")]
    sd = {k: synth.synth_tensor(k, s, kind, seed) for k, s, kind in spec}
    if up:
        sd["conv.blur.kernel"] = orc.make_blur_kernel() * 4
    return sd


@pytest.mark.parametrize("res,up", [(4, False), (8, True)])
def test_styled_conv_batch8_auto_takes_the_packed_tiles(res, up, monkeypatch):
    """The generator's 512 -> 512 masked StyledConv at 4^2 and 8^2 -> 16^2, batch 8, under the default precision policy: path 3, == the
    reference's 12 passes x one-hot mask to 1e-4 of the output scale."""
    from e4s_amd import kernels as K
    from e4s_amd.stylegan2 import StyledConv
    monkeypatch.setattr(K, "PRECISION", "auto")
    monkeypatch.setattr(K, "LAST_REGION_PATH", 0)
    b = 8
    sd = _styled_sd(512, 512, up, 12)
    m = StyledConv(512, 512, 3, 512, upsample=up, mask_op=True)
    m.load_state_dict(sd)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(b, 512, res, res, generator=g)
    style = torch.randn(b, 12, 512, generator=g)
    mask = synth.onehot(synth.synth_labels_blocks(b, 512, 64, seed=7))
    out_res = res * 2 if up else res
    noise = torch.randn(b, 1, out_res, out_res, generator=g)
    want = orc.styled_conv(sd, "", x, style, mask, noise, up, True)
    got = m(x.to(DEV), style.to(DEV), mask.to(DEV), noise=noise.to(DEV))
    assert K.LAST_REGION_PATH == (3 if K.REGION_PACK else 1)
    scale = float(want.abs().max())
    print(f"\n[few-tile] StyledConv {res}^2 up={up}: {maxabs(got, want) / scale:.3e} of max-abs {scale:.3f}")
    assert maxabs(got, want) < 1e-4 * scale


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b, h, w, cin, cout): stride 2, 3x3
GATHER = [(1, 16, 16, 256, 128),       # smallest split launch
          (2, 12, 20, 256, 128),       # 60 outputs per image: a tile straddles samples
          (1, 8, 8, 512, 64),          # half-used column tile
          (2, 32, 32, 512, 512)]       # the encoder layer's channels at batch 2


def _pack(w):
    cout, cin, kh, kw = w.shape
    return w.permute(2, 3, 0, 1).reshape(1, kh * kw, cout, cin).contiguous()


@pytest.mark.parametrize("b,h,w,cin,cout", GATHER)
def test_split_gather_conv(b, h, w, cin, cout, guard):
    """A stride-2 3x3 conv the gather kernel splits over its input channels: the workspace is asked for and fully written, == fp64 conv2d to
    1e-4 of the output's max-abs with and without bias + PReLU, bit-reproducible, and with want_stats + se the statistics and the gate are
    those of instnorm_stats / se_gate on the returned y, bit for bit."""
    from e4s_amd import kernels as K, lib
    g = torch.Generator().manual_seed(35)
    x = torch.randn(b, cin, h, w, generator=g, dtype=torch.float64) * 1.1 - 0.1
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / math.sqrt(cin * 9)
    bias = torch.randn(cout, generator=g) * 0.1
    slope = torch.rand(cout, generator=g) * 0.5
    wp = _pack(wt.float()).to(DEV)
    xd = K.nchw_to_nhwc(x.float().to(DEV))
    ws = K.split_bf16x2(wp)
    guard.check()

    p = lib.ConvParams()
    ctypes.memset(ctypes.byref(p), 0, ctypes.sizeof(p))
    p.B, p.Ha, p.Wa, p.Hi, p.Wi, p.Ho, p.Wo, p.Cin, p.Cout = b, h // 2, w // 2, h, w, h // 2, w // 2, cin, cout
    p.istride, p.ostride, p.ntaps, p.ncls, p.groups_per_batch = 2, 1, 9, 1, 1
    nws = lib.load().e4s_conv_bf16x3_ws_floats(ctypes.byref(p))
    assert nws > 0 and nws % (b * (h // 2) * (w // 2) * cout) == 0      # the split really runs

    want = F.conv2d(x.float().double(), wt.float().double(), stride=2, padding=1)
    scale = float(want.abs().max())
    y = K.conv_mfma(xd, wp, cout, istride=2, ntaps=9, w_split=ws)
    assert tuple(y.shape) == (b, h // 2, w // 2, cout) and unwritten(y) == 0
    slabs = [t for t in guard.insides(torch.float32) if t.numel() == nws]
    assert len(slabs) == 1 and unwritten(slabs[0]) == 0                  # every slab element written before the second stage read it
    guard.check()
    err = maxabs(K.nhwc_to_nchw(y), want)
    print(f"\n[few-tile] gather {(b, h, w, cin, cout)}: {err / scale:.3e} of max-abs {scale:.3f}")
    assert err < 1e-4 * scale
    assert 0 < maxabs(y, K.conv_mfma(xd, wp, cout, istride=2, ntaps=9))  # (the exact fp32 gather kernel differs)
    assert torch.equal(y, K.conv_mfma(xd, wp, cout, istride=2, ntaps=9, w_split=ws))

    # bias + PReLU in the second stage
    ya = K.conv_mfma(xd, wp, cout, istride=2, ntaps=9, w_split=ws, bias=bias.to(DEV), slope=slope.to(DEV), act=2)
    wa = F.prelu(want + bias.double()[None, :, None, None], slope.double())
    assert unwritten(ya) == 0
    assert maxabs(K.nhwc_to_nchw(ya), wa) < 1e-4 * float(wa.abs().max())

    # a split launch emits no epilogue statistics: they are those of the separate pass over y, and the gate is se_gate on them
    cr = max(cout // 16, 1)
    fc1 = (torch.randn(cr, cout, generator=g) * 50).to(DEV)
    fc2 = (torch.randn(cout, cr, generator=g) * 1e6).to(DEV)
    ys, (stats, gate) = K.conv_mfma(xd, wp, cout, istride=2, ntaps=9, w_split=ws, want_stats=True, se=(fc1, fc2))
    assert torch.equal(ys, y)
    stats2, pooled = K.instnorm_stats(ys, want_pooled=True)
    assert torch.equal(stats, stats2) and torch.equal(gate, K.se_gate(pooled, fc1, fc2))
    guard.check()


def test_encoder_unit_512_stride2_split_vs_oracle(monkeypatch):
    """bottleneck_IR_SE_Ours(512, 512, 2) at 32^2, batch 2, split-bf16: its stride-2 conv is 8 tiles x 8 K splits."""
    from e4s_amd import kernels as K
    from e4s_amd.encoders import bottleneck_IR_SE_Ours
    monkeypatch.setattr(K, "PRECISION", "bf16x3")
    cin = depth = 512
    spec = [("res_layer.1.weight", (depth, cin, 3, 3), "conv"), ("res_layer.2.weight", (depth,), "prelu"),
            ("res_layer.3.weight", (depth, depth, 3, 3), "conv"), ("res_layer.5.fc1.weight", (depth // 16, depth, 1, 1), "conv"),
            ("res_layer.5.fc2.weight", (depth, depth // 16, 1, 1), "conv")]
    sd = {k: synth.synth_tensor(k, s, kind, 5) for k, s, kind in spec}
    m = bottleneck_IR_SE_Ours(cin, depth, 2)
    m.load_state_dict(sd)
    m = m.to(DEV)
    x = torch.randn(2, cin, 32, 32, generator=torch.Generator().manual_seed(10)) * 1.7 + 0.3
    want = orc.encoder_unit(sd, "", x, cin, depth, 2)
    assert K.gather_split(8, 512, 9) == 8
    got = m(x.to(DEV))
    scale = float(want.abs().max())
    print(f"\n[few-tile] encoder unit: {maxabs(got, want) / scale:.3e} of max-abs {scale:.3f}")
    assert maxabs(got, want) < 1e-4 * scale
