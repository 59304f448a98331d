"""The swap step's small kernels (regional means, LocalMLP layers, style prologue, the ToRGB tails, the mask's label map)
against fp64 torch statements of what they compute, at the shapes the step runs them at and at odd ones.

Bounds.  Every kernel here accumulates in fp32 (unit roundoff u = 2^-24 = 6e-8).  A sum of n products added in any order
is within n u sum|terms| of the exact one and, for the roughly pairwise orders these kernels use (per-lane partial sums,
then a butterfly), typically within a few sqrt(n) u of the result's scale: for n <= 4096 that is < 4e-6 of the scale.
The bounds below are 2e-5 of the largest expected magnitude (five times that estimate, the factor
test_fused_activation_backward_and_demod_gradient uses), 1e-5 absolute for the regional means of unit-variance features
(test_region_mean_exact_zero_for_empty_regions's) and 5e-5 absolute for the ToRGB outputs (test_torgb_vs_oracle's).
Each result must also be the same bits on a second call and from a captured graph's replay."""
import math

import pytest
import torch

from e4s_amd import synth
from oracle import e4s_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def maxabs(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def twice_and_replayed(fn):
    """fn() -> tensor.  The eager result, after asserting that a second eager call and a captured replay give its bits."""
    first = fn()
    second = fn()
    torch.cuda.synchronize()
    assert torch.equal(first, second)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = fn()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, captured)
    return first


def nearest_labels(lab, h, w):
    """labels [B,1,Hm,Wm] int64 -> [B,h,w] by legacy 'nearest' (F.interpolate(mask, mode='nearest')): source index
    min(floor(dst * float(in) / float(out)), in - 1), in fp32 as ATen computes it."""
    def src(n_in, n_out):
        scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
        return (torch.arange(n_out, dtype=torch.float32) * scale).floor().long().clamp(max=n_in - 1)
    return lab[:, 0][:, src(lab.shape[2], h)][:, :, src(lab.shape[3], w)]


# ---- item 2: regional means -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,res", [(256, 64), (512, 32), (512, 16), (64, 24)])
def test_region_mean_vs_fp64_with_empty_regions(c, res):
    from e4s_amd import kernels as K
    b, r = 3, 12
    g = torch.Generator().manual_seed(100 + res)
    feats = torch.randn(b, res, res, c, generator=g)                      # NHWC
    lab = synth.synth_labels_face(b, 512, seed=7)
    lab[lab == 9] = 1                                                     # region 9 empty in every sample
    lab[0][lab[0] == 4] = 2                                               # and region 4 in sample 0
    small = nearest_labels(lab, res, res)
    want = torch.zeros(b, r, c, dtype=torch.float64)
    for i in range(b):
        for j in range(r):
            sel = small[i] == j
            if int(sel.sum()) > 0:
                want[i, j] = feats[i].double()[sel].mean(0)
    labels, _ = K.mask_labels(synth.onehot(lab).to(DEV))
    fd = feats.to(DEV)

    def run():
        out = torch.full((b, r, c + 64), 7.0, device=DEV)                 # means land at a column offset of a wider row
        K.region_mean_into(fd, labels, out, r, 64)
        return out

    got = twice_and_replayed(run)
    assert float((got[:, :, :64] - 7.0).abs().max()) == 0.0               # columns outside [off, off + C) untouched
    print("region_mean", c, res, maxabs(got[:, :, 64:], want))
    assert maxabs(got[:, :, 64:], want) < 1e-5
    assert float(got[:, 9, 64:].abs().max()) == 0.0 and float(got[0, 4, 64:].abs().max()) == 0.0
    # a sample's means do not depend on the batch it is in
    one = torch.zeros(1, r, c + 64, device=DEV)
    K.region_mean_into(fd[1:2].contiguous(), labels[1:2].contiguous(), one, r, 64)
    assert torch.equal(one[0, :, 64:], got[1, :, 64:])


# ---- item 3: style prologue --------------------------------------------------------------------------------------------
def test_style_prologue_s_and_d_of_every_generator_layer_vs_fp64():
    """One e4s_rowdot_multi_f32 launch per pass over the modulation (512 -> Cin) and demodulation (Cin -> Cout) jobs of
    every styled layer of a 1024^2 generator: masked layers with G = B * 12 rows, the others with G = B."""
    from e4s_amd import kernels as K
    b, r, nlat = 2, 12, 18
    g = torch.Generator().manual_seed(31)
    lat = torch.randn(b, r, nlat, 512, generator=g)
    chans = {4: 512, 8: 512, 16: 512, 32: 512, 64: 512, 128: 256, 256: 128, 512: 64, 1024: 32}
    layers = [(512, 512, 0, True), (512, None, 1, True)]                  # (cin, cout or None for ToRGB, latent index, masked)
    idx, cin = 1, 512
    for res in (8, 16, 32, 64, 128, 256, 512, 1024):
        cout = chans[res]
        masked = res <= 128
        layers += [(cin, cout, idx, masked), (cout, cout, idx + 1, masked), (cout, None, idx + 2, masked)]
        idx += 2
        cin = cout
    sjobs, djobs, keep, want_s, want_d = [], [], [], [], []
    s_off = d_off = 0
    latd = lat.double()
    for cin, cout, li, masked in layers:
        mw = torch.randn(cin, 512, generator=g)
        mb = torch.randn(cin, generator=g) * 0.1 + 1.0
        gn = b * r if masked else b
        stride = nlat * 512 if masked else r * nlat * 512
        mwd, mbd = mw.to(DEV), mb.to(DEV)
        keep += [mwd, mbd]
        sjobs.append(dict(in_off=li * 512, in_stride=stride, out_off=s_off, M=mwd, bias=mbd, G=gn, O=cin, K=512,
                          scale=1.0 / math.sqrt(512)))
        style = latd[:, :, li].reshape(b * r, 512) if masked else latd[:, 0, li]
        s64 = style @ mw.double().t() / math.sqrt(512) + mb.double()
        want_s.append((s_off, s64))
        if cout is not None:
            wsq = torch.rand(cout, cin, generator=g) * 9.0                # sum over the 3 x 3 taps of W^2
            scale = 1.0 / math.sqrt(cin * 9)
            wd = wsq.to(DEV)
            keep.append(wd)
            djobs.append(dict(in_off=s_off, in_stride=cin, out_off=d_off, M=wd, bias=None, G=gn, O=cout, K=cin, scale=scale))
            want_d.append((d_off, s_off, gn, cin, wsq.double(), scale))
            d_off += gn * cout
        s_off += gn * cin
    st, dt = K.rowdot_jobs(sjobs, DEV), K.rowdot_jobs(djobs, DEV)
    ld = lat.to(DEV)

    def run():
        sbuf = torch.empty(s_off, device=DEV)
        dbuf = torch.empty(d_off, device=DEV)
        K.rowdot_multi(*st, ld, sbuf, 0)
        K.rowdot_multi(*dt, sbuf, dbuf, 1)
        return torch.cat([sbuf, dbuf])

    got = twice_and_replayed(run).cpu()
    sbuf, dbuf = got[:s_off], got[s_off:]
    for off, s64 in want_s:
        have = sbuf[off:off + s64.numel()].view_as(s64)
        assert maxabs(have, s64) < 2e-5 * float(s64.abs().max()), (off, maxabs(have, s64))
    for off, so, gn, cin, wsq, scale in want_d:
        s32 = sbuf[so:so + gn * cin].view(gn, cin).double()               # d of the s the kernel produced
        d64 = scale / torch.sqrt(scale * scale * (s32 * s32) @ wsq.t() + 1e-8)
        have = dbuf[off:off + d64.numel()].view_as(d64)
        assert maxabs(have, d64) < 2e-5 * float(d64.abs().max()), (off, maxabs(have, d64))


# ---- item 4: LocalMLP layers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 8, 11])
@pytest.mark.parametrize("r,k,o", [(12, 512, 416), (12, 1280, 512), (3, 1024, 2048), (1, 512, 512), (2, 1280, 100)])
def test_grouped_linear_small_k_vs_fp64(b, r, k, o):
    """(12, 512, 416) / (12, 1280, 512): the LocalMLP's two layers (the second narrowed from 6656 rows: same kernel, the
    rows of a region are independent); (3, 1024, 2048): the middle K range; the last two stay on the one-row kernel."""
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(k + o + b)
    x = torch.randn(b, r, k, generator=g)
    w = torch.randn(r, o, k, generator=g)
    bias = torch.randn(r, o, generator=g)
    add = torch.randn(o, generator=g)
    scale = 1.0 / math.sqrt(k)
    xd, wd, bd, ad = x.to(DEV), w.to(DEV), bias.to(DEV), add.to(DEV)
    pre = torch.einsum("brk,rok->bro", x.double(), w.double()) * scale + bias.double()
    want_act = torch.where(pre > 0, pre, pre * 0.01) + add.double()
    got_act = twice_and_replayed(lambda: K.grouped_linear(xd, wd, bd, ad, scale, act=1, alpha=0.01))
    print("grouped_linear", b, r, k, o, maxabs(got_act, want_act))
    assert maxabs(got_act, want_act) < 2e-5 * float(want_act.abs().max())
    want = torch.einsum("brk,rok->bro", x.double(), w.double()) * 0.37
    got = K.grouped_linear(xd, wd, None, None, 0.37)
    assert maxabs(got, want) < 2e-5 * float(want.abs().max())
    # a sample's outputs do not depend on the batch
    assert torch.equal(K.grouped_linear(xd[-1:].contiguous(), wd, bd, ad, scale, act=1, alpha=0.01)[0], got_act[-1])


# ---- item 5: the streaming kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h,w,with_skip", [(2, 1024, 1024, True), (2, 64, 64, False), (1, 10, 6, True), (3, 7, 9, False),
                                             (2, 12, 20, True)])
def test_torgb_finish_vs_fp64(b, h, w, with_skip):
    """out = partial + bias + upfirdn2d(skip, k4, up=2, pad=(2, 1))   (model.py:441-446)"""
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(h + w)
    partial = torch.randn(b, 3, h, w, generator=g)
    bias = torch.randn(1, 3, 1, 1, generator=g)
    k4 = orc.make_blur_kernel() * 4
    skip = torch.randn(b, 3, h // 2, w // 2, generator=g) if with_skip else None
    want = partial.double() + bias.double()
    if with_skip:
        want = want + orc.upfirdn2d(skip.double(), k4.double(), up=2, down=1, pad=(2, 1))
    pd, bd, kd = partial.to(DEV), bias.to(DEV), k4.to(DEV)
    sd = skip.to(DEV) if with_skip else None
    got = twice_and_replayed(lambda: K.torgb_finish(pd, bd, sd, kd if with_skip else None))
    print("torgb_finish", b, h, w, maxabs(got, want))
    assert maxabs(got, want) < 2e-5 * float(want.abs().max())


@pytest.mark.parametrize("cin,h,w,masked,with_skip", [(256, 128, 128, True, True), (512, 64, 64, True, True),
                                                     (512, 4, 4, True, False), (256, 6, 10, True, True),
                                                     (320, 5, 7, False, False), (256, 14, 6, False, True)])
def test_torgb_wide_channels_vs_fp64(cin, h, w, masked, with_skip):
    """ToRGB at Cin >= 256: out[b, ch, p] = sum_c x[b, p, c] ws[g(b, p), ch, c] + bias[ch] + upsampled skip, g = b * R + label(p)
    on a masked layer (model.py:422-448 with the one-hot mask folded into a per-pixel choice of style)."""
    from e4s_amd import kernels as K
    b, r = 2, 12
    g = torch.Generator().manual_seed(cin + h)
    x = torch.randn(b, h, w, cin, generator=g)
    ws = torch.randn(b * r if masked else b, 3, cin, generator=g) / math.sqrt(cin)
    bias = torch.randn(3, generator=g)
    k4 = orc.make_blur_kernel() * 4
    skip = torch.randn(b, 3, h // 2, w // 2, generator=g) if with_skip else None
    lab = synth.synth_labels_blocks(b, 512, 64, seed=2)
    if masked:
        gi = nearest_labels(lab, h, w) + torch.arange(b).view(b, 1, 1) * r                 # [B,h,w]
    else:
        gi = torch.arange(b).view(b, 1, 1).expand(b, h, w)
    want = torch.einsum("bhwc,bhwkc->bkhw", x.double(), ws.double()[gi]) + bias.double().view(1, 3, 1, 1)
    if with_skip:
        want = want + orc.upfirdn2d(skip.double(), k4.double(), up=2, down=1, pad=(2, 1))
    labels = K.mask_labels(synth.onehot(lab).to(DEV))[0] if masked else None
    xd, wd, bd, kd = x.to(DEV), ws.to(DEV), bias.to(DEV), k4.to(DEV)
    sd = skip.to(DEV) if with_skip else None
    got = twice_and_replayed(lambda: K.torgb(xd, wd, bd, sd, kd if with_skip else None, labels, r))
    print("torgb", cin, h, w, masked, maxabs(got, want))
    assert maxabs(got, want) < 5e-5


@pytest.mark.parametrize("b,r,h,w", [(2, 12, 512, 512), (3, 12, 256, 256), (2, 5, 7, 9), (1, 12, 6, 10), (2, 3, 5, 4)])
def test_mask_labels_vs_argmax(b, r, h, w):
    """labels = the FIRST largest plane per pixel; flags != 0 exactly when some pixel is not one-hot."""
    from e4s_amd import kernels as K
    g = torch.Generator().manual_seed(h * w)
    lab = torch.randint(0, r, (b, 1, h, w), generator=g)
    mask = synth.onehot(lab, r)
    md = mask.to(DEV)
    got = twice_and_replayed(lambda: K.mask_labels(md)[0])
    assert torch.equal(got.cpu().long(), lab[:, 0])
    assert int(K.mask_labels(mask.to(DEV))[1].item()) == 0
    soft = torch.rand(b, r, h, w, generator=g)
    soft[0, :, h // 2, w // 2] = 0.25                                     # a tie: the first plane wins
    lab2, flags = K.mask_labels(soft.to(DEV))
    first_max = (soft == soft.max(1, keepdim=True).values).float().argmax(1)
    assert torch.equal(lab2.cpu().long(), first_max) and int(flags.item()) != 0
    for bad in (0.5, 1.0):                                                # one stray value / two ones in the last pixel
        m2 = mask.clone()
        m2[b - 1, (int(lab[b - 1, 0, h - 1, w - 1]) + 1) % r, h - 1, w - 1] = bad
        assert int(K.mask_labels(m2.to(DEV))[1].item()) != 0


# ---- item 1: the overflow launch behind a masked conv -------------------------------------------------------------------
def _masked_conv_case(b, h, w, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    r = 12
    x = torch.randn(b, h, w, cin, generator=g).to(DEV)
    wt = torch.randn(1, 9, cout, cin, generator=g).to(DEV) / math.sqrt(cin * 9)
    kw = dict(num_regions=r, ncls=1, ostride=1,
              in_scale=(torch.rand(b * r, cin, generator=g) + 0.5).to(DEV), out_scale=(torch.rand(b * r, cout, generator=g) + 0.5).to(DEV),
              noise=torch.randn(b, 1, h, w, generator=g).to(DEV), noise_w=torch.tensor([0.2], device=DEV),
              bias=(torch.randn(cout, generator=g) * 0.1).to(DEV), act=1)
    face = synth.synth_labels_face(b, 512, seed=seed).view(b, 512, 512)[:, ::512 // h, ::512 // w].contiguous()
    noise = torch.randint(0, r, (b, h, w), generator=g)               # per-pixel random regions: every tile overflows
    return x, wt, kw, face.to(torch.uint8).to(DEV), noise.to(torch.uint8).to(DEV)


@pytest.mark.parametrize("b,h,w,cin,cout", [(2, 64, 64, 64, 128), (8, 64, 64, 64, 256), (1, 32, 32, 512, 512)])
def test_overflow_launch_behind_a_masked_conv(b, h, w, cin, cout):
    """The launch behind the variant-rows kernels (8-wave, one-wave-per-SIMD and split-K forms) contracts the tiles they flagged on
    the region-select kernel and leaves at once when none is flagged.  Per-pixel random regions: every tile is flagged and the
    output is the region-select kernel's, bit for bit (bound of test_region_rows_kernel_*: 5e-6 of the output scale).  Face maps: the
    output is within that bound of the region-select kernel's.  One captured launch replayed over face -> noise -> one region -> face
    labels == the eager launch on each (a flag table left by the previous map must not leak), and the face result comes back bit
    for bit."""
    from e4s_amd import kernels as K
    x, wt, kw, face, noise = _masked_conv_case(b, h, w, cin, cout, 50 + b)
    ws, ws16 = K.split_bf16x2(wt), K.split16_bf16x2(wt)
    lab = face.clone()
    rows = lambda: K.conv_mfma(x, wt, cout, w_split=ws, w_split16=ws16, labels=lab, **kw)
    select = lambda: K.conv_mfma(x, wt, cout, w_split=ws, labels=lab, **kw)
    y_face = twice_and_replayed(rows)
    assert K.LAST_REGION_PATH in (1, 2)
    sel_face = select()
    scale = float(sel_face.abs().max())
    print("overflow launch", b, h, w, cin, cout, "face: rows vs select", maxabs(y_face, sel_face) / scale)
    assert maxabs(y_face, sel_face) < 5e-6 * scale
    lab.copy_(noise)
    y_noise, sel_noise = rows(), select()
    print("overflow launch noise: rows vs select", maxabs(y_noise, sel_noise) / scale)
    assert maxabs(y_noise, sel_noise) < 5e-6 * scale and torch.equal(y_noise, sel_noise)
    lab.copy_(face)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rows()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = rows()
    for labels, want in ((face, y_face), (noise, y_noise), (torch.full_like(face, 3), None), (face, y_face)):
        lab.copy_(labels)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, rows())
        if want is not None:
            assert torch.equal(y, want)
