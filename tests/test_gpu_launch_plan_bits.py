"""The conv launchers take their tiles, K split and workspace layout from one launch plan per entry point (csrc/conv_launch.h; the split
rules from csrc/split_policy.h).  Moving the host code there changed no kernel and no launch: every output is bit-identical to the
commit before the move.  Per seeded case, on the smallest shape that takes the branch (batch 1, 16x16 map unless the case says
otherwise): the workspace query answers the size stated here, then SHA-256 of the output bytes == tests/golden/launch_plan_parent_digests.json
(tools/parent_digests.py wrote it from that commit's library: tools/build_prev_lib.sh + E4S_LIB_PATH).  The launchers the other bit
fixtures do not reach: the plain persistent kernel in its four column-tile configurations, split and whole, with and without styles
(the split launches' second stage applies the demodulation), its InstanceNorm-staging form; the strided gather kernel; the 8-wave
Winograd kernel, with the split its last-split guard refuses; e4s_conv_mfma_f32's own split.  The split cases digest the output only
(the slabs are scratch).  The module talks to the library through ctypes directly, so that the parent's library -- another ABI version,
same entry points -- can run the same cases."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plan_parent_digests.json")
GOLDEN_ENV = {}

# id: (entry, Hi = Wi, Cin, Cout, form, floats of split-K workspace the query must answer)
# entry: plain / up (polyphase, ncls 4) / gather3 / gather1 (stride 2, 16x16 anchors) / wino / mfma; form: "", "styled" (in_scale, out_scale,
# noise, bias, leaky-relu) or "in_stats"
CASES = {
    "plainL16-128to128-split2x2-styled": ("plain", 16, 128, 128, "styled", 2 * 256 * 128),
    "plainL16-160to128-split3+2": ("plain", 16, 160, 128, "", 2 * 256 * 128),
    "plainL16-64to128-whole": ("plain", 16, 64, 128, "styled", 0),
    "plainM-64to64-whole": ("plain", 16, 64, 64, "styled", 0),
    "plainS-32to32-whole": ("plain", 16, 32, 32, "", 0),
    "plainSHUF-128to32-up-split-styled": ("up", 16, 128, 32, "styled", 2 * 1024 * 32),
    "plainL16-128to128-in_stats-split": ("plain", 16, 128, 128, "in_stats", 2 * 256 * 128),
    "gather-256to128-split4x2": ("gather3", 32, 256, 128, "", 4 * 256 * 128),
    "gather-128to128-whole": ("gather3", 32, 128, 128, "", 0),
    "gather-1x1-256to128-whole": ("gather1", 32, 256, 128, "", 0),
    "wino8w-64to128-split2x2": ("wino", 16, 64, 128, "", 2 * 256 * 128),
    "wino8w-112to128-guard-whole": ("wino", 16, 112, 128, "", 0),           # 3 + 3 + 1 chunks of 16: refused, one launch
    "mfma-8x8-128to128-split4x1": ("mfma", 8, 128, 128, "styled", 4 * 64 * 128),
    "mfma-8x8-64to128-whole": ("mfma", 8, 64, 128, "styled", 0),
}


def golden_cases():
    return {cid: (cid,) for cid in CASES}


_so = None


def _lib():
    """The library under test, without e4s_amd.lib.load()'s ABI check (see the module docstring); argument types from lib.SIGNATURES."""
    global _so
    if _so is None:
        from e4s_amd import lib
        _so = ctypes.CDLL(lib.LIB_PATH)
        for name in ("e4s_split_bf16x2_f32", "e4s_conv_bf16x3_ws_floats", "e4s_conv_bf16x3_f32", "e4s_wino_weights_bytes", "e4s_wino_weights_f32",
                     "e4s_conv_wino_ws_floats", "e4s_conv_wino_bf16x3_f32", "e4s_conv_mfma_ws_floats", "e4s_conv_mfma_f32"):
            fn = getattr(_so, name)
            fn.argtypes = lib.SIGNATURES[name]
            fn.restype = ctypes.c_int64 if name in lib.INT64_RETURN else ctypes.c_int
    return _so


def run_case(cid):
    """Builds the launch of case `cid` from seeded tensors, asserts the workspace query, launches -> {"y": output}."""
    from e4s_amd import lib
    entry, hi, cin, cout, form, want_ws = CASES[cid]
    so, dev = _lib(), "cuda"
    g = torch.Generator().manual_seed(sum(cid.encode()))
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).to(dev)
    up, stride = entry == "up", 2 if entry in ("gather3", "gather1") else 1
    ncls, ostride, ntaps = (4, 2, 9) if up else (1, 1, 1 if entry == "gather1" else 9)
    ha = hi // stride
    ho = ha * ostride
    x, w = rnd(1, hi, hi, cin), rnd(ncls, ntaps, cout, cin) * (1.0 / (ntaps * cin) ** 0.5)
    y = torch.full((1, ho, ho, cout), float("nan"), device=dev)
    keep = [x, w, y]
    p = lib.ConvParams()
    ctypes.memset(ctypes.byref(p), 0, ctypes.sizeof(p))
    p.x, p.w, p.y = lib.fptr(x), lib.fptr(w), lib.fptr(y)
    p.B, p.Ha, p.Wa, p.Hi, p.Wi, p.Ho, p.Wo, p.Cin, p.Cout = 1, ha, ha, hi, hi, ho, ho, cin, cout
    p.istride, p.ostride, p.ntaps, p.ncls, p.groups_per_batch = stride, ostride, ntaps, ncls, 1
    p.alpha, p.gain = 0.2, 2.0 ** 0.5
    if form == "styled":
        keep += [rnd(1, cin) * 0.3 + 1.0, rnd(1, cout) * 0.3 + 1.0, rnd(1, ho, ho), rnd(1) * 0.5, rnd(cout)]
        p.in_scale, p.out_scale, p.noise, p.noise_w, p.bias = (lib.fptr(t) for t in keep[-5:])
        p.noise_bstride, p.act = 0, 1
    elif form == "in_stats":
        keep.append(torch.stack([rnd(1, cin) * 0.2, rnd(1, cin).abs() + 0.5], dim=2).contiguous())       # [B][Cin][{mean, rstd}]
        p.in_stats = lib.fptr(keep[-1])
    st = lib.stream()

    def workspace(nws):
        assert nws == want_ws, (cid, nws, want_ws)
        if nws:
            keep.append(torch.full((nws,), float("nan"), device=dev))
            p.splitk_ws = lib.fptr(keep[-1])

    if entry == "mfma":
        workspace(so.e4s_conv_mfma_ws_floats(ctypes.byref(p), 1))
        lib.check(so.e4s_conv_mfma_f32(ctypes.byref(p), 1, st), cid)
    elif entry == "wino":
        u = torch.empty(so.e4s_wino_weights_bytes(cout, cin), device=dev, dtype=torch.uint8)
        lib.check(so.e4s_wino_weights_f32(lib.fptr(w), lib.ptr(u), cout, cin, st), cid)
        keep.append(u)
        p.w = lib.ptr(u)
        workspace(so.e4s_conv_wino_ws_floats(ctypes.byref(p)))
        lib.check(so.e4s_conv_wino_bf16x3_f32(ctypes.byref(p), st), cid)
    else:
        ws = torch.empty_like(w)
        lib.check(so.e4s_split_bf16x2_f32(lib.fptr(w), lib.ptr(ws), w.numel() // cin, cin, st), cid)
        keep.append(ws)
        p.w = lib.fptr(ws)
        workspace(so.e4s_conv_bf16x3_ws_floats(ctypes.byref(p)))
        lib.check(so.e4s_conv_bf16x3_f32(ctypes.byref(p), st), cid)
    torch.cuda.synchronize()
    return {"y": y}


def digests(out):
    torch.cuda.synchronize()
    return {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, v in sorted(out.items())}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_launch_is_bit_identical_to_the_parent(cid, golden):
    out = run_case(cid)
    assert bool(torch.isfinite(out["y"]).all()), "the launch left part of the output unwritten"
    got, want = digests(out), golden["cases"][cid]
    print(cid, "digest", got, "parent", want)
    assert got == want
