"""Host side of the few-tile launches (no GPU): the geometry of the packed small-map tiles (csrc/few_tile_geom.h) walked by a stand-alone
C++ program under AddressSanitizer + UBSan, and the K-split rules of the packed masked launches and of the strided gather kernel restated
in Python and compared with what the library's workspace functions answer (the launchers ask the same functions: region_split /
gather_split in csrc/conv_bf16x3.hip)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "e4s_amd", "csrc")


def n_img(h, w):
    """few_tile_geom.h pack_geom: whole images of an h x w map per 256-row tile with a 324-slot halo array (0: not eligible)."""
    if not (1 <= h <= 16 and 1 <= w <= 16):
        return 0
    n = min(324 // ((h + 2) * (w + 2)), 256 // (h * w))
    return n if n >= 2 else 0


def pack_split(tiles, nchunk):
    """few_tile_geom.h pack_split -> (ksplit, cper)"""
    want = min(256 // tiles, nchunk) if tiles >= 1 else 0
    if nchunk < 2 or want < 2:
        return 1, nchunk
    cper = -(-nchunk // want)
    return -(-nchunk // cper), cper


def few_tiles_split(tiles, nchunk):
    """csrc/conv_bf16x3.hip few_tiles_split -> ksplit"""
    if tiles > 128 or nchunk < 4:
        return 1
    want = min(-(-256 // tiles), nchunk // 2)
    if want < 2:
        return 1
    cper = -(-nchunk // want)
    return -(-nchunk // cper)


@pytest.fixture(scope="module")
def geom_run(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the geometry check")
    exe = str(tmp_path_factory.mktemp("few_tile") / "few_tile_geom")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "few_tile_geom_main.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return res.stdout.splitlines()


def test_packed_tile_geometry_under_sanitizers(geom_run):
    """Every (image, y, x) in exactly one live row, every tap of a live row inside its own image's halo block and on the right pixel or the
    zero ring, slots < 324, rows < 256 -- for every eligible map and b = 1 .. 2 n_img + 1 (asserted by the program); the eligible maps and
    their images per tile are those of the rule restated here: 9 at 4x4, 3 at 8x8, none at 16x16."""
    assert geom_run[-1].startswith("OK ")
    got = {(int(a), int(b)): int(c) for a, b, c in (ln.split() for ln in geom_run if ln[0].isdigit())}
    want = {(h, w): n_img(h, w) for h in range(1, 19) for w in range(1, 19) if n_img(h, w)}
    assert got == want and int(geom_run[-1].split()[1]) == len(want)
    assert want[(4, 4)] == 9 and want[(8, 8)] == 3 and want[(4, 8)] == 5 and want[(5, 7)] == 5 and (16, 16) not in want and (8, 16) not in want


def test_pack_split_restated(geom_run):
    rows = [tuple(int(v) for v in ln.split()[1:]) for ln in geom_run if ln.startswith("split ")]
    assert len(rows) == 300 * 32
    for tiles, nchunk, ksplit, cper in rows:
        assert (ksplit, cper) == pack_split(tiles, nchunk), (tiles, nchunk)
    # the workload's four layers at batch 8 (Cin = 512: 16 chunks; 4 column tiles): 4^2 conv, 4^2 -> 8^2, 8^2 conv, 8^2 -> 16^2
    assert [pack_split(t, 16) for t in (4, 16, 12, 48)] == [(16, 1), (16, 1), (16, 1), (4, 4)]


def _params(lib, b, h, w, cin, cout, *, up=False, masked=True, stride=1, ntaps=9, ycs=0):
    p = lib.ConvParams()
    ctypes.memset(ctypes.byref(p), 0, ctypes.sizeof(p))
    s = 2 if up else 1
    p.B, p.Ha, p.Wa = b, h // stride, w // stride
    p.Hi, p.Wi, p.Ho, p.Wo, p.Cin, p.Cout = h, w, h // stride * s, w // stride * s, cin, cout
    p.istride, p.ostride, p.ntaps, p.ncls = stride, s, ntaps, 4 if up else 1
    p.groups_per_batch = 12 if masked else 1
    p.y_cstride = ycs
    if masked:
        p.labels = p.in_scale = 64            # never dereferenced by the host-side policy functions
        p.Hm, p.Wm = p.Ho, p.Wo
    return p


@pytest.fixture(scope="module")
def so():
    from e4s_amd import lib
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in ("e4s_conv_region_ws_floats", "e4s_conv_bf16x3_ws_floats"):
        getattr(so, n).restype = ctypes.c_int64
        getattr(so, n).argtypes = [ctypes.POINTER(lib.ConvParams)]
    so.e4s_conv_region_path.restype = ctypes.c_int
    so.e4s_conv_region_path.argtypes = [ctypes.POINTER(lib.ConvParams)]
    return so


@pytest.mark.parametrize("b,h,w,cin,cout,up", [
    (8, 4, 4, 512, 512, False), (8, 4, 4, 512, 512, True), (8, 8, 8, 512, 512, False), (8, 8, 8, 512, 512, True), (1, 8, 8, 512, 512, False),
    (9, 4, 4, 64, 128, False), (10, 4, 4, 64, 256, True), (3, 8, 8, 128, 128, False), (5, 4, 8, 64, 128, False), (2, 5, 7, 32, 128, True),
    (1, 4, 4, 512, 512, False), (8, 16, 16, 512, 512, False), (8, 16, 16, 512, 512, True), (1, 32, 32, 512, 512, False), (8, 8, 16, 128, 128, False)])
def test_masked_workspace_follows_the_restated_split(so, b, h, w, cin, cout, up):
    """Both workspace entry points of a masked launch report the slabs of the restated rule -- pack_split over ceil(B / n_img) tiles per
    class for the small maps (path 3), few_tiles_split over one tile per image and 16x16 patch otherwise (paths 1 / 2) -- plus, for the
    variant-rows entry, its tile-flag table."""
    from e4s_amd import kernels as K, lib
    p = _params(lib, b, h, w, cin, cout, up=up)
    ncls, s = (4, 2) if up else (1, 1)
    n = n_img(h, w) if K.REGION_PACK else 0
    if n:
        ksplit = pack_split(-(-b // n) * ncls * (cout // 128), cin // 32)[0]
    else:
        ksplit = few_tiles_split(b * -(-h // 16) * -(-w // 16) * ncls * (cout // 128), cin // 32)
    slabs = ksplit * b * h * s * w * s * cout if ksplit > 1 else 0
    assert so.e4s_conv_bf16x3_ws_floats(ctypes.byref(p)) == slabs
    assert so.e4s_conv_region_ws_floats(ctypes.byref(p)) == slabs + b * -(-h // 16) * -(-w // 16) * ncls
    path = so.e4s_conv_region_path(ctypes.byref(p))
    assert (path == 3) == bool(n) and path in (1, 2, 3)


@pytest.mark.parametrize("b,h,w,cin,cout,ntaps,ycs", [
    (16, 32, 32, 512, 512, 9, 0), (2, 32, 32, 512, 512, 9, 0), (1, 16, 16, 256, 128, 9, 0), (2, 12, 20, 256, 128, 9, 0), (1, 8, 8, 512, 64, 9, 0),
    (2, 6, 10, 512, 512, 9, 0), (3, 32, 48, 128, 256, 9, 0), (16, 64, 64, 128, 128, 9, 0), (1, 16, 16, 512, 128, 1, 0), (17, 32, 32, 512, 512, 9, 0),
    (1, 16, 16, 256, 128, 9, 160), (1, 16, 16, 256, 128, 9, 130)])
def test_gather_workspace_follows_the_restated_split(so, b, h, w, cin, cout, ntaps, ycs):
    """kernels.gather_split (the policy side, encoders._conv_strided) == the library's rule: 3x3, <= 64 tiles, Cin >= 256, >= 2 chunks per split;
    a channel stride that is no multiple of 4 keeps the launch whole (16-byte slab reads)."""
    from e4s_amd import kernels as K, lib
    p = _params(lib, b, h, w, cin, cout, masked=False, stride=2, ntaps=ntaps, ycs=ycs)
    npix = b * (h // 2) * (w // 2)
    tiles = -(-npix // 256) * -(-cout // 128)
    ksplit = K.gather_split(tiles, cin, ntaps) if (ycs or cout) % 4 == 0 else 1
    assert ksplit == (few_tiles_split(tiles, cin // 32) if (ntaps == 9 and tiles <= 64 and cin >= 256 and (ycs or cout) % 4 == 0) else 1)
    assert so.e4s_conv_bf16x3_ws_floats(ctypes.byref(p)) == (ksplit * npix * (ycs or cout) if ksplit > 1 else 0)
    if (b, cin, cout) == (16, 512, 512):
        assert ksplit == 4                   # the encoder's last stride-2 conv at 16 images: 64 tiles x 4 = one block per CU, 36 stages each
