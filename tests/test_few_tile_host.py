"""Host side of the few-tile launches (no GPU): the geometry of the packed small-map tiles (csrc/few_tile_geom.h) and every K-split rule
(csrc/split_policy.h) walked by stand-alone C++ programs under AddressSanitizer + UBSan, and the rules restated in Python and compared
with those programs' rows over their whole grid and with what the library's workspace functions answer (the launchers read the same
launch plans: csrc/conv_launch.h)."""
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
    """split_policy.h pack_split -> (ksplit, cper)"""
    want = min(256 // tiles, nchunk) if tiles >= 1 else 0
    if nchunk < 2 or want < 2:
        return 1, nchunk
    cper = -(-nchunk // want)
    return -(-nchunk // cper), cper


def few_tiles_split(tiles, nchunk):
    """split_policy.h few_tiles_split -> ksplit"""
    if tiles > 128 or nchunk < 4:
        return 1
    want = min(-(-256 // tiles), nchunk // 2)
    if want < 2:
        return 1
    cper = -(-nchunk // want)
    return -(-nchunk // cper)


def wino_split(tiles, nchunk):
    """split_policy.h few_tiles_split_guarded (the Winograd kernels, 16-channel chunks) -> ksplit: a split whose last part is ONE chunk is refused"""
    if tiles > 128 or nchunk < 4:
        return 1
    want = min(-(-256 // tiles), nchunk // 2)
    if want < 2:
        return 1
    cper = -(-nchunk // want)
    ksplit = -(-nchunk // cper)
    return ksplit if nchunk - (ksplit - 1) * cper >= 2 else 1


def _build_and_run(tmp_path_factory, name):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the host checks")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                    os.path.join(ROOT, "tests", name + "_main.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return res.stdout.splitlines()


@pytest.fixture(scope="module")
def geom_run(tmp_path_factory):
    return _build_and_run(tmp_path_factory, "few_tile_geom")


@pytest.fixture(scope="module")
def policy_rows(tmp_path_factory):
    """split_policy_main's rows: {rule: {(tiles, nchunk): (ksplit, cper)}}; the program itself asserted, under the sanitizers, that every
    chunk lies in exactly one non-empty split, ksplit cper >= nchunk > (ksplit - 1) cper, and the Winograd form's last split >= 2 chunks."""
    lines = _build_and_run(tmp_path_factory, "split_policy")
    assert lines[-1] == "OK"
    rows = {}
    for rule, tiles, nchunk, ksplit, cper in (ln.split() for ln in lines[:-1]):
        rows.setdefault(rule, {})[(int(tiles), int(nchunk))] = (int(ksplit), int(cper))
    return rows


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


def test_every_rule_restated_over_the_whole_grid(policy_rows):
    """The C++ rules == the Python restatements above for every tiles 1..300 x chunks 1..128 (cper: the smallest part size that gives
    ksplit parts, which is what ceil(nchunk / want) is)."""
    assert sorted(policy_rows) == ["few", "gather", "gather1x1", "pack", "wino"]
    grid = {(t, n) for t in range(1, 301) for n in range(1, 129)}
    for rule, rows in policy_rows.items():
        assert set(rows) == grid, rule
    for (t, n), (ksplit, cper) in policy_rows["few"].items():
        assert ksplit == few_tiles_split(t, n), (t, n)
        assert cper == (-(-n // min(-(-256 // t), n // 2)) if ksplit > 1 else n), (t, n)
    for (t, n), (ksplit, cper) in policy_rows["wino"].items():
        assert ksplit == wino_split(t, n), (t, n)
        assert (ksplit, cper) in ((1, n), policy_rows["few"][(t, n)]), (t, n)
    for (t, n), (ksplit, cper) in policy_rows["gather"].items():
        assert ksplit == (few_tiles_split(t, n) if t <= 64 and n >= 8 else 1), (t, n)
        assert (ksplit, cper) in ((1, n), policy_rows["few"][(t, n)]), (t, n)
    assert set(policy_rows["gather1x1"].values()) <= {(1, n) for n in range(1, 129)}
    for (t, n), got in policy_rows["pack"].items():
        assert got == pack_split(t, n), (t, n)
    # few_tiles_split's last split may hold ONE chunk (the header says so); the Winograd form refuses exactly those
    assert policy_rows["few"][(43, 16)] == (6, 3) and policy_rows["wino"][(43, 16)] == (1, 16)
    assert policy_rows["few"][(1, 7)] == (3, 3) and policy_rows["wino"][(1, 7)] == (1, 7) and policy_rows["wino"][(1, 4)] == (2, 2)


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


# ---- the launch plans (csrc/conv_launch.h) over a grid of shapes: what a workspace query answers is what the restated rule predicts ----
GRID_B = (1, 2, 3, 5, 8, 9, 16)
GRID_HW = (4, 8, 12, 16, 20, 32, 48, 64, 128)
GRID_C = (32, 64, 128, 256, 512)


def _grid():
    return [(b, hw, cin, cout) for b in GRID_B for hw in GRID_HW for cin in GRID_C for cout in GRID_C]


def test_plain_and_upconv_plans_over_the_grid(so):
    """e4s_conv_bf16x3_ws_floats without a label map: column tile 128 / 64 / 32 by Cout (polyphase up-conv: 4 Cout columns of 128),
    few_tiles_split over batch x 16x16 patches x column tiles."""
    from e4s_amd import lib
    for b, hw, cin, cout in _grid():
        for up in (False, True):
            n = 4 * cout if up else cout
            bn = 128 if n % 128 == 0 else 64 if n % 64 == 0 else 32
            ksplit = few_tiles_split(b * (-(-hw // 16)) ** 2 * (n // bn), cin // 32)
            s = 2 if up else 1
            want = ksplit * b * hw * s * hw * s * cout if ksplit > 1 else 0
            assert so.e4s_conv_bf16x3_ws_floats(ctypes.byref(_params(lib, b, hw, hw, cin, cout, up=up, masked=False))) == want, (b, hw, cin, cout, up)


def test_masked_plan_over_the_grid(so):
    """Both workspace queries and the path query of a masked launch read ONE plan: path 3 (packed small maps, pack_split), else
    few_tiles_split over one tile per image, patch, class and 128 columns; path 2 (one wave per SIMD) exactly when nothing is split and
    Cout % 256 == 0.  Widths the variant-rows entry does not cover: no workspace, path 0."""
    from e4s_amd import kernels as K, lib
    for b, hw, cin, cout in _grid():
        for up in (False, True):
            p = _params(lib, b, hw, hw, cin, cout, up=up)
            ncls, s = (4, 2) if up else (1, 1)
            if cout % 128:
                assert so.e4s_conv_region_ws_floats(ctypes.byref(p)) == 0 and so.e4s_conv_region_path(ctypes.byref(p)) == 0
                continue
            n = n_img(hw, hw) if K.REGION_PACK else 0
            flags = b * (-(-hw // 16)) ** 2 * ncls
            ksplit = pack_split(-(-b // n) * ncls * (cout // 128), cin // 32)[0] if n else few_tiles_split(flags * (cout // 128), cin // 32)
            slabs = ksplit * b * hw * s * hw * s * cout if ksplit > 1 else 0
            path = 3 if n else 2 if (K.REGION_1W and ksplit == 1 and cout % 256 == 0) else 1
            case = (b, hw, cin, cout, up)
            assert so.e4s_conv_bf16x3_ws_floats(ctypes.byref(p)) == slabs, case
            assert so.e4s_conv_region_ws_floats(ctypes.byref(p)) == slabs + flags, case
            assert so.e4s_conv_region_path(ctypes.byref(p)) == path, case


def test_gather_and_winograd_plans_over_the_grid(so):
    """Stride-2 3x3 and 1x1 launches (gather kernel): few_tiles_split where 3x3, <= 64 tiles and Cin >= 256, and e4s_gather_ksplit
    (kernels.gather_split) says the same.  Winograd: few_tiles_split over 16-channel chunks with the last-split guard."""
    from e4s_amd import kernels as K, lib
    so.e4s_conv_wino_ws_floats.restype = ctypes.c_int64
    so.e4s_conv_wino_ws_floats.argtypes = [ctypes.POINTER(lib.ConvParams)]
    for b, hw, cin, cout in _grid():
        if cout % 128 == 0 or cout == 64:
            npix = b * (hw // 2) ** 2
            tiles = -(-npix // 256) * -(-cout // 128)
            for ntaps in (9, 1):
                ksplit = few_tiles_split(tiles, cin // 32) if (ntaps == 9 and tiles <= 64 and cin >= 256) else 1
                assert K.gather_split(tiles, cin, ntaps) == ksplit, (tiles, cin, ntaps)
                p = _params(lib, b, hw, hw, cin, cout, masked=False, stride=2, ntaps=ntaps)
                assert so.e4s_conv_bf16x3_ws_floats(ctypes.byref(p)) == (ksplit * npix * cout if ksplit > 1 else 0), (b, hw, cin, cout, ntaps)
        p = _params(lib, b, hw, hw, cin, cout, masked=False)
        covered = hw % 16 == 0 and cout % 128 == 0
        ksplit = wino_split(b * (hw // 16) ** 2 * (cout // 128), cin // 16) if covered else 1
        assert so.e4s_conv_wino_ws_floats(ctypes.byref(p)) == (ksplit * b * hw * hw * cout if ksplit > 1 else 0), (b, hw, cin, cout)


# ---- the Python policy: one fill estimate (kernels.fills_chip) behind three predicates; their decisions are those of the expressions they replaced ----
def _old_asked(tiles, nchunk):
    split = min(nchunk // 2, -(-256 // tiles)) if nchunk >= 4 else 1
    return tiles * max(split, 1) >= 64


def _old_want_bf16x3(K, b, h, w, cin, cout, ncls=1, masked=False):
    if K.PRECISION == "f32" or not K.bf16x3_eligible(cin, cout, ncls=ncls, ostride=2 if ncls == 4 else 1, masked=masked):
        return False
    if K.PRECISION == "bf16x3":
        return True
    n = 4 * cout if (ncls == 4 and not masked) else cout
    bn = 128 if n % 128 == 0 else 64 if n % 64 == 0 else 32
    tiles = b * ((h + 15) // 16) * ((w + 15) // 16) * (n // bn) * (ncls if masked else 1)
    if tiles >= K.BF16X3_MIN_BLOCKS:
        return True
    return _old_asked(tiles, cin // 32)


def _old_wino_eligible(K, b, h, w, cin, cout, in_stats=False):
    if not K.WINO or K.PRECISION == "f32":
        return False
    if h % 16 or w % 16 or cin % 16 or cin < 32 or cout % 128:
        return False
    if in_stats and cin > 1024:
        return False
    if K.PRECISION == "bf16x3":
        return True
    tiles = b * (h // 16) * (w // 16) * (cout // 128)
    if tiles >= K.BF16X3_MIN_BLOCKS:
        return True
    return _old_asked(tiles, cin // 16)


def _old_gather_split(tiles, cin, ntaps):
    if ntaps != 9 or tiles < 1 or tiles > 64 or cin < 256 or cin % 32:
        return 1
    nchunk = cin // 32
    want = min(nchunk // 2, -(-256 // tiles))
    if want < 2:
        return 1
    cper = -(-nchunk // want)
    return -(-nchunk // cper)


def _old_strided(K, b, h, wd, cin, cout, stride, ntaps):
    covered = cout % 128 == 0 or cout == 64
    tiles = (b * (h // stride) * (wd // stride) + 255) // 256 * ((cout + 127) // 128 if covered else 0)
    filled = tiles >= K.BF16X3_MIN_BLOCKS or tiles * _old_gather_split(tiles, cin, ntaps) >= 64
    return K.PRECISION != "f32" and covered and (K.PRECISION == "bf16x3" or filled)


@pytest.mark.parametrize("precision", ["auto", "f32", "bf16x3"])
def test_policy_decisions_are_those_of_the_replaced_expressions(monkeypatch, precision):
    from e4s_amd import encoders, kernels as K
    monkeypatch.setattr(K, "PRECISION", precision)
    diffs = []
    for b, hw, cin, cout in _grid():
        for ncls, masked in ((1, False), (4, False), (1, True), (4, True)):
            if K.want_bf16x3(b, hw, hw, cin, cout, ncls, masked=masked) != _old_want_bf16x3(K, b, hw, hw, cin, cout, ncls, masked):
                diffs.append(("want_bf16x3", b, hw, cin, cout, ncls, masked))
        for in_stats in (False, True):
            if K.wino_eligible(b, hw, hw, cin, cout, in_stats=in_stats) != _old_wino_eligible(K, b, hw, hw, cin, cout, in_stats):
                diffs.append(("wino_eligible", b, hw, cin, cout, in_stats))
        for ntaps in (9, 1):
            if bool(encoders.strided_bf16x3(b, hw, hw, cin, cout, 2, ntaps)) != bool(_old_strided(K, b, hw, hw, cin, cout, 2, ntaps)):
                diffs.append(("strided", b, hw, cin, cout, ntaps))
    assert not diffs, diffs[:20]


def test_product_library_reads_no_unset_split_switch():
    """The seven environment switches that steered split counts (and so summation order) exist only in profiling builds
    (E4S_BUILD_ABLATIONS=1): a product library does not contain their names."""
    from e4s_amd import lib
    with open(lib.LIB_PATH, "rb") as fh:
        blob = fh.read()
    assert b"E4S_REGION_PACK" in blob and b"E4S_WINO_WT" in blob            # (the search does find the switches that stay)
    for name in (b"E4S_F32_MAX_SPLIT", b"E4S_F32_MIN_CHUNKS", b"E4S_F32_PLAIN_SPLIT", b"E4S_WGRAD_BF16X3", b"E4S_WGRAD_BLOCKS",
                 b"E4S_WGRAD_MASKED_MIN_ANCHORS", b"E4S_WINO_GRID"):
        assert name not in blob, name
