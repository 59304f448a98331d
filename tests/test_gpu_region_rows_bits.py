"""The two variant-rows kernels of the masked StyledConv (csrc/conv_region.hip, csrc/conv_region1w.hip) take their tile -- row layout,
tables, analysis, staging items -- from one header (csrc/region_rows.h).  Moving it there changed no arithmetic and no order of
addition: every output is bit-identical to the commit before the move.  Per seeded case, on the smallest shapes that reach each code
path: SHA-256 of the output bytes == tests/golden/region_rows_parent_digests.json (tools/parent_digests.py wrote it from that commit's
library: tools/build_prev_lib.sh + E4S_LIB_PATH), and K.LAST_REGION_PATH is the path the case is there for.
8-wave kernel (path 1): ragged tiles; polyphase; K split with slabs and the second stage; a map whose left half overflows the variant
rows (flags + the region-select launch behind them); all 16 regions.  One-wave kernel (path 2), default layout: one column tile with
face-like maps; polyphase with partial tiles; overflow on one side; one 32-channel chunk on a ragged map.  The four one-wave cases again
under E4S_REGION_1W=2 and =3 (the other two wave layouts) and =0 (the 8-wave kernel takes them), one fresh child process per value: the
library reads the switch once per process."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

from region_cases import region_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "region_rows_parent_digests.json")
GOLDEN_ENV = {}

# (batch, H, W, Cin, Cout, polyphase up-conv, label map, regions)
CASES_8W = [(2, 48, 40, 64, 128, False, "face", 12), (2, 32, 32, 64, 128, True, "face", 12), (1, 32, 32, 512, 512, False, "face", 12),
            (2, 64, 64, 64, 128, False, "half-noise", 12), (2, 32, 48, 64, 128, False, "blocks", 16)]
CASES_1W = [(8, 64, 64, 64, 256, False, "face", 12), (3, 48, 40, 64, 256, True, "face", 12), (8, 64, 64, 64, 256, False, "half-noise", 12),
            (5, 33, 49, 32, 256, False, "face", 12)]
CHILD_MODES = ["2", "3", "0"]            # E4S_REGION_1W: 4 x 2 waves, 2 x 2 waves with the weight ring, the 8-wave kernel


def case_id(case):
    b, h, w, cin, cout, up, kind, R = case
    return "b%d-%dx%d-%dto%d%s-%s-R%d" % (b, h, w, cin, cout, "-up" if up else "", kind, R)


def golden_cases():
    return {case_id(c): (c,) for c in CASES_8W + CASES_1W}


def run_case(case):
    """The launch under test -> {name: tensor} of everything it wrote; K.LAST_REGION_PATH says which kernel took it."""
    from e4s_amd import kernels as K
    b, h, w, cin, cout, up, kind, R = case
    x, wt, kw = region_case(b, h, w, cin, cout, up, kind, R)
    y = K.conv_mfma(x, wt, cout, w_split=K.split_bf16x2(wt), w_split16=K.split16_bf16x2(wt), **kw)
    return {"y": y}


def digests(out):
    torch.cuda.synchronize()
    return {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, v in sorted(out.items())}


def _child():
    """Runs in the child process: the one-wave cases under the E4S_REGION_1W it was started with -> one JSON line."""
    from e4s_amd import kernels as K
    res = {}
    for c in CASES_1W:
        d = digests(run_case(c))
        res[case_id(c)] = {"path": K.LAST_REGION_PATH, "y": d["y"]}
    print("DIGESTS " + json.dumps(res, sort_keys=True))


def child_digests(mode):
    env = dict(os.environ, E4S_REGION_1W=mode,
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, "-c", "import test_gpu_region_rows_bits as t; t._child()"], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-4000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("DIGESTS ")][-1]
    return json.loads(line[len("DIGESTS "):])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _variant_rows_per_tile(case):
    """Variant rows that each 16 x 16 tile of the case's FIRST image needs, counted on the CPU (tools/variant_rows_stats.py).  Only for
    maps given at output resolution (the lookup inside the kernel is then the identity)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("variant_rows_stats", os.path.join(ROOT, "tools", "variant_rows_stats.py"))
    stats = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stats)
    b, h, w, cin, cout, up, kind, R = case
    labels = region_case(b, h, w, cin, cout, up, kind, R)[2]["labels"]
    assert tuple(labels.shape[1:]) == ((2 * h, 2 * w) if up else (h, w))
    return stats.variant_rows(labels[:1].cpu().numpy().astype(int)), stats.VMAX


@pytest.mark.parametrize("case", CASES_8W + CASES_1W, ids=case_id)
def test_masked_conv_is_bit_identical_to_the_parent(case, golden):
    from e4s_amd import kernels as K
    want_path = 2 if case in CASES_1W else 1
    assert K.REGION_1W or want_path == 1, "E4S_REGION_1W=0 is set: the one-wave cases cannot reach their kernel in this process"
    if case[6] == "half-noise":
        # what the case is there for: some tiles overflow the variant rows (the rows kernel flags them and returns before it computes
        # anything; their output can only come from the region-select launch over the flag table), others do not
        rows, vmax = _variant_rows_per_tile(case)
        print(case_id(case), "variant rows per tile of image 0", rows.tolist(), "limit", vmax)
        assert (rows > vmax).any() and (rows <= vmax).any()
    got, want = digests(run_case(case)), golden["cases"][case_id(case)]
    path = K.LAST_REGION_PATH
    print(case_id(case), "path", path, "digest", got, "parent", want)
    assert path == want_path
    assert got == want


@pytest.mark.parametrize("mode", CHILD_MODES)
def test_one_wave_cases_under_the_other_layouts(mode, golden):
    got, want = child_digests(mode), golden["children"][mode]
    print("E4S_REGION_1W=" + mode, got, "parent", want)
    assert sorted(got) == sorted(case_id(c) for c in CASES_1W)
    for cid in got:
        assert got[cid]["path"] == (1 if mode == "0" else 2), cid
        assert got[cid]["y"] == want[cid]["y"], cid
