"""Host side of the one-wave-per-SIMD gather conv (no GPU): the LDS addressing of csrc/gather1w_rows.h walked lane group by lane group by a
stand-alone C++ program under AddressSanitizer + UBSan (every granule of a stage stored once, ds_write_b128 and ds_read_b128 service groups
free of bank conflicts), and the staging-row deal restated in Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "e4s_amd", "csrc")


@pytest.fixture(scope="module")
def rows_run(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the host checks")
    exe = str(tmp_path_factory.mktemp("gather1w_rows") / "gather1w_rows")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "gather1w_rows_main.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return res.stdout.splitlines()


def test_lds_stage_under_sanitizers(rows_run):
    assert rows_run[-1] == "OK" and len(rows_run) == 65


def test_stage_row_restated(rows_run):
    """bits 0 and 2 of the row index swapped: a bijection of 0..63 whose consecutive pairs are four rows apart"""
    got = [int(v) for v in rows_run[:64]]
    want = [(q & ~5) | ((q & 1) << 2) | ((q >> 2) & 1) for q in range(64)]
    assert got == want and sorted(got) == list(range(64))
    assert all(got[q + 1] - got[q] == 4 for q in range(0, 64, 2))
