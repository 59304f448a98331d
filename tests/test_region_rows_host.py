"""Host side of the variant-rows tile (no GPU): the layout functions of csrc/region_rows.h and csrc/rows64.h -- the ones the two masked
conv kernels compile -- walked by a stand-alone C++ program under AddressSanitizer + UBSan (tests/region_rows_main.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "e4s_amd", "csrc")


@pytest.fixture(scope="module")
def layout_run(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the layout check")
    exe = str(tmp_path_factory.mktemp("region_rows") / "region_rows")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "region_rows_main.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    return res.stdout.splitlines()


def test_halo_and_variant_rows_partition_the_buffer_and_own_row_reads_are_conflict_free(layout_run):
    """324 halo rows + 252 variant rows = 576 distinct LDS rows; 8 row tiles x 9 taps x 2 k-halves x {hi, lo} x 2 lane groups of a
    ds_read_b128, each hitting 16 different 16-byte slots of the bank line (asserted by the program, case by case)."""
    assert layout_run[-1] == "OK 576 %d" % (8 * 9 * 2 * 2 * 2)
    assert not [ln for ln in layout_run if ln.startswith("FAILED")]

