"""The gather-GEMM conv tile (csrc/gather_gemm.h) computes the recorded bits: the packed weight image and the whole output buffer of every
case of tests/gather_conv_cases.py, in both precisions, against tests/golden/gather_conv_bits.json."""
import json

import pytest

import gather_conv_cases as gc

pytestmark = pytest.mark.gpu


def test_packed_weights_and_outputs_keep_their_recorded_bits():
    """The accuracy tests of the two conv families hold a split-bf16 layer to 1e-3 x scale, far above what another summation order moves,
    so this test holds the tile to its bits: (tap, 32-channel chunk, k-step) order, lo x hi then hi x lo then hi x hi.  A mismatch
    after a change that was meant to keep the arithmetic is a finding about that change.  A DELIBERATE change of the summation order
    or of a packed layout re-records the fixture (`python tests/gather_conv_cases.py --record tests/golden/gather_conv_bits.json`
    on an MI355X) and says in its commit message which order changed and why; the input hashes must not change with it
    (tests/test_gather_conv_cases_host.py)."""
    with open(gc.FIXTURE) as fh:
        fx = json.load(fh)
    bad = []
    for name in gc.cases():
        assert gc.input_hashes(name) == fx[name]["inputs"], name
        for precision in gc.PRECISIONS:
            pack, y = gc.run(name, precision)
            got = dict(pack=gc.sha(pack), out=gc.sha(y))
            bad += [(name, precision, k) for k in got if got[k] != fx[name][precision][k]]
    assert not bad, bad
