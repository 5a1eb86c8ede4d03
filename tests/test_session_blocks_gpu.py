"""Where a hosted agent's block lies, how a session changes rank and what drains its streams are stated once in the
session core (SessionCore::agent_block, RankChange / redimension, drain) instead of per session kind and per call.  That
moved host orchestration only -- no kernel, no launch order, no argument -- so every output must equal the commit
before: tests/golden/session_blocks_parent.npz was written on an MI355X by tools/record_session_blocks.py --lib <a
library built from that commit's own sources> --out ...; the tree's library must compute every array BIT FOR BIT.

The cases (tools/record_session_blocks.py): tinyGrid3D over 3 agents (contiguous blocks of the mirror, SE ordering) and
range_aided_slam_test_2d with its 2 robots (listed columns, the range-aided ordering), r = 3, each as one process
(iterations, get_X, round with the anchor read on the device and passed from the host, a refused certify, the lift along
its direction, three more iterations, project), as a two-rank job (the same through the exchange, with certify and
certify_live; one process per rank) and as a two-rank robust job (a collective weight update before certify_live).
Times in the info arrays are left out by index; a difference is a finding to explain, never a tolerance to add."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
RECORD = os.path.join(HERE, "golden", "session_blocks_parent.npz")

import record_session_blocks as rec  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(RECORD))


def test_the_record_holds_every_case(recorded):
    assert sorted({"/".join(k.split("/")[:2]) for k in recorded}) == sorted(rec.CASES)


@pytest.mark.parametrize("case", rec.CASES)
def test_every_array_is_bitwise_the_parents(built, recorded, case):
    import dcora_amd as da
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    got = rec.compute_case(case)
    want = {k: v for k, v in recorded.items() if k.startswith(case + "/")}
    assert want and sorted(got) == sorted(want)
    for k in sorted(want):
        same_shape = got[k].shape == want[k].shape
        print(k, "max |difference|", float(np.max(np.abs(got[k] - want[k]), initial=0.0)) if same_shape else "shapes differ")
    assert rec.differing(got, want) == []
    # the case is the one it is meant to be: the certificate refused, the lift escaped to r + 1, and (one process) the
    # projection went down to d
    cert = got[case + ("/certify/scalars" if case.endswith("single") else "/certify_live/scalars")]
    lift = got[case + "/lift/scalars"]
    assert cert[0] == 0.0 and cert[1] < 0.0 and lift[0] == 1.0 and lift[6] == rec.R0 + 1
    if case.endswith("single"):
        assert got[case + "/project/scalars"][0] == 1.0 and got[case + "/project/basis"].shape[0] == rec.R0 + 1
