"""The certificate's eigensolver states its thick-restart recurrence (lanczos_restart.h) and the plan of
computeMinimumEigenPair (min_eig_plan.h) once, for the one-GPU run, the row-block run of a job and the preconditioner's
regularisation.  That moved host code only -- no kernel, no launch order, no argument -- so every output must equal the
commit before: tests/golden/min_eig_parent.npz was written on an MI355X by tools/record_min_eig.py --lib <a library built
from that commit's own sources> --out ...; the tree's library must compute every array BIT FOR BIT.

The cases (tools/record_min_eig.py): dcora_cert_min_eig with the cycle kept on the device and in the per-step form
(DCORA_LANCZOS=sync; a child process each) on an indefinite certificate of smallGrid3D (r = 3, with its launch count),
the zero matrix, 2 I, a diagonal with three eigenvalues and its negative, lambda_min = -50 under 4e6 (the shortcut and
the outward ladder), single_drone minus 1e-3 I (the fallback's first shift) and 0.05 single_drone minus 1e-3 I (the
inward ladder); dcora_graph_precond_regularization on the agents' Q of range_aided_slam_test_2d; and two ranks sharing
the GPU (a process each) on tinyGrid3D / 3 agents and range_aided_slam_test_2d (scattered rows), certify and
certify_live at eta = 1e-3 and certify_live at eta = 1e-7.  A difference is a finding to explain, never a tolerance to
add."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
RECORD = os.path.join(HERE, "golden", "min_eig_parent.npz")

import record_min_eig as me  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(RECORD))


def test_the_record_holds_every_case(recorded):
    assert sorted({"/".join(k.split("/")[:2]) for k in recorded}) == sorted(me.CASES)
    for form in me.FORMS:
        assert {k.split("/")[2] for k in recorded if k.startswith("single/%s/" % form)} == set(me.MATRICES) | {"reg"}


def test_the_recorded_cases_take_the_branches_they_are_named_for(recorded):
    """with the parent's library (its DCORA_INIT_TIMING lines were read when the record was written): the negated
    diagonal is done after the first run (its 20 matvecs); the zero matrix too; the grid's spectrum-shifted run
    delivers (tol / lambda_lm = 1e-3 / 1166); the huge spectrum skips that run (no 10 000 matvecs) and its -50 lies
    below the first shift, which the Cholesky therefore refuses: -100 factors and converges in 20 solves; single_drone
    skips it too (ratio 5e-9) and its inverse run converges at the first shift after 3150 solves; scaled by 0.05 its
    spectrum-shifted run spends the 1000 restarts, and so do the inverse runs at -10, -5 and -2.5: the ladder moves
    INWARD and -1.25 converges after 7260 solves (the count returned holds the first two runs and the inverse run that
    delivered, 20 + 10 020 + 7260, not the three that did not); on two ranks the default eta is delivered collectively
    and the small one by rank 0's fallback"""
    for form in me.FORMS:
        s = {m: recorded["single/%s/%s/scalars" % (form, m)] for m in me.MATRICES}
        assert all(v[0] == 1.0 for v in s.values())
        assert s["neg_diag"][1] < 0 and s["neg_diag"][2] == 20 and s["zero"][1] == 0 and s["zero"][2] == 20
        assert s["grid"][1] < 0 and s["grid"][2] > 20
        assert s["huge"][1] < -10.0 and 20 < s["huge"][2] < 2000
        assert abs(s["drone"][1] + 1e-3) < 1e-8 and 20 < s["drone"][2] < 10020
        assert abs(s["drone_inward"][1] + 1e-3) < 1e-8 and 20 + 10020 < s["drone_inward"][2] < 20 + 2 * 10020
        assert recorded["single/%s/grid/launches" % form][0] > 0
    for w in me.rec.WORKLOADS:
        for tag, dist in (("certify", 1.0), ("certify_live", 1.0), ("certify_live_small", 0.0)):
            sc = recorded["ranks/%s/%s/scalars" % (w, tag)]
            assert sc[0] == 0.0 and sc[2] < 0.0 and sc[4] == dist, (w, tag, sc)


@pytest.mark.parametrize("case", me.CASES)
def test_every_array_is_bitwise_the_parents(built, recorded, case):
    """(the launch count of one min_eig call on the smallGrid3D certificate is one of the arrays)"""
    got = me.compute_case(case)
    want = {k: v for k, v in recorded.items() if k.startswith(case + "/")}
    assert want and sorted(got) == sorted(want)
    for k in sorted(want):
        same_shape = got[k].shape == want[k].shape
        print(k, "max |difference|", float(np.max(np.abs(got[k] - want[k]), initial=0.0)) if same_shape else "shapes differ")
    assert me.rec.differing(got, want) == []
