"""k_fused_grad requests its independent loads together and ahead of the gate test (the same was built for k_rtr_init,
k_rtr_decide, k_eval_finish and k_g_nesterov, which these cases cover as well); only WHEN a load is issued may differ
from the commit before, never what is added to what.  The existing differential tests compare forms that share these kernels, so this
one pins bits to a record of that commit: tests/golden/eval_chains_parent.npz was written on an MI355X by
tools/record_eval_chains.py --lib <a library built from that commit's own sources> --out ...; it holds what that
library computed on the cases below, and the tree's library must compute every array BIT FOR BIT.  The same tool with
--check passed against both libraries (profiles/eval_chains.txt, section 3).

The cases (tools/record_eval_chains.py, compute(); computed once per test session):
  chain/...      9-pose SE(3) chains with a hub (rows of 35 entries: more than the gather's first batch of 24) and
                 without (rows of at most 11), r = 4 and 5, random G; default parameters, long tCG runs, large initial
                 radii (rejected RTR steps: both branches of k_rtr_decide), a solve from a converged iterate
                 (k_rtr_init ends it; everything queued behind is gated off) and one of the same problem after it
  two_pass/...   100 poses, pose 5 sees every other one: the first k_fused_grad workgroup stages 1869 entries, more
                 than kHessTile = 1536 (a second tile pass), and no row is a long row (399 <= 512)
  session/...    smallGrid3D over 2 agents (62 / 63 poses), r = 5 and 4, restart_interval = 4, 12 iterations -- plain
                 rounds, restart rounds, the round after -- and the 6-pose planar graph over 2 agents (k_fused_grad<2>),
                 each with the default chain (G rides in the evaluation) and with DCORA_CHAIN=launches
Every case asserts the path it is meant for: the solves' tCG form inside compute(), the sessions' launches here."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
RECORD = os.path.join(HERE, "golden", "eval_chains_parent.npz")
RESULT = {k: i for i, k in enumerate(("fInit", "fOpt", "gradNormInit", "gradNormOpt", "outer_iterations",
                                      "inner_iterations", "accepted_steps", "tCGStatus"))}


@pytest.fixture(scope="module")
def computed(built):
    import record_eval_chains
    return record_eval_chains.compute()


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(RECORD))


def _equal_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("family", ["chain/", "two_pass/", "session/smallGrid3D/", "session/planar/"])
def test_every_array_is_bitwise_the_parents(computed, recorded, family):
    names = sorted(k for k in recorded if k.startswith(family))
    assert names and names == sorted(k for k in computed if k.startswith(family))
    for k in names:
        print(k, "max |difference|", float(np.max(np.abs(computed[k] - recorded[k]))) if computed[k].shape ==
              recorded[k].shape else "shapes differ")
        assert _equal_bits(computed[k], recorded[k]), k


def test_the_solves_hold_rejected_steps_and_an_early_exit(computed):
    res = {k: v for k, v in computed.items() if k.endswith("/result")}
    rejected = [k for k, v in res.items() if v[RESULT["accepted_steps"]] < v[RESULT["outer_iterations"]]]
    accepted = [k for k, v in res.items() if v[RESULT["accepted_steps"]] > 0]
    print("solves with rejected steps:", rejected)
    assert rejected and accepted
    early = computed["chain/hub/r5/converged/result"]
    assert early[RESULT["outer_iterations"]] == 0 and early[RESULT["inner_iterations"]] == 0
    assert _equal_bits(computed["chain/hub/r5/converged/X"], computed["chain/hub/r5/default/X"])  # nothing moved
    after = computed["chain/hub/r5/after_converged/result"]
    assert after[RESULT["outer_iterations"]] > 0 and after[RESULT["inner_iterations"]] > 0


@pytest.mark.parametrize("r", [5, 4])
def test_the_sessions_ran_the_chain_they_are_meant_for(computed, r):
    """a plain accelerated round enqueues k_g_nesterov, [G], evaluation, k_rtr_init, three RTR iterations x [run,
    evaluation, decision], k_g_nesterov, evaluation, epilogue: 15 launches, 16 with G as a launch of its own
    (tests/test_rbcd_chain_gpu.py::test_launches_per_round); with restart_interval = 4 every fourth round, counted from
    the third, restarts and solves a second time: 27 or 28"""
    for chain, plain, restart in (("ride", 15, 27), ("launches", 16, 28)):
        sc = computed["session/smallGrid3D/r%d/%s/scalars" % (r, chain)]
        assert sc[:, 4].astype(int).tolist() == [3] * 12  # (three RTR iterations in every local solve)
        want = [restart if it % 4 == 2 else plain for it in range(12)]
        assert sc[:, 3].astype(int).tolist() == want, (chain, sc[:, 3].tolist())
        assert len(set(sc[:, 2].tolist())) > 1  # (more than one agent was selected)


def test_the_planar_session_forms_g_in_the_evaluation(computed):
    """d = 2 has no one-launch tCG run (k_tcg_run is built for d = 3), so a planar round is not the 15-launch chain: its
    tCG iterations are launches of their own, 33 per round here.  What puts the session on k_fused_grad<2, true> is that
    the default chain enqueues exactly one launch less per round -- k_spmm's G -- than DCORA_CHAIN=launches."""
    a, b = computed["session/planar/r3/ride/scalars"], computed["session/planar/r3/launches/scalars"]
    assert np.array_equal(b[:, 3] - a[:, 3], np.ones(len(a))), (a[:, 3].tolist(), b[:, 3].tolist())
