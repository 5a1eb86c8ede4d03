"""The team rules on the host (dcora_team_params_default / dcora_team_ready_to_terminate / dcora_team_decide; no
device): the reference's defaults (ref include/DCORA/Agent.h:113-125) and, over seeded random inputs and the edge
cases, the decisions of the Python restatement of src/Agent.cpp:567-585, 1123-1156, 1280-1330 (team_rules_ref.py)."""
import itertools

import numpy as np
import pytest

import team_rules_ref as ref


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    return dcora_amd


def test_defaults_are_the_references(da):
    assert da.team_params().as_dict() == dict(max_num_iters=500, rel_change_tol=5e-3, robust_opt_num_weight_updates=10,
                                              robust_opt_num_resets=0, robust_opt_inner_iters=30,
                                              robust_opt_min_convergence_ratio=0.8)


def _status(q, it, ready, state=ref.INITIALIZED, rel=0.0):
    return dict(agent_id=q, state=state, instance_number=0, iteration_number=it, ready_to_terminate=int(ready),
                relative_change=rel)


def _both(da, p, robust, it, wuc, inner, latest, statuses, active=None):
    got = da.team_decide(p, robust, it, wuc, inner, latest, statuses, active)
    want = (ref.should_terminate(p, robust, it, wuc, statuses, active),
            ref.should_update_weights(p, robust, wuc, inner, latest, statuses, active))
    assert got == want, (robust, it, wuc, inner, latest, statuses, active)
    return got


def test_ready_to_terminate_equals_the_restatement(da):
    rng = np.random.default_rng(11)
    p = da.team_params()
    cases = []
    for _ in range(3000):
        total = int(rng.integers(0, 12))
        acc = int(rng.integers(0, total + 1))
        rej = int(rng.integers(0, total - acc + 1))
        rel = float(rng.choice([0.0, 4e-3, 5e-3, np.nextafter(5e-3, 1), 1.0, 5.0, np.nextafter(5.0, 6), 7.0,
                                rng.uniform(0, 8)]))
        cases.append((bool(rng.integers(2)), int(rng.integers(0, 3)), bool(rng.integers(2)), rel, acc, rej, total))
    # edges: no loop closures at all (0 / 0 passes), the ratio exactly at the bound, the loose tolerance of the first
    # robust round, a failed optimisation
    cases += [(False, 0, True, 0.0, 0, 0, 0), (True, 0, True, 4.9, 0, 0, 0), (True, 1, True, 4.9, 0, 0, 0),
              (False, 0, True, 4.9, 0, 0, 0), (False, 0, True, 0.0, 4, 4, 10), (False, 0, True, 0.0, 4, 3, 10),
              (False, 0, False, 0.0, 5, 5, 10), (True, 0, True, 5.0, 1, 0, 1), (True, 0, True, 5.000001, 1, 0, 1)]
    seen = set()
    for c in cases:
        got = da.team_ready_to_terminate(p, *c)
        assert got == ref.ready_to_terminate(p, *c), c
        seen.add(got)
    assert seen == {True, False}
    assert da.team_ready_to_terminate(p, False, 0, True, 0.0, 0, 0, 0)
    assert not da.team_ready_to_terminate(p, False, 0, True, 0.0, 4, 3, 10)
    assert da.team_ready_to_terminate(da.team_params(robust_opt_min_convergence_ratio=0.7), False, 0, True, 0.0, 4, 3, 10)


def test_decide_equals_the_restatement_on_random_inputs(da):
    rng = np.random.default_rng(12)
    seen = set()
    for _ in range(4000):
        R = int(rng.integers(1, 7))
        p = da.team_params(max_num_iters=int(rng.integers(1, 40)), robust_opt_num_weight_updates=int(rng.integers(0, 4)),
                           robust_opt_inner_iters=int(rng.integers(1, 8)))
        latest = int(rng.integers(0, 30))
        statuses = []
        for q in range(R):
            if rng.random() < 0.15:
                statuses.append(None)
            else:
                state = ref.INITIALIZED if rng.random() < 0.9 else int(rng.integers(0, 2))
                statuses.append(_status(q, int(rng.integers(0, 40)), rng.random() < 0.8, state))
        active = None if rng.random() < 0.5 else [int(rng.random() < 0.8) for _ in range(R)]
        seen.add(_both(da, p, bool(rng.integers(2)), int(rng.integers(0, 45)), int(rng.integers(0, 5)),
                       int(rng.integers(0, 10)), latest, statuses, active))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_decide_edge_cases(da):
    p = da.team_params(max_num_iters=50, robust_opt_num_weight_updates=3, robust_opt_inner_iters=5)
    ready = [_status(q, 10, True) for q in range(3)]
    # L2: terminates when all are ready, never re-weights
    assert _both(da, p, False, 10, 0, 99, 0, ready) == (True, False)
    # robust: no termination below the number of weight updates (0, below, at the limit); the update stops at it
    assert _both(da, p, True, 10, 0, 0, 0, ready) == (False, True)
    assert _both(da, p, True, 10, 2, 0, 0, ready) == (False, True)
    assert _both(da, p, True, 10, 3, 0, 0, ready) == (True, False)
    assert _both(da, p, True, 10, 3, 99, 0, ready) == (True, False)
    # the inner counter below / at the cap, with a team that is not ready
    busy = [_status(0, 10, True), _status(1, 10, False), _status(2, 10, True)]
    assert _both(da, p, True, 10, 1, 4, 0, busy) == (False, False)
    assert _both(da, p, True, 10, 1, 5, 0, busy) == (False, True)
    # a missing status
    missing = [ready[0], None, ready[2]]
    assert _both(da, p, False, 10, 0, 0, 0, missing) == (False, False)
    assert _both(da, p, True, 10, 1, 0, 0, missing) == (False, False)
    # a status older than the latest weight update: no update, but termination does not look at its age
    assert _both(da, p, True, 12, 1, 0, 11, ready) == (False, False)
    assert _both(da, p, True, 12, 1, 0, 10, ready) == (False, True)
    assert _both(da, p, True, 12, 3, 0, 11, ready) == (True, False)
    # an inactive robot with a missing status is skipped
    assert _both(da, p, False, 10, 0, 0, 0, missing, [1, 0, 1]) == (True, False)
    assert _both(da, p, True, 10, 1, 0, 0, missing, [1, 0, 1]) == (False, True)
    assert _both(da, p, False, 10, 0, 0, 0, missing, [1, 1, 0]) == (False, False)
    # a robot that is not initialised
    waiting = [ready[0], _status(1, 10, True, state=1), ready[2]]
    assert _both(da, p, False, 10, 0, 0, 0, waiting) == (False, False)
    assert _both(da, p, True, 10, 1, 0, 0, waiting) == (False, False)
    # the iteration number at max_num_iters ends everything, whatever the statuses
    assert _both(da, p, False, 49, 0, 0, 0, missing) == (False, False)
    assert _both(da, p, False, 50, 0, 0, 0, missing) == (True, False)
    assert _both(da, p, True, 50, 0, 0, 0, [None] * 3) == (True, False)
    for robust, wuc, inner in itertools.product((False, True), (0, 2, 3), (0, 5)):
        _both(da, p, robust, 10, wuc, inner, 0, ready)
