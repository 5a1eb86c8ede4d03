"""The RBCD iteration with G = X C of the selected agent formed by the start-point evaluation of its local solve
(k_fused_grad, the default chain) against every step as a launch of its own (DCORA_CHAIN=launches, read when a session
is created, so both live side by side in one process): k_spmm's sums in k_spmm's order, so everything a caller can see
is the same BIT FOR BIT."""
import os

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

ITERS = 12


def _session(da, ds, R, r, chain, **kw):
    if chain is not None:
        os.environ["DCORA_CHAIN"] = chain
    try:
        return da.RbcdSession(ds, num_robots=R, r=r, **kw)
    finally:
        os.environ.pop("DCORA_CHAIN", None)


def _blocks_take_the_run_form(da, ds, R, r):
    """the agents' local problems at these sizes solve on the one-launch tCG run (the chain the issue is about)"""
    import bench
    for b in sorted({0, R - 1}):
        nb, ids, vals = bench.agent_block(ds, R, b)
        P = da.QuadraticProblem(r, ds.d, nb, da.build_Q_pgo(ds, n=nb, agent=b, ids=ids, vals=vals))
        info = P.solver_info()
        P.close()
        assert info["tcg"] == "one launch per run", (R, r, b, info)


def _trace(s, X0, iters):
    s.set_X(X0)
    out, sel = [], 0
    for _ in range(iters):
        c2, gn, bn, nxt = s.iterate(sel)
        out.append((s.get_X(), c2, gn, bn.copy(), nxt))
        sel = nxt
    return out


@pytest.mark.parametrize("name,R,r", [("smallGrid3D", 2, 5), ("smallGrid3D", 2, 4), ("sphere2500", 5, 5)])
def test_sessions_are_bitwise_the_launches(built, name, R, r):
    """12 iterations from a seeded random start with restart_interval = 4 -- plain rounds, restart rounds (whose second
    solve reads the G the first one's evaluation stored) and the round after a restart -- on smallGrid3D over 2 agents
    (62 / 63 poses: a last k_fused_grad workgroup that is not full) and on the headline split: X, 2 f, |grad|, the
    block norms and the next selected agent after every iterate"""
    import dcora_amd as da
    ds = common.product_dataset(name)
    _blocks_take_the_run_form(da, ds, R, r)
    X0 = common.random_point(r, ds.d, ds.n, 3, da.manifold_project)
    got = {}
    for chain in ("launches", None):
        s = _session(da, ds, R, r, chain, restart_interval=4)
        got[chain] = _trace(s, X0, ITERS)
        s.close()
    for it, (a, b) in enumerate(zip(got["launches"], got[None])):
        assert a[1] == b[1] and a[2] == b[2] and a[4] == b[4], (it, a[1:], b[1:])
        assert np.array_equal(a[3], b[3]), (it, a[3], b[3])
        assert np.array_equal(a[0], b[0]), (it, np.abs(a[0] - b[0]).max())
    assert len({t[4] for t in got[None]}) > 1  # (more than one agent was selected)


def test_phases_called_one_by_one_see_the_same_state(built):
    """the phases called one by one, with get_X and pack_public_dev between phase_selected and the evaluation, mixed
    with whole iterations: the same X, packed poses and evaluations as under the chain of launches"""
    import dcora_amd as da
    from test_exchange_gpu import Hip
    ds = common.product_dataset("smallGrid3D")
    R, r = 2, 5
    hip = Hip()
    X0 = common.random_point(r, ds.d, ds.n, 3, da.manifold_project)
    got = {}
    for chain in ("launches", None):
        s = _session(da, ds, R, r, chain, restart_interval=4)
        s.set_X(X0)
        sel, seen = 0, []
        for it in range(6):
            if it % 2 == 0:
                sel = s.iterate(sel)[3]
                continue
            s.phase_nonselected(sel)
            s.phase_selected(sel)
            X = s.get_X()
            packed = np.zeros(max(s.public_count(sel), 1) * (ds.d + 1) * r)
            buf = hip.malloc(packed.nbytes)
            s.pack_public_dev(sel, buf)
            s.synchronize()
            hip.d2h(packed, buf, packed.nbytes)
            hip.free(buf)
            c2, gn, bn, nxt = s.evaluate()
            seen.append((X, packed, c2, gn, nxt))
            sel = nxt
        seen.append((s.get_X(),))
        got[chain] = seen
        s.close()
    for a, b in zip(got["launches"], got[None]):
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y))


def test_launches_per_round(built):
    """the debug counter: a plain accelerated round whose local solve takes three RTR iterations enqueues one launch
    less -- k_spmm (G) -- than the chain of launches"""
    import dcora_amd as da
    ds = common.product_dataset("sphere2500")
    R, r = 5, 5
    X0 = common.random_point(r, ds.d, ds.n, 3, da.manifold_project)
    per_round = {}
    for chain in ("launches", None):
        s = _session(da, ds, R, r, chain)
        s.set_X(X0)
        sel = 0
        for _ in range(2):
            sel = s.iterate(sel)[3]
        n0 = s.debug_launches()
        s.iterate(sel)
        per_round[chain] = s.debug_launches() - n0
        assert s.last_result()["outer_iterations"] == 3
        s.close()
    # k_g_nesterov, G, evaluation, k_rtr_init, 3 x [run, evaluation, decision], k_g_nesterov, evaluation, epilogue
    assert per_round["launches"] == 16, per_round
    assert per_round[None] == 15, per_round
