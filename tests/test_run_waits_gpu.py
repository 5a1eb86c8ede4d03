"""The one-launch tCG run (k_tcg_run), whose prologue requests the CSR entries, row pointers, poses and gradient image
ahead of the rows of the inverse, against the launches per iteration (DCORA_SOLVER_TCG=launch): bit for bit, on the
shapes where its gather and its grid step take every path (profiles/run_waits.txt: written for a gather that requested
the neighbours' old direction in front of the grid step, measured slower and taken out; the cases stay).

Graphs are an SE(3) chain plus loop closures around two hubs, the smallest shapes at which the gather takes each of its
paths: pose 5 has degree 9, so its three rotation rows hold 39 entries (Q keeps no structural zeros: 4 of the pose's own,
4 per edge that leaves it, 3 per edge that enters it) -- the batch of 24 and two chunks of 8 behind the step, the second
one partial; pose 20 has degree 6, rows of 27 entries: one partial chunk; every other row fits the batch.
  n =  33: an odd n, the last workgroup holds one pose, 17 of the 32 arrival shards are in use
  n = 161: 81 workgroups, every shard in use
  n = 2, 3: one workgroup (a grid step of one) and two, one of which holds a single pose
After a rejected step the next run starts from the same iterate with the directions of the run before left in both
buffers: the case with a smaller trust region has boundary exits after at most two inner iterations and rejected steps
(asserted on the launches, the reference here)."""
import os

import numpy as np
import pytest

import common  # noqa: F401

pytestmark = pytest.mark.gpu

HUBS = {5: [9, 12, 15, 18, 21, 24, 27], 20: [2, 7, 11, 30]}  # pose: the far ends of its loop closures
_graphs = {}


def _edges(n):
    edges = [(i, i + 1) for i in range(n - 1)]
    if n > 30:
        edges += [(h, j) for h, far in HUBS.items() for j in far]
    return edges


def _graph(n):
    """chain 0 - 1 - ... - n-1 plus the hubs' loop closures (n > 30); built once per n"""
    if n in _graphs:
        return _graphs[n]
    import dcora_amd as da
    rng = np.random.default_rng(7000 + n)

    def rot(scale):
        q, u = np.linalg.qr(np.eye(3) + scale * rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(u))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        return q

    Rg = [rot(0.8) for _ in range(n)]
    tg = [3.0 * rng.standard_normal(3) for _ in range(n)]
    ids, vals = [], []
    for i, j in _edges(n):
        Rij = Rg[i].T @ Rg[j] @ rot(0.05)
        tij = Rg[i].T @ (tg[j] - tg[i]) + 0.05 * rng.standard_normal(3)
        ids.append([0, i, 0, j])
        vals.append(np.r_[Rij.T.reshape(-1), tij, rng.uniform(50, 150), rng.uniform(5, 15), 1.0])
    ds = da.Dataset(3, n, np.array(ids), np.array(vals))
    Q = da.build_Q_pgo(ds)
    if n > 30:
        rows = np.diff(np.asarray(Q.rp))
        assert list(rows[20:23]) == [39] * 3 and list(rows[80:83]) == [27] * 3, (rows[20:24], rows[80:84])
        rows[20:23] = rows[80:83] = 0
        assert rows.max() <= 24, rows.max()   # every other row fits the batch
    _graphs[n] = (ds, Q)
    return _graphs[n]


def _start(r, n):
    import dcora_amd as da
    rng = np.random.default_rng(100 * n + r)
    k = 4 * n
    return 0.3 * rng.standard_normal((r, k)), da.manifold_project(r, 3, n, rng.uniform(-1, 1, (r, k)))


def _solve(form, r, n, prm, repeats=1):
    """[(X, result)] of `repeats` solves on one problem handle; form "launch" or None (the run form)"""
    import dcora_amd as da
    ds, Q = _graph(n)
    G, X = _start(r, n)
    if form:
        os.environ["DCORA_SOLVER_TCG"] = form
    try:
        P = da.QuadraticProblem(r, ds.d, n, Q, G=G)
    finally:
        os.environ.pop("DCORA_SOLVER_TCG", None)
    want = "two launches" if form else "one launch per run"
    assert P.solver_info()["tcg"] == want, (r, n, P.solver_info())
    out = []
    for _ in range(repeats):
        opt = da.QuadraticOptimizer(P, prm)
        Xs = opt.optimize(X)
        out.append((Xs, opt.getOptResult()))
        assert P.solver_info()["tcg"] == want   # (the run form did not give up)
    P.close()
    return out


KEYS = ("outer_iterations", "inner_iterations", "tCGStatus", "fOpt", "gradNormOpt")


def _same(a, b, what):
    (Xa, ra), (Xb, rb) = a, b
    for key in KEYS:
        assert ra[key] == rb[key], (what, key, ra[key], rb[key])
    assert np.array_equal(Xa, Xb), (what, np.abs(Xa - Xb).max())


def _params(long_runs, **kw):
    import dcora_amd as da
    if long_runs:
        kw.update(RTR_tCG_iterations=60, gradnorm_tol=1e-9)
    return da.ROptParameters(**kw)


@pytest.mark.parametrize("long_runs", [False, True])
@pytest.mark.parametrize("n", [33, 161])
@pytest.mark.parametrize("r", [4, 5, 6])
def test_hub_rows_are_bitwise_the_launches(built, r, n, long_runs):
    prm = _params(long_runs)
    a, b = _solve("launch", r, n, prm)[0], _solve(None, r, n, prm)[0]
    print("r %d n %d: outer %d inner %d status %s" % (r, n, b[1]["outer_iterations"], b[1]["inner_iterations"], b[1]["tCGStatus"]))
    assert b[1]["inner_iterations"] > 0
    _same(a, b, (r, n, long_runs))


@pytest.mark.parametrize("long_runs", [False, True])
@pytest.mark.parametrize("n", [2, 3])
def test_smallest_grids_are_bitwise_the_launches(built, n, long_runs):
    prm = _params(long_runs)
    a, b = _solve("launch", 5, n, prm)[0], _solve(None, 5, n, prm)[0]
    assert b[1]["inner_iterations"] > 0
    _same(a, b, (n, long_runs))


# the trust region at which the launches' first runs leave through the boundary after one or two inner iterations and a
# step is rejected (found with the CPU oracle's RTR on this graph; asserted below on the launch form itself)
EARLY_RADIUS = 30.0


def test_runs_that_end_early_and_refused_steps(built):
    r, n = 5, 33
    # the launch form one RTR iteration at a time: the differences are the single runs
    runs, prev = [], {"inner_iterations": 0, "accepted_steps": 0}
    for m in range(1, 7):
        res = _solve("launch", r, n, _params(False, RTR_iterations=m, RTR_initial_radius=EARLY_RADIUS))[0][1]
        if res["outer_iterations"] < m:
            break
        runs.append((res["inner_iterations"] - prev["inner_iterations"], res["tCGStatus"],
                     res["accepted_steps"] - prev["accepted_steps"]))
        prev = res
    print("launch form, (inner iterations, tCG status, accepted) per run:", runs)
    assert any(inner <= 2 and status in (0, 1) for inner, status, _ in runs), runs   # TR_NEGCURVTURE, TR_EXCREGION
    assert any(acc == 0 for _, _, acc in runs), runs
    prm = _params(False, RTR_iterations=6, RTR_initial_radius=EARLY_RADIUS)
    a, b = _solve("launch", r, n, prm)[0], _solve(None, r, n, prm)[0]
    assert a[1]["accepted_steps"] == b[1]["accepted_steps"]
    _same(a, b, "early exits")


def test_three_solves_on_one_handle_repeat(built):
    prm = _params(True)
    a = _solve("launch", 5, 161, prm)[0]
    for i, b in enumerate(_solve(None, 5, 161, prm, repeats=3)):
        _same(a, b, "solve %d" % i)
