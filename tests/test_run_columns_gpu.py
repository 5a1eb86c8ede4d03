"""The one-launch tCG run (k_tcg_run) with its neighbours' columns fetched once per workgroup (the column-slot map of
dcora_amd/csrc/column_slots.h; the default) against the same run with every row gathering its own entries
(DCORA_GATHER=entries) and against the launches per iteration (DCORA_SOLVER_TCG=launch): bit for bit on X and on the
result keys tests/test_run_waits_gpu.py compares, on that module's hub graphs and on the shapes at which the map itself
takes another path:
  closures i -> i + 2 for even i: the two poses of a workgroup share neighbours (one column block serves both)
  a hub of 17 neighbours: its workgroup names more pose blocks than a list holds, so the problem's runs gather entry by
      entry (asserted through gather_info: the map says one workgroup overflows, the others do not)
  the largest star whose workgroup still fits the run's staging of CSR entries: the same fall-back at the other limit
The launch form is the reference of every case and is computed once per case."""
import os

import numpy as np
import pytest

import common  # noqa: F401
from test_run_waits_gpu import EARLY_RADIUS, KEYS
from test_run_waits_gpu import _graph as _hub_graph

pytestmark = pytest.mark.gpu

_graphs, _reference = {}, {}


def _edges(kind, n):
    edges = [(i, i + 1) for i in range(n - 1)]
    if kind == "shared":
        edges += [(i, i + 2) for i in range(0, n - 2, 2)]
    elif kind == "overflow":    # pose 20 with 17 neighbours: 18 pose blocks with its own, 19 with its partner's
        edges += [(20, j) for j in range(22, 37)]
    elif isinstance(kind, tuple):   # ("star", degree): pose 2 and `degree` far ends
        edges += [(2, j) for j in range(4, 4 + kind[1] - 2)]
    return edges


def _graph(kind, n):
    """an SE(3) chain plus the closures of `kind`, as tests/test_run_waits_gpu.py draws its measurements; "hubs": that
    module's own graph (pose 5 of degree 9, pose 20 of degree 6)"""
    if kind == "hubs":
        return _hub_graph(n)
    if (kind, n) in _graphs:
        return _graphs[(kind, n)]
    import dcora_amd as da
    rng = np.random.default_rng(9000 + n + len(str(kind)))

    def rot(scale):
        q, u = np.linalg.qr(np.eye(3) + scale * rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(u))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        return q

    Rg = [rot(0.8) for _ in range(n)]
    tg = [3.0 * rng.standard_normal(3) for _ in range(n)]
    ids, vals = [], []
    for i, j in _edges(kind, n):
        Rij = Rg[i].T @ Rg[j] @ rot(0.05)
        tij = Rg[i].T @ (tg[j] - tg[i]) + 0.05 * rng.standard_normal(3)
        ids.append([0, i, 0, j])
        vals.append(np.r_[Rij.T.reshape(-1), tij, rng.uniform(50, 150), rng.uniform(5, 15), 1.0])
    ds = da.Dataset(3, n, np.array(ids), np.array(vals))
    _graphs[(kind, n)] = (ds, da.build_Q_pgo(ds))
    return _graphs[(kind, n)]


def _start(r, n):
    import dcora_amd as da
    rng = np.random.default_rng(100 * n + r)
    return 0.3 * rng.standard_normal((r, 4 * n)), da.manifold_project(r, 3, n, rng.uniform(-1, 1, (r, 4 * n)))


ENV = {"launch": {"DCORA_SOLVER_TCG": "launch"}, "entries": {"DCORA_GATHER": "entries"}, "columns": {}}


def _solve(form, kind, r, n, prm, repeats=1, gather=None, with_G=True):
    """[(X, result)] of `repeats` solves on one handle; gather: what gather_info says the run form does (None: what the
    form asks for)"""
    import dcora_amd as da
    ds, Q = _graph(kind, n)
    G, X = _start(r, n)
    os.environ.update(ENV[form])
    try:
        P = da.QuadraticProblem(r, ds.d, n, Q, G=G if with_G else None)
    finally:
        for key in ENV[form]:
            os.environ.pop(key, None)
    want = "two launches" if form == "launch" else "one launch per run"
    assert P.solver_info()["tcg"] == want, (form, r, n, P.solver_info())
    info = P.gather_info()
    if form != "launch":
        assert info["gather"] == (gather or form), (form, info)
        assert info["map"] == (form == "columns")
    out = []
    for _ in range(repeats):
        opt = da.QuadraticOptimizer(P, prm)
        Xs = opt.optimize(X)
        out.append((Xs, opt.getOptResult()))
        assert P.solver_info()["tcg"] == want   # (the run form did not give up)
    P.close()
    return out, info


def _same(a, b, what):
    (Xa, ra), (Xb, rb) = a, b
    for key in KEYS:
        assert ra[key] == rb[key], (what, key, ra[key], rb[key])
    assert np.array_equal(Xa, Xb), (what, np.abs(Xa - Xb).max())


def _params(long_runs, **kw):
    import dcora_amd as da
    if long_runs:
        kw.update(RTR_tCG_iterations=60, gradnorm_tol=1e-9)
    return da.ROptParameters(**kw), tuple(sorted(kw.items()))


def _three_forms(kind, r, n, long_runs, gather=None, **kw):
    """the launches (once per case), the run with its own entries, the run with the column lists: all the same"""
    prm, key = _params(long_runs, **kw)
    ref = _reference.setdefault((kind, r, n, key), _solve("launch", kind, r, n, prm)[0][0])
    (ent,), _ = _solve("entries", kind, r, n, prm)
    (col,), info = _solve("columns", kind, r, n, prm, gather=gather)
    assert col[1]["inner_iterations"] > 0
    _same(ref, ent, (kind, r, n, "entries against the launches"))
    _same(ref, col, (kind, r, n, "columns against the launches"))
    return ref, info


@pytest.mark.parametrize("long_runs", [False, True])
@pytest.mark.parametrize("n", [33, 161])
@pytest.mark.parametrize("r", [4, 5, 6])
def test_hub_graphs_are_bitwise_the_entries_and_the_launches(built, r, n, long_runs):
    ref, info = _three_forms("hubs", r, n, long_runs)
    assert info["overflow"] == 0 and info["workgroups"] == (n + 1) // 2
    assert info["max_poses"] >= 10   # pose 5 names itself and its 9 neighbours


@pytest.mark.parametrize("long_runs", [False, True])
@pytest.mark.parametrize("n", [2, 3])
def test_smallest_grids(built, n, long_runs):
    _, info = _three_forms("chain", 5, n, long_runs)
    assert info["max_poses"] == n


@pytest.mark.parametrize("r", [4, 5, 6])
def test_two_poses_of_a_workgroup_share_their_neighbours(built, r):
    _, info = _three_forms("shared", r, 33, True)
    assert info["overflow"] == 0 and info["max_poses"] == 5   # i - 2 .. i + 2 for the pair (i, i + 1), i even


def test_a_workgroup_that_overflows_sends_the_runs_to_the_entries(built):
    """pose 20 names 18 pose blocks, a list holds 16: the map flags that workgroup alone, and the problem's runs gather
    entry by entry -- on every workgroup, so that neither kernel carries both gathers"""
    _, info = _three_forms("overflow", 5, 41, True, gather="entries")
    assert info["map"] and info["overflow"] == 1 and info["workgroups"] == 21 and info["max_poses"] >= 18


def test_the_largest_star_the_run_form_admits(built):
    """the most neighbours at which the CSR entries of the hub's workgroup still fit the run's staging (1024 entries):
    one more and the problem solves on the launches"""
    import dcora_amd as da
    n, cap = 80, 1024

    def rows_nnz(deg):
        rp = np.asarray(_graph(("star", deg), n)[1].rp)
        return max(rp[min(n, p + 2) * 4] - rp[p * 4] for p in range(0, n, 2))

    deg = max(d for d in range(20, 77) if rows_nnz(d) <= cap)
    assert rows_nnz(deg + 1) > cap and deg + 6 <= n
    ds, Q = _graph(("star", deg + 1), n)
    P = da.QuadraticProblem(5, 3, n, Q)
    assert P.solver_info()["tcg"] == "two launches"
    P.close()
    _, info = _three_forms(("star", deg), 5, n, False, gather="entries")
    assert info["overflow"] >= 1 and info["max_poses"] >= deg + 1


def test_runs_that_end_early_and_refused_steps(built):
    ref, _ = _three_forms("hubs", 5, 33, False, RTR_iterations=6, RTR_initial_radius=EARLY_RADIUS)
    assert ref[1]["accepted_steps"] < ref[1]["outer_iterations"]   # a step was refused (test_run_waits_gpu.py shows which)


def test_three_solves_on_one_handle_repeat(built):
    prm, key = _params(True)
    ref = _reference.setdefault(("hubs", 5, 161, key), _solve("launch", "hubs", 5, 161, prm)[0][0])
    for i, b in enumerate(_solve("columns", "hubs", 5, 161, prm, repeats=3)[0]):
        _same(ref, b, "solve %d" % i)


def test_a_problem_reranked_into_the_run_form_builds_its_map(built):
    """created at r = 3, where there is no run form and no map, and taken to r = 5 in place (what a session's lift does to
    its agents' problems): the map is built from the pattern on the device, the runs fetch columns, and the solve is
    bitwise that of problems created at r = 5 on the launches, with the entries' gather and with the column lists"""
    import dcora_amd as da
    r, n = 5, 33
    ds, Q = _graph("hubs", n)
    prm, _ = _params(True)
    X = _start(r, n)[1]
    P = da.QuadraticProblem(3, ds.d, n, Q)
    before = P.gather_info()
    assert P.solver_info()["tcg"] != "one launch per run" and not before["map"] and before["gather"] == "entries"
    P.debug_rerank(r)
    after = P.gather_info()
    assert P.solver_info()["tcg"] == "one launch per run"
    assert after["map"] and after["gather"] == "columns" and after["overflow"] == 0 and after["workgroups"] == 17
    opt = da.QuadraticOptimizer(P, prm)
    got = (opt.optimize(X), opt.getOptResult())
    assert P.solver_info()["tcg"] == "one launch per run" and got[1]["inner_iterations"] > 0
    P.close()
    for form in ("launch", "entries", "columns"):
        (ref,), _ = _solve(form, "hubs", r, n, prm, with_G=False)
        _same(ref, got, "reranked against a problem created at r = 5, " + form)
