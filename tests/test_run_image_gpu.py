"""The one-launch tCG run (k_tcg_run) with its padded LDS image, its row sums requested ahead of the all-gather and its
done words published by a whole wave, against the launches per iteration (DCORA_SOLVER_TCG=launch): bit for bit.

Graphs are an SE(3) chain with a few seeded loop closures, at the sizes where the kernel takes another path:
  n =  33, k =  132, 2 steps: an odd n, the last workgroup holds one pose; waves 2, 3 never take a step
  n = 161, k =  644, 6 steps: waves 0, 1 take two steps, the others one
  n = 500, k = 2000, 16 steps: the headline geometry, 250 workgroups; every pad of the image is crossed in every step
r = 4, 5, 6, with the default parameters and with long runs (60 inner iterations, gradnorm_tol 1e-9)."""
import os

import numpy as np
import pytest

import common  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [33, 161, 500]
_graphs = {}


def _graph(n):
    """chain 0 - 1 - ... - n-1 plus n // 8 + 2 loop closures between seeded pairs; built once per n"""
    if n in _graphs:
        return _graphs[n]
    import dcora_amd as da
    rng = np.random.default_rng(4000 + n)

    def rot(scale):
        q, u = np.linalg.qr(np.eye(3) + scale * rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(u))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        return q

    Rg = [rot(0.8) for _ in range(n)]
    tg = [3.0 * rng.standard_normal(3) for _ in range(n)]
    edges = [(i, i + 1) for i in range(n - 1)]
    seen = set(edges)
    while len(edges) < n - 1 + n // 8 + 2:
        i, j = sorted(rng.integers(0, n, 2).tolist())
        if j - i > 1 and (i, j) not in seen:
            seen.add((i, j))
            edges.append((i, j))
    ids, vals = [], []
    for i, j in edges:
        Rij = Rg[i].T @ Rg[j] @ rot(0.05)
        tij = Rg[i].T @ (tg[j] - tg[i]) + 0.05 * rng.standard_normal(3)
        ids.append([0, i, 0, j])
        vals.append(np.r_[Rij.T.reshape(-1), tij, rng.uniform(50, 150), rng.uniform(5, 15), 1.0])
    ds = da.Dataset(3, n, np.array(ids), np.array(vals))
    _graphs[n] = (ds, da.build_Q_pgo(ds))
    return _graphs[n]


@pytest.mark.parametrize("long_runs", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("r", [4, 5, 6])
def test_run_form_is_bitwise_the_launches(built, r, n, long_runs):
    import dcora_amd as da
    ds, Q = _graph(n)
    k = (ds.d + 1) * n
    assert (k + 127) // 128 == {33: 2, 161: 6, 500: 16}[n]
    rng = np.random.default_rng(100 * n + r)
    G = 0.3 * rng.standard_normal((r, k))
    X = da.manifold_project(r, ds.d, n, rng.uniform(-1, 1, (r, k)))
    prm = da.ROptParameters(RTR_tCG_iterations=60, gradnorm_tol=1e-9) if long_runs else da.ROptParameters()
    got = {}
    for form in ("launch", None):
        if form:
            os.environ["DCORA_SOLVER_TCG"] = form
        try:
            P = da.QuadraticProblem(r, ds.d, n, Q, G=G)
        finally:
            os.environ.pop("DCORA_SOLVER_TCG", None)
        want = "two launches" if form else "one launch per run"
        assert P.solver_info()["tcg"] == want, (r, n, P.solver_info())
        opt = da.QuadraticOptimizer(P, prm)
        Xs = opt.optimize(X)
        got[form] = (Xs, opt.getOptResult())
        assert P.solver_info()["tcg"] == want   # (the run form did not give up)
        P.close()
    (Xa, ra), (Xb, rb) = got["launch"], got[None]
    print("r %d n %d: outer %d inner %d status %s" % (r, n, rb["outer_iterations"], rb["inner_iterations"], rb["tCGStatus"]))
    for key in ("outer_iterations", "inner_iterations", "tCGStatus", "fOpt", "gradNormOpt"):
        assert ra[key] == rb[key], (r, n, key, ra[key], rb[key])
    assert rb["inner_iterations"] > 0
    assert np.array_equal(Xa, Xb), np.abs(Xa - Xb).max()
