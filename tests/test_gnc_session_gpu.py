"""Robust weights updated inside a live RBCD session (dcora_rbcd_create_robust / update_weights / set_weights,
Agent::initializeRobustOptimization and updateMeasurementWeights, ref src/Agent.cpp:1332-1346, 1397-1441):
creation equals the plain session, the device weights equal the host's RobustCost, an in-place weight change equals a
fresh session built with those weights, cached preconditioner images stay intact, and the one-session GNC flow
rejects exactly the injected outliers."""

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

GNC = dict(GNCBarc=10.0, GNCMuStep=2.0)  # as tests/test_gnc_distributed.py


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    if dcora_amd.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return dcora_amd


def _with_outliers(ds_cls, base, n_out, seed):
    # (copied from tests/test_gnc_distributed.py)
    rng = np.random.default_rng(seed)
    d, n = base.d, base.n
    ids, vals = [base.ids], [base.vals]
    for _ in range(n_out):
        i = int(rng.integers(0, n - 10))
        j = int(rng.integers(i + 5, n))
        Q = np.linalg.qr(rng.standard_normal((d, d)))[0]
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        row = np.concatenate([Q.reshape(-1, order="F"), 5.0 * rng.standard_normal(d), [12.5, 100.0, 1.0]])
        ids.append(np.array([[0, i, 0, j]], np.int32))
        vals.append(row[None, :])
    return ds_cls(d, n, np.vstack(ids), np.vstack(vals))


def _copy(da, ds, w=None):
    c = da.Dataset(ds.d, ds.n, ds.ids.copy(), ds.vals.copy())
    if w is not None:
        c.vals[:, -1] = w
    return c


def _start(da, ds, r, seed=3):
    return common.random_point(r, ds.d, ds.n, seed, da.manifold_project)


def _same_run(a, b):
    assert np.array_equal(a["selected"], b["selected"])
    assert np.array_equal(a["cost"], b["cost"]), np.abs(a["cost"] - b["cost"]).max()
    assert np.array_equal(a["gradnorm"], b["gradnorm"])


@pytest.mark.parametrize("name,R", [("smallGrid3D", 5), ("sphere2500", 5)])
def test_creation_equals_the_plain_session(da, name, R):
    """weight 1 on every loop closure at creation: the same matrices, the same 35 iterations (the restart at 30)"""
    from dcora_amd import driver
    from dcora_amd import robust as rb
    ds = common.product_dataset(name)
    lc = driver.loop_closure_mask(ds, R)
    rng = np.random.default_rng(5)
    given = _copy(da, ds)
    given.vals[lc, -1] = rng.uniform(0.2, 0.9, int(lc.sum()))  # initializeRobustOptimization overrides these
    ones = _copy(da, ds)
    ones.vals[lc, -1] = 1.0
    X0 = _start(da, ds, 5)
    A = da.RbcdSession(given, num_robots=R, r=5, robust=rb.RobustCostParameters("GNC_TLS"))
    P = da.RbcdSession(ones, num_robots=R, r=5)
    outs, Xs = [], []
    for s in (A, P):
        s.set_X(X0)
        outs.append(s.run(max_iters=35, rgrad_tol=0.0))
        Xs.append(s.get_X())
    _same_run(*outs)
    assert np.array_equal(Xs[0], Xs[1])
    assert np.array_equal(A.get_weights(), ones.vals[:, -1])
    assert A.robust_info()["updates"] == 0
    A.close()
    P.close()


def _check_weights(da, ds, X, lc_upd, w_before, w, counts, params, updates):
    from dcora_amd import robust as rb
    e = rb.measurement_errors(ds, X)
    exp = w_before.copy()
    exp[lc_upd] = rb.robust_weights(np.sqrt(e[lc_upd]), params, num_updates=updates)
    cls = lambda v: np.where(v < 1e-8, 0, np.where(v > 1 - 1e-8, 2, 1))
    assert np.array_equal(cls(w), cls(exp))
    assert np.abs(w - exp).max() <= 1e-14
    assert np.array_equal(w[~lc_upd], w_before[~lc_upd])  # odometry and fixed weights untouched
    c = cls(w[lc_upd])
    assert counts == {"accepted": int(np.sum(c == 2)), "rejected": int(np.sum(c == 0)),
                      "undecided": int(np.sum(c == 1))}
    assert sum(counts.values()) == int(lc_upd.sum())


@pytest.mark.parametrize("cost", ["L2", "L1", "TLS", "Huber", "GM", "GNC_TLS"])
def test_weights_equal_the_hosts(da, cost):
    from dcora_amd import driver
    from dcora_amd import robust as rb
    R, r = 5, 5
    ds = _with_outliers(da.Dataset, common.product_dataset("smallGrid3D"), 12, seed=2)
    lc = driver.loop_closure_mask(ds, R)
    fixed = np.zeros(ds.m, bool)
    fixed[np.nonzero(lc)[0][::7]] = True  # every seventh loop closure keeps its (non-unit) weight
    ds.vals[fixed, -1] = 0.75
    upd = lc & ~fixed
    kw = dict(GNC) if cost == "GNC_TLS" else dict(TLSThreshold=3.0, HuberThreshold=1.0)
    params = rb.RobustCostParameters(cost, **kw)
    s = da.RbcdSession(ds, num_robots=R, r=r, robust=params, fixed_weight=fixed)
    T = da.chordal_initialization(common.product_dataset("smallGrid3D"))
    X0 = np.zeros((r, 4 * ds.n))
    X0[:3] = T
    s.set_X(X0)
    checked = {0, 3, 8} if cost == "GNC_TLS" else {0}
    for u in range(max(checked) + 1):
        s.run(max_iters=5, rgrad_tol=0.0)
        X, before = s.get_X(), s.get_weights()
        counts = s.update_weights()
        w = s.get_weights()
        if u in checked:
            _check_weights(da, ds, X, upd, before, w, counts, params, u)
        assert s.robust_info()["updates"] == u + 1
        assert np.array_equal(s.get_X(), X)  # the iterate lives on (no reset asked for)
    if cost == "GNC_TLS":
        assert s.robust_info()["mu"] == pytest.approx(1e-4 * 2.0 ** (max(checked) + 1), rel=1e-12)
    s.close()


def _tcg_runs(s):
    return s.profile_tcg_read()["launches"]


@pytest.mark.parametrize("name,R,zeros", [("smallGrid3D", 5, False), ("sphere2500", 5, False), ("torus3D", 8, False),
                                          ("smallGrid3D", 5, True), ("sphere2500", 5, True), ("torus3D", 8, True)])
def test_in_place_equals_a_fresh_session(da, name, R, zeros):
    from dcora_amd import robust as rb
    ds = common.product_dataset(name)
    rng = np.random.default_rng(7)
    w = rng.uniform(0.05, 1.0, ds.m)
    if zeros:
        w[rng.choice(ds.m, ds.m // 10, replace=False)] = 0.0
    A = da.RbcdSession(ds, num_robots=R, r=5, robust=rb.RobustCostParameters("GNC_TLS"))
    A.set_X(_start(da, ds, 5))
    A.run(max_iters=10, rgrad_tol=0.0)
    A.set_weights(w)
    assert np.array_equal(A.get_weights(), w)
    A.set_acceleration(False)
    X = A.get_X()
    B = da.RbcdSession(_copy(da, ds, w), num_robots=R, r=5, acceleration=False)
    B.set_X(X)
    outs, Xs, runs = [], [], []
    for s in (A, B):
        s.profile_tcg_runs(True)
        s.profile_tcg_read()
        outs.append(s.run(max_iters=40, rgrad_tol=0.0))
        runs.append(_tcg_runs(s))
        s.profile_tcg_runs(False)
        Xs.append(s.get_X())
    assert runs[0] == runs[1]
    if zeros and name == "torus3D":  # the sparse preconditioner: the Q-apply's pattern keeps explicit zeros
        assert np.array_equal(outs[0]["selected"], outs[1]["selected"])
        assert np.allclose(outs[0]["cost"], outs[1]["cost"], rtol=1e-9, atol=0)
        assert common.rel(Xs[0], Xs[1]) < 1e-7
    else:
        _same_run(*outs)
        assert np.array_equal(Xs[0], Xs[1])
    A.close()
    B.close()


def test_cached_images_stay_intact(da):
    """a robust session that attached a plain session's cached inverses replaces them on a weight update, it never
    writes them: the plain session's next iterations are those it ran before, and those of a fresh twin"""
    from dcora_amd import driver
    from dcora_amd import robust as rb
    R, r = 5, 5
    ds = _with_outliers(da.Dataset, common.product_dataset("sphere2500"), 30, seed=4)
    ds.vals[driver.loop_closure_mask(ds, R), -1] = 1.0
    X0 = _start(da, ds, r)
    P = da.RbcdSession(ds, num_robots=R, r=r)
    P.set_X(X0)
    before = P.run(max_iters=20, rgrad_tol=0.0)
    hits = da.precond_cache_info()["hits"]
    A = da.RbcdSession(ds, num_robots=R, r=r, robust=rb.RobustCostParameters("GNC_TLS", **GNC))
    assert da.precond_cache_info()["hits"] >= hits + R  # every agent of A attached P's images
    A.set_X(X0)
    A.run(max_iters=10, rgrad_tol=0.0)
    c = A.update_weights()
    assert c["accepted"] + c["undecided"] + c["rejected"] > 0 and not np.all(A.get_weights() == 1.0)
    A.run(max_iters=3, rgrad_tol=0.0)
    P.set_X(X0)
    after = P.run(max_iters=20, rgrad_tol=0.0)
    T = da.RbcdSession(_copy(da, ds), num_robots=R, r=r)
    T.set_X(X0)
    twin = T.run(max_iters=20, rgrad_tol=0.0)
    _same_run(before, after)
    _same_run(after, twin)
    for s in (A, P, T):
        s.close()


@pytest.mark.parametrize("name,n_out,seed,optimum", [("smallGrid3D", 12, 2, 1025.398), ("sphere2500", 30, 4, 1687.02)])
def test_gnc_in_one_session_rejects_the_injected_outliers(da, name, n_out, seed, optimum):
    from dcora_amd import driver
    from dcora_amd import robust as rb
    R, r = 5, 5
    clean = common.product_dataset(name)
    T = da.chordal_initialization(clean)
    X0 = np.zeros((r, (clean.d + 1) * clean.n))
    X0[:clean.d] = T
    outs = {}
    for tag, flow in (("session", driver.multi_robot_gnc_session), ("example", driver.multi_robot_gnc_example)):
        ds = _with_outliers(da.Dataset, clean, n_out, seed=seed)
        outs[tag] = flow(ds, X0, num_robots=R, r=r, robust=rb.RobustCostParameters("GNC_TLS", **GNC),
                         num_weight_updates=20, inner_iters=30, rgrad_tol=0.1)
        assert np.array_equal(ds.vals[:, -1], outs[tag]["weights"])
    out = outs["session"]
    lc, w = out["loop_closures"], out["weights"]
    m0 = clean.m
    assert np.all(w[m0:] < 1e-8), "every injected closure is rejected"
    assert np.all(w[:m0][lc[:m0]] > 1 - 1e-8), "every original closure is kept"
    assert np.all(w[~lc] == 1.0)
    assert out["rounds"][-1]["rejected"] == n_out
    assert abs(out["final"]["cost_2f"] - optimum) < 0.05
    cls = lambda v: np.where(v < 1e-8, 0, np.where(v > 1 - 1e-8, 2, 1))
    assert np.array_equal(cls(w), cls(outs["example"]["weights"]))


def test_refusals_leave_the_session_untouched_and_reset_restores_the_start(da):
    from dcora_amd import capi, driver
    from dcora_amd import robust as rb
    R, r = 5, 5
    ds = common.product_dataset("smallGrid3D")
    lc = driver.loop_closure_mask(ds, R)
    fixed = np.zeros(ds.m, bool)
    zero_edge = int(np.nonzero(lc)[0][0])
    fixed[zero_edge] = True
    ds.vals[zero_edge, -1] = 0.0  # a fixed weight 0: not in the session's pattern
    params = rb.RobustCostParameters("GNC_TLS", **GNC)
    X0, X1 = _start(da, ds, r, 3), _start(da, ds, r, 4)
    A = da.RbcdSession(ds, num_robots=R, r=r, robust=params, fixed_weight=fixed)
    B = da.RbcdSession(ds, num_robots=R, r=r, robust=params, fixed_weight=fixed)
    for s in (A, B):
        s.set_X(X0)
        s.run(max_iters=7, rgrad_tol=0.0)
    w0 = A.get_weights()
    Xa = A.get_X()
    bad = []
    for v in (np.nan, -0.5, np.inf):
        w = w0.copy()
        w[3] = v
        bad.append(w)
    w = w0.copy()
    w[zero_edge] = 0.5
    bad.append(w)
    for w in bad:
        with pytest.raises(capi.DcoraError) as e:
            A.set_weights(w)
        assert e.value.status == 1  # DCORA_ERR_BAD_ARG
    assert np.array_equal(A.get_weights(), w0) and np.array_equal(A.get_X(), Xa)
    assert A.robust_info() == B.robust_info()
    _same_run(A.run(max_iters=12, rgrad_tol=0.0), B.run(max_iters=12, rgrad_tol=0.0))
    assert np.array_equal(A.get_X(), B.get_X())
    # the wrong kind of session
    P = da.RbcdSession(ds, num_robots=R, r=r)
    for call in (lambda: P.update_weights(), lambda: P.set_weights(w0), lambda: P.get_weights(),
                 lambda: P.robust_info()):
        with pytest.raises(capi.DcoraError) as e:
            call()
        assert e.value.status == 1
    P.close()
    with pytest.raises(capi.DcoraError) as e:
        da.RbcdSession(ds, num_robots=R, r=r, robust=params, world_size=2)
    assert e.value.status == 8  # DCORA_ERR_UNSUPPORTED
    # robustOptNumResets: X back to the last set_X
    A.set_X(X1)
    A.run(max_iters=6, rgrad_tol=0.0)
    A.update_weights(reset_to_initial=True)
    assert np.array_equal(A.get_X(), X1)
    assert A.robust_info()["updates"] == 1
    A.close()
    B.close()
