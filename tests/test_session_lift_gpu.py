"""The Riemannian staircase's step inside a live session (dcora_rbcd_lift / dcora_ra_rbcd_lift, ref
examples/MultiRobotExample.cpp:352-366, src/QuadraticProblem.cpp:138-234): the session goes from rank r to r + 1 in
place and keeps what does not depend on r.

(theta, v) always comes from the host path (da.dual_certificate + da.fast_verification), so both sides of a comparison
get the same eigenvector.  Tolerances: the lift against the whole-graph problem's escapeSaddle 1e-12 max|X| (the same
kernels on the same inputs), against the oracle's escape_saddle common.rel < 1e-9 (tests/test_gpu_parity.py); a lifted
session against a fresh one bitwise; the certificate after a lift tests/test_session_certify_gpu.py's."""
import numpy as np
import pytest

import common
import ra_loops
from test_raslam import ra_path

pytestmark = pytest.mark.gpu

ETA = 1e-3
GNC = dict(GNCBarc=10.0, GNCMuStep=2.0)  # as tests/test_gnc_session_gpu.py
UNSUPPORTED, BAD_ARG = 8, 1


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


class Pgo:
    """a pose-graph fixture with its host matrices, shared and left unchanged"""

    def __init__(self, da, orc, name, R):
        self.name, self.R = name, R
        self.ds, self.dso = common.product_dataset(name), common.oracle_dataset(name)
        self.d, self.n, self.k = self.ds.d, self.ds.n, (self.ds.d + 1) * self.ds.n
        self.Q, self.Qo = da.build_Q_pgo(self.ds), orc.build_Q_pgo(self.dso)
        self.block, self.kw, self.reg = self.d + 1, {}, 0.1
        self.tol = dict(gradient_tolerance=1e-6, preconditioned_gradient_tolerance=1e-6)

    def session(self, da, r, **kw):
        return da.RbcdSession(self.ds, num_robots=self.R, r=r, **kw)

    def point(self, orc, r, seed):
        return common.random_point(r, self.d, self.n, seed, orc.project_to_manifold)


class Ra:
    """a range-aided fixture; reg: what driver.multi_robot_raslam_example passes to its whole-graph problem"""

    def __init__(self, da, orc, name):
        self.name = name
        self.ra = da.RADataset(ra_path(name))
        ra = self.ra
        self.d, self.n, self.k = ra.d, ra.n, ra.k
        self.Q, self.Qo = ra.Q, orc.CSR.from_scipy(ra.Q.to_scipy())
        self.block, self.kw = 1, dict(l=ra.l, b=ra.b)
        self.reg = da.precond_regularization(ra.Q)
        self.tol = dict(gradient_tolerance=1e-4, preconditioned_gradient_tolerance=1e-4)

    def session(self, da, r, **kw):
        return da.RaRbcdSession(self.ra, r, **kw)

    def point(self, orc, r, seed):
        rng = np.random.default_rng(seed)
        return orc.project_to_manifold(r, self.d, self.n, rng.uniform(-1, 1, (r, self.k)), **self.kw)


@pytest.fixture(scope="module")
def fixtures(env):
    da, orc = env
    made = {}

    def get(name):
        if name not in made:
            made[name] = (Ra(da, orc, name) if name.startswith("range_aided") else
                          Pgo(da, orc, name, 3 if name == "tinyGrid3D" else 5))
        return made[name]
    return get


def _direction(da, fx, r, X):
    """(theta, v) of the refused host certificate at X"""
    S = da.dual_certificate(r, fx.d, fx.n, X, fx.Q, **fx.kw)
    psd, theta, v, lmin = da.fast_verification(S, ETA, block=fx.block)
    assert not psd, "the case needs a refused certificate"
    return theta, v


def _whole_graph(da, fx, r):
    return da.QuadraticProblem(r, fx.d, fx.n, fx.Q, reg=fx.reg, **fx.kw)


def _host_rule(P, X, v, gtol, pgtol):
    """src/QuadraticProblem.cpp:161-233 with the whole-graph problem's own operations -> (escaped, trials)"""
    k = X.shape[1]
    Xp = np.vstack([X, np.zeros((1, k))])
    D = np.zeros_like(Xp)
    D[-1] = v
    FX, alpha, fv = P.f(Xp), 1.0, []
    while alpha >= 1e-6:
        Xt = P.Retract(Xp, alpha * D)
        g = P.RieGrad(Xt)
        fv.append(P.f(Xt))
        if fv[-1] < FX and np.linalg.norm(g) > gtol and np.linalg.norm(P.PreCondition(Xt, g)) > pgtol:
            return True, len(fv)
        alpha /= 2
    return min(fv) < FX, len(fv)


# ---- 1. the lift is the parent's path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r", [("smallGrid3D", 3), ("smallGrid3D", 5), ("smallGrid3D", 7), ("smallGrid3D", 8),
                                    ("range_aided_slam_test_2d", 2), ("range_aided_slam_test_2d", 3),
                                    ("range_aided_slam_test_3d", 3)])
def test_lift_is_escape_saddle_of_the_whole_graph_problem(env, fixtures, name, r):
    """5 -> 6 crosses into k_tcg_run<3, 6, 4>'s last rank, 7 -> 8 stays fused, 8 -> 9 is where `fused` ends"""
    da, orc = env
    fx = fixtures(name)
    X = fx.point(orc, r, 4)
    theta, v = _direction(da, fx, r, X)
    s = fx.session(da, r)
    s.set_X(X)
    assert np.array_equal(s.get_X(), X)
    escaped, info = s.lift(theta, v, **fx.tol)
    Xl = s.get_X()
    P = _whole_graph(da, fx, r + 1)
    Xn = P.escapeSaddle(X, theta, v, fx.tol["gradient_tolerance"], fx.tol["preconditioned_gradient_tolerance"])
    h_escaped, h_trials = _host_rule(P, X, v, fx.tol["gradient_tolerance"], fx.tol["preconditioned_gradient_tolerance"])
    P.close()
    Po = orc.Problem(r + 1, fx.d, fx.n, fx.Qo, reg=fx.reg, **fx.kw)
    Xo = Po.escape_saddle(X, theta, v, gtol=fx.tol["gradient_tolerance"],
                          pgtol=fx.tol["preconditioned_gradient_tolerance"])
    assert escaped == (Xn is not None) == h_escaped == (Xo is not None)
    assert escaped, "a random point is no minimum: the case needs an escape"
    assert info["trials"] == h_trials, (info, h_trials)
    assert s.r == r + 1 and Xl.shape == (r + 1, fx.k)
    diff = np.abs(Xl - Xn).max()
    print("%s r %d -> %d: trials %d, alpha %.6g, f %.9g -> %.9g, max |X_lift - X_escapeSaddle| %.3g, rel to oracle "
          "%.3g" % (name, r, r + 1, info["trials"], info["alpha"], info["f_before"], info["f_after"], diff,
                    common.rel(Xl, Xo)))
    assert diff <= 1e-12 * np.abs(Xn).max()
    assert common.rel(Xl, Xo) < 1e-9
    assert info["f_after"] < info["f_before"]
    s.close()


# ---- 2. the lifted session is a fresh session ---------------------------------------------------------------------------
def _solve_facts(s):
    res = s.last_result()
    res.pop("elapsedMs")
    return res


@pytest.mark.parametrize("name,r,iters", [("smallGrid3D", 5, 12), ("tinyGrid3D", 3, 35)])
def test_lifted_pose_graph_session_runs_as_a_fresh_one(env, fixtures, name, r, iters):
    """35 iterations on tinyGrid3D cross the restart at 30"""
    da, orc = env
    fx = fixtures(name)
    X = fx.point(orc, r, 4)
    theta, v = _direction(da, fx, r, X)
    A = fx.session(da, r)
    A.set_X(X)
    A.run(max_iters=7, rgrad_tol=0.0)  # (a session in mid-flight: sequences, counters and a last solve to forget)
    A.set_X(X)
    escaped, _ = A.lift(theta, v)
    assert escaped and A.r == r + 1
    Xl = A.get_X()
    B = fx.session(da, r + 1)
    B.set_X(Xl)
    outs, Xs, facts, runs = [], [], [], []
    for s in (A, B):
        s.profile_tcg_runs(True)
        s.profile_tcg_read()
        outs.append(s.run(max_iters=iters, rgrad_tol=0.0))
        runs.append(s.profile_tcg_read()["launches"])
        s.profile_tcg_runs(False)
        Xs.append(s.get_X())
        facts.append(_solve_facts(s))
    for key in ("selected", "cost", "gradnorm"):
        assert outs[0][key].size == iters and np.array_equal(outs[0][key], outs[1][key]), key
    assert np.array_equal(Xs[0], Xs[1])
    assert facts[0] == facts[1] and runs[0] == runs[1], (facts, runs)  # the same solver form was picked
    A.close()
    B.close()


@pytest.mark.parametrize("name,r", [("range_aided_slam_test_2d", 2), ("range_aided_slam_test_3d", 3)])
def test_lifted_range_aided_session_runs_as_a_fresh_one(env, fixtures, name, r):
    """12 greedy iterations, then 3 coloured sweeps with acceleration off"""
    da, orc = env
    fx = fixtures(name)
    X = fx.point(orc, r, 4)
    theta, v = _direction(da, fx, r, X)
    A = fx.session(da, r, restart_interval=5)
    A.set_X(X)
    A.run(max_iters=4, rgrad_tol=0.0)
    A.set_X(X)
    escaped, _ = A.lift(theta, v, **fx.tol)
    assert escaped and A.r == r + 1
    Xl = A.get_X()
    B = fx.session(da, r + 1, restart_interval=5)
    B.set_X(Xl)
    got = []
    for s in (A, B):
        greedy = s.run(max_iters=12, rgrad_tol=0.0)
        Xg = s.get_X()
        facts = _solve_facts(s)
        s.set_acceleration(False)
        sweeps = s.run_coloured(max_sweeps=3, rgrad_tol=0.0)
        got.append((greedy, Xg, facts, sweeps, s.get_X()))
    a, b = got
    for key in ("selected", "cost", "gradnorm"):
        assert a[0][key].size == 12 and np.array_equal(a[0][key], b[0][key]), key
    assert np.array_equal(a[1], b[1]) and a[2] == b[2]
    for key in ("cost", "gradnorm"):
        assert a[3][key].size == 3 and np.array_equal(a[3][key], b[3][key]), key
    assert np.array_equal(a[4], b[4])
    A.close()
    B.close()


# ---- 3. a real staircase in one session -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,R,r_min,seed", [("tinyGrid3D", 3, 3, 21), ("smallGrid3D", 5, 3, 4)])
def test_pose_graph_staircase_in_one_session(env, name, R, r_min, seed):
    """tests/test_param_space.py::test_riemannian_staircase_of_the_multi_robot_driver's cases through
    driver.multi_robot_staircase_session, against the driver that re-creates its sessions"""
    da, orc = env
    from dcora_amd import driver
    ds, dso = common.product_dataset(name), common.oracle_dataset(name)
    X0 = common.random_point(r_min, ds.d, ds.n, seed, orc.project_to_manifold)
    kw = dict(num_robots=R, r_min=r_min, r_max=r_min + 6, max_iters=400, rgrad_tol=0.05)
    out = driver.multi_robot_staircase_session(ds, X0, **kw)
    ref = driver.multi_robot_example(ds, X0, **kw)
    print("%s: ranks %s, iterations %s, final 2f %.9g (re-created sessions: ranks %s, 2f %.9g)" %
          (name, [lv["rank"] for lv in out["levels"]], [lv["iterations"] for lv in out["levels"]],
           out["levels"][-1]["cost_2f"], [lv["rank"] for lv in ref["levels"]], ref["levels"][-1]["cost_2f"]))
    assert out["certified"] and ref["certified"]
    assert out["rank"] > r_min and out["X"].shape == (out["rank"], (ds.d + 1) * ds.n)
    assert [lv["escaped"] for lv in out["levels"][:-1]] == [True] * (len(out["levels"]) - 1)
    assert [lv["rank"] for lv in out["levels"]] == list(range(r_min, out["rank"] + 1))
    n0 = out["levels"][0]["iterations"]  # the first level has no eigenvector in it: the same trace
    assert np.array_equal(out["selected"][:n0], ref["selected"][:n0])
    assert np.array_equal(out["cost"][:n0], ref["cost"][:n0])
    f, f_ref = out["levels"][-1]["cost_2f"], ref["levels"][-1]["cost_2f"]
    assert abs(f - f_ref) < 1e-3 * abs(f_ref)
    assert out["suboptimality_gap_f"] is not None and out["suboptimality_gap_f"] >= 0
    So = orc.dual_certificate(out["rank"], ds.d, ds.n, out["X"], orc.build_Q_pgo(dso))
    assert orc.fast_verification(So, 1e-3, block=ds.d + 1)[0]


@pytest.mark.parametrize("name", ["range_aided_slam_test_2d", "range_aided_slam_test_3d"])
def test_range_aided_staircase_in_one_session(env, name):
    """tests/test_ra_session.py::test_multi_robot_raslam_driver_reaches_the_certified_optimum's cases through
    driver.raslam_staircase_session"""
    da, orc = env
    from dcora_amd import driver
    ra = da.RADataset(ra_path(name))
    d = ra.d
    rng = np.random.default_rng(12)
    X0 = orc.project_to_manifold(d, d, ra.n, rng.standard_normal((d, ra.k)), l=ra.l, b=ra.b)
    out = driver.raslam_staircase_session(ra, X0, max_iters=300, rgrad_tol=1e-3, r_max=d + 5)
    print("%s: ranks %s, iterations %s, final 2f %.3g" % (name, [lv["rank"] for lv in out["levels"]],
                                                         [lv["iterations"] for lv in out["levels"]],
                                                         out["levels"][-1]["cost_2f"]))
    assert out["certified"], out["levels"]
    assert out["rank"] > d
    assert [lv["escaped"] for lv in out["levels"][:-1]] == [True] * (len(out["levels"]) - 1)
    assert out["levels"][-1]["cost_2f"] < 1e-3
    So = orc.dual_certificate(out["rank"], d, ra.n, out["X"], orc.CSR.from_scipy(ra.Q.to_scipy()), l=ra.l, b=ra.b)
    assert orc.fast_verification(So, 1e-3, block=1)[0]


# ---- 4. state survives --------------------------------------------------------------------------------------------------
def _with_outliers(ds_cls, base, n_out, seed):
    # (copied from tests/test_gnc_session_gpu.py)
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


def _robust_state_survives(da, A, fresh, direction, r, mu_step, tol):
    """A: a robust session at rank r with its team enabled, after two weight updates; fresh(w) -> a robust session at
    r + 1 with the weights w; direction(X, w) -> (theta, v) of the host certificate with those weights"""
    w, rinfo, tinfo = A.get_weights(), A.robust_info(), A.team_info()
    assert rinfo["updates"] == 2
    X = A.get_X()
    theta, v = direction(X, w)
    escaped, info = A.lift(theta, v, **tol)
    assert escaped and A.r == r + 1 and info["precond_built"]
    assert np.array_equal(A.get_weights(), w)
    assert A.robust_info() == rinfo
    after = A.team_info()
    assert after["weight_updates"] == tinfo["weight_updates"] and after["resets"] == tinfo["resets"]
    assert after["inner_iter"] == 0  # (the round counters are set_X's)
    assert all(A.agent_status(q) is None for q in range(A.R))  # statuses unknown after the lift
    Xl = A.get_X()
    B = fresh(w)
    B.set_X(Xl)
    outs, Xs = [], []
    for s in (A, B):
        outs.append(s.run(max_iters=12, rgrad_tol=0.0))
        Xs.append(s.get_X())
    assert np.array_equal(outs[0]["selected"], outs[1]["selected"])
    if np.any(w == 0.0):  # explicit zeros on the live session's patterns: tests/test_gnc_session_gpu.py:167-169's bounds
        assert np.allclose(outs[0]["cost"], outs[1]["cost"], rtol=1e-9, atol=0)
        assert common.rel(Xs[0], Xs[1]) < 1e-7
    else:
        assert np.array_equal(outs[0]["cost"], outs[1]["cost"]) and np.array_equal(Xs[0], Xs[1])
    B.close()
    assert any(A.agent_status(q) is not None for q in range(A.R))
    A.update_weights()
    now = A.robust_info()
    assert now["updates"] == 3 and now["mu"] == pytest.approx(rinfo["mu"] * mu_step, rel=1e-12)
    # a second lift finds the central preconditioner stale: the weights have changed
    X2 = A.get_X()
    theta2, v2 = direction(X2, A.get_weights())
    escaped2, info2 = A.lift(theta2, v2, **tol)
    assert info2["precond_built"]
    assert A.r == r + 1 + int(escaped2)
    out = A.run_team()
    assert out["iters"] > 0
    A.close()


def test_robust_pose_graph_session_keeps_its_state(env):
    da, orc = env
    from dcora_amd import robust as rb
    R, r = 5, 5
    ds = _with_outliers(da.Dataset, common.product_dataset("smallGrid3D"), 12, seed=2)
    params = rb.RobustCostParameters("GNC_TLS", **GNC)
    A = da.RbcdSession(ds, num_robots=R, r=r, robust=params)
    A.enable_team(max_num_iters=20)
    X0 = np.zeros((r, 4 * ds.n))
    X0[:3] = da.chordal_initialization(common.product_dataset("smallGrid3D"))
    A.set_X(X0)
    for _ in range(2):
        A.run(max_iters=5, rgrad_tol=0.0)
        A.update_weights()

    def with_weights(w):
        c = da.Dataset(ds.d, ds.n, ds.ids.copy(), ds.vals.copy())
        c.vals[:, -1] = w
        return c

    def direction(X, w):
        S = da.dual_certificate(X.shape[0], ds.d, ds.n, X, da.build_Q_pgo(with_weights(w)))
        psd, theta, v, lmin = da.fast_verification(S, ETA, block=ds.d + 1)
        assert not psd
        return theta, v

    def fresh(w):
        B = da.RbcdSession(ds, num_robots=R, r=r + 1, robust=params)
        B.set_weights(w)
        return B

    _robust_state_survives(da, A, fresh, direction, r, GNC["GNCMuStep"],
                           dict(gradient_tolerance=1e-6, preconditioned_gradient_tolerance=1e-6))


def test_robust_range_aided_session_keeps_its_state(env, tmp_path):
    """the loop-closure variant of tiers the range-aided GNC tests use (ra_loops.GNC_FIXTURE), rank 3 -> 4"""
    da, orc = env
    from dcora_amd import robust as rb
    path = ra_loops.write_loops_variant(tmp_path, **ra_loops.GNC_FIXTURE)[0]
    ra = da.RADataset(path)
    r = 3
    params = rb.RobustCostParameters("GNC_TLS", **ra_loops.GNC_PARAMS)
    A = da.RaRbcdSession(ra, r, restart_interval=5, robust=params)
    A.enable_team(max_num_iters=12)
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    A.set_X(X0)
    for _ in range(2):
        A.run(max_iters=5, rgrad_tol=0.0)
        A.update_weights()

    def direction(X, w):
        f = da.RADataset(path)
        f.set_pose_pose_weights(w)
        S = da.dual_certificate(X.shape[0], ra.d, ra.n, X, f.Q, l=ra.l, b=ra.b)
        psd, theta, v, lmin = da.fast_verification(S, ETA, block=1)
        assert not psd
        return theta, v

    def fresh(w):
        B = da.RaRbcdSession(da.RADataset(path), r + 1, restart_interval=5, robust=params)
        B.set_weights(w)
        return B

    _robust_state_survives(da, A, fresh, direction, r, ra_loops.GNC_PARAMS["GNCMuStep"],
                           dict(gradient_tolerance=1e-4, preconditioned_gradient_tolerance=1e-4))


# ---- 5. the certificate after a lift ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r", [("smallGrid3D", 5), ("range_aided_slam_test_3d", 3)])
def test_certificate_after_a_lift(env, fixtures, name, r):
    """the session has certified before the lift, so the certificate's r-sized buffer is re-sized, not built anew"""
    da, orc = env
    fx = fixtures(name)
    X = fx.point(orc, r, 4)
    s = fx.session(da, r)
    s.set_X(X)
    psd, theta, v, lmin, info = s.certify(ETA)
    assert not psd
    escaped, _ = s.lift(theta, v, **fx.tol)
    assert escaped
    Xl = s.get_X()
    psd, theta, v, lmin, info = s.certify(ETA)
    S = da.dual_certificate(r + 1, fx.d, fx.n, Xl, fx.Q, **fx.kw)
    hpsd, htheta, hv, hlmin = da.fast_verification(S, ETA, block=fx.block)
    A = S.to_scipy()
    print("%s after the lift: psd %s / host %s, theta %.12g / host %.12g, lambda_min %.12g / host %.12g" %
          (name, psd, hpsd, theta, htheta, lmin, hlmin))
    assert not hpsd and not psd
    assert abs(theta - htheta) <= 2e-3 * abs(htheta)
    assert abs(np.linalg.norm(v) - 1) <= 1e-12
    assert abs(theta - v @ (A @ v)) <= fx.d * 1e-9
    w0 = np.linalg.eigvalsh(A.toarray() + ETA * np.eye(A.shape[0]))[0]
    assert abs(lmin - w0) <= 2e-3 * max(1.0, abs(w0))
    s.close()


# ---- 6. nothing happens when nothing should -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,r", [("smallGrid3D", 5), ("range_aided_slam_test_2d", 3)])
def test_no_escape_leaves_the_session_untouched(env, fixtures, name, r):
    da, orc = env
    fx = fixtures(name)
    X = fx.point(orc, r, 4)
    got = []
    for calls in (True, False):
        s = fx.session(da, r)
        s.set_X(X)
        s.run(max_iters=3, rgrad_tol=0.0)
        if calls:
            escaped, info = s.lift(-1.0, np.zeros(fx.k), **fx.tol)
            assert not escaped and info["alpha"] == 0 and info["trials"] > 0
            assert s.r == r
        Xs = s.get_X()
        out = s.run(max_iters=10, rgrad_tol=0.0)
        got.append((Xs, out, s.get_X()))
        s.close()
    a, b = got
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    for key in ("selected", "cost", "gradnorm"):
        assert a[1][key].size == 10 and np.array_equal(a[1][key], b[1][key]), key


def test_refusals(env, fixtures):
    da, orc = env
    fx = fixtures("smallGrid3D")
    v = np.ones(fx.k) / np.sqrt(fx.k)
    ranked = da.RbcdSession(fx.ds, num_robots=4, r=5, rank=0, world_size=2)
    with pytest.raises(da.DcoraError) as e:
        ranked.lift(-1.0, v)
    assert e.value.status == UNSUPPORTED and ranked.r == 5
    ranked.close()
    top = da.RbcdSession(fx.ds, num_robots=5, r=16)
    with pytest.raises(da.DcoraError) as e:
        top.lift(-1.0, v)
    assert e.value.status == BAD_ARG and top.r == 16
    top.close()
    s = da.RbcdSession(fx.ds, num_robots=5, r=5)
    X = fx.point(orc, 5, 4)
    s.set_X(X)
    bad = v.copy()
    bad[7] = np.nan
    for args, kw in (((-1.0, bad), {}), ((np.nan, v), {}), ((-1.0, v), dict(gradient_tolerance=np.inf))):
        with pytest.raises(da.DcoraError) as e:
            s.lift(*args, **kw)
        assert e.value.status == BAD_ARG
    assert s.r == 5 and np.array_equal(s.get_X(), X)
    s.close()
    fr = fixtures("range_aided_slam_test_2d")
    t = da.RaRbcdSession(fr.ra, 2, rank=0, world_size=2)
    with pytest.raises(da.DcoraError) as e:
        t.lift(-1.0, np.ones(fr.k))
    assert e.value.status == UNSUPPORTED
    t.close()


def test_lifts_build_one_preconditioner(env, fixtures):
    """the first lift pays the central preconditioner, the agents' images are kept: at most one cache miss; the second
    lift none"""
    da, orc = env
    fx = fixtures("smallGrid3D")
    r = 4
    X = fx.point(orc, r, 4)
    s = fx.session(da, r)
    s.set_X(X)
    m0 = da.precond_cache_info()["misses"]
    escaped, info = s.lift(*_direction(da, fx, r, X))
    m1 = da.precond_cache_info()["misses"]
    assert escaped and info["precond_built"] and m1 - m0 <= 1
    X1 = s.get_X()
    escaped, info = s.lift(*_direction(da, fx, r + 1, X1))
    m2 = da.precond_cache_info()["misses"]
    assert escaped and not info["precond_built"] and info["precond_ms"] == 0 and m2 == m1
    assert s.r == r + 2
    s.close()
