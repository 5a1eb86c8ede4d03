"""The Riemannian staircase's step across the ranks of a job (dcora_rbcd_reserve_rank / dcora_ra_rbcd_reserve_rank,
dcora_exchange_lift; ref examples/MultiRobotExample.cpp:352-366, src/QuadraticProblem.cpp:138-234).

(theta, v) always comes from the host path (da.dual_certificate + da.fast_verification) and goes to every rank as a file,
so every side of a comparison gets the same eigenvector.  One process per rank, all on device 0, at most 4 ranks.

The collective lift takes the third test of the search with the agents' own preconditioners,
|P grad|^2 = sum_a |Proj(rgrad_a M_a^-1)|^2, the single-process lift with the whole graph's.  The cases that compare
the two are therefore cases where the two norms cannot decide differently, and the tests assert that on the
single-process side: every deciding comparison clears its threshold by a factor 10, every deciding f difference
exceeds 1e-9 |f|.  Tolerances: the accepted point is one retraction of the same images by the same kernel, so it is
held to the 1e-12 max|X| that tests/test_session_lift_gpu.py holds between the session and the host problem, and to
common.rel < 1e-9 against the oracle's escape_saddle; between rank counts and transports it is the same retraction
of the same bits pose by pose: bit-equal.  A lifted job against a fresh one at r + 1: bit-equal X and selected, costs
as the rank tests compare them (tests/test_gnc_ranks_gpu.py: rtol 1e-11 / 1e-9; bit-equal here, where both sides have
the same ranks and agents)."""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import common
from test_raslam import ra_path
from test_session_lift_gpu import ETA, Pgo, Ra, _direction, _whole_graph

pytestmark = pytest.mark.gpu

WORKER = os.path.join(common.HERE, "lift_ranks_worker.py")
UNSUPPORTED, BAD_ARG = 8, 1
PGO_TOL = dict(gradient_tolerance=1e-6, preconditioned_gradient_tolerance=1e-6)
RA_TOL = dict(gradient_tolerance=1e-4, preconditioned_gradient_tolerance=1e-4)
# dcora_debug_launch_count of ranks 0 and 1 of the unreserved twin job of test_no_escape_leaves_the_job_untouched --
# creation, set_X, 3 and then 10 greedy iterations from the seed-4 point, 2 ranks -- taken with a build of the commit
# before dcora_exchange_lift existed (the RA job's second rank hosts one small agent)
PARENT_LAUNCHES = {"smallGrid3D": (162, 150), "range_aided_slam_test_2d": (134, 53)}


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


def run_ranks(tmp_path, world, cfg, X0, v=None, transport=None):
    d = str(tmp_path)
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "X0.npy"), X0)
    if v is not None:
        np.save(os.path.join(d, "v.npy"), v)
    with open(os.path.join(d, "job.json"), "w") as f:
        json.dump(cfg, f)
    job = "l%s" % uuid.uuid4().hex[:12]
    env_ = dict(os.environ)
    env_["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env_["DCORA_EXCHANGE_TIMEOUT_S"] = "60"
    env_.pop("DCORA_EXCHANGE_WAIT", None)
    if transport:
        env_["DCORA_EXCHANGE"] = transport
    else:
        env_.pop("DCORA_EXCHANGE", None)
    procs = [subprocess.Popen([sys.executable, WORKER, str(k), str(world), job, d], env=env_, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for k in range(world)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode(errors="replace"))
    for k, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (k, outs[k][-3000:])
    return [np.load(os.path.join(d, "rank%d.npz" % k)) for k in range(world)]


# ---- the cases, computed once and left unchanged -----------------------------------------------------------------------
class Case:
    """a fixture at rank r with a point, the refused host certificate's direction there and the single-process lift"""

    def __init__(self, da, orc, name, R, r, tol):
        self.name, self.R, self.r = name, R, r
        self.ra = name.startswith("range_aided")
        self.fx = Ra(da, orc, name) if self.ra else Pgo(da, orc, name, R)
        self.tol = dict(RA_TOL if self.ra else PGO_TOL, **tol)
        fx = self.fx
        self.X = fx.point(orc, r, 4)
        self.theta, self.v = _direction(da, fx, r, self.X)
        s = fx.session(da, r)
        s.set_X(self.X)
        self.escaped, self.info = s.lift(self.theta, self.v, **self.tol)
        self.Xs = s.get_X()
        s.close()

    def cfg(self, **kw):
        base = dict(kind="ra", path=ra_path(self.name)) if self.ra else dict(kind="pgo", name=self.name, R=self.R)
        return dict(base, r=self.r, reserve=self.r + 1, theta=self.theta, tol=self.tol, **kw)

    def agent_columns(self):
        """the global columns of every agent, in the agent's own ordering, with its (n, l, b)"""
        fx = self.fx
        if self.ra:
            return [(own, dims3) for dims3, own in (fx.ra.agent_columns[rb] for rb in sorted(fx.ra.agent_columns))]
        per, dh = fx.n // self.R, fx.d + 1
        ends = [(b + 1) * per if b < self.R - 1 else fx.n for b in range(self.R)]
        return [(np.arange(b * per * dh, ends[b] * dh), (ends[b] - b * per, 0, 0)) for b in range(self.R)]


@pytest.fixture(scope="module")
def cases(env):
    da, orc = env
    made = {}

    def get(name, R, r, **tol):
        key = (name, R, r, tuple(sorted(tol.items())))
        if key not in made:
            made[key] = Case(da, orc, name, R, r, tol)
        return made[key]
    return get


class BlockNorm:
    """|P grad|^2 = sum_a |Proj(rgrad_a M_a^-1)|^2 from per-agent QuadraticProblems on Q_aa at rank r + 1, with the
    regularisation the agents' solves use (0.1 on a pose graph, the lambda_max rule of the agent's Q_aa otherwise)"""

    def __init__(self, da, case):
        A = case.fx.Q.to_scipy().tocsr()
        self.parts = []
        for own, (na, la, ba) in case.agent_columns():
            Qaa = da.Csr.from_scipy(A[own][:, own].tocsr())
            reg = da.precond_regularization(Qaa) if case.ra else 0.1
            self.parts.append((own, da.QuadraticProblem(case.r + 1, case.fx.d, na, Qaa, reg=reg, l=la, b=ba)))

    def __call__(self, Xt, g):
        return np.sqrt(sum(np.linalg.norm(P.PreCondition(Xt[:, own], g[:, own])) ** 2 for own, P in self.parts))

    def close(self):
        for _, P in self.parts:
            P.close()


def block_rule(da, case):
    """_block_rule, computed once per case"""
    if not hasattr(case, "_rule"):
        case._rule = _block_rule(da, case)
    return case._rule


def _block_rule(da, case):
    """src/QuadraticProblem.cpp:161-233 restated in numpy over the whole-graph problem's f, Retract and RieGrad and the
    block-preconditioned norm -> (escaped, trials, alpha, X, margins of the deciding comparisons)"""
    fx, r = case.fx, case.r
    gtol, pgtol = case.tol["gradient_tolerance"], case.tol["preconditioned_gradient_tolerance"]
    P, pn = _whole_graph(da, fx, r + 1), BlockNorm(da, case)
    Xp = np.vstack([case.X, np.zeros((1, fx.k))])
    D = np.zeros_like(Xp)
    D[-1] = case.v
    FX, alpha, alphas, fv, seen = P.f(Xp), 1.0, [], [], []
    try:
        while alpha >= 1e-6:
            Xt = P.Retract(Xp, alpha * D)
            g = P.RieGrad(Xt)
            f, gn, bn, wn = P.f(Xt), np.linalg.norm(g), pn(Xt, g), np.linalg.norm(P.PreCondition(Xt, g))
            alphas.append(alpha)
            fv.append(f)
            seen.append(dict(f=f, gn=gn, block=bn, whole=wn))
            if f < FX and gn > gtol and bn > pgtol:
                return True, len(fv), alpha, Xt, dict(FX=FX, seen=seen)
            alpha /= 2
        i = int(np.argmin(fv))
        if fv[i] < FX:
            return True, len(fv), alphas[i], P.Retract(Xp, alphas[i] * D), dict(FX=FX, seen=seen)
        return False, len(fv), 0.0, None, dict(FX=FX, seen=seen)
    finally:
        P.close()
        pn.close()


def assert_cannot_decide_differently(case, margins):
    """on the single-process side: every comparison that decided clears its threshold by a factor 10 with either
    preconditioned norm, every f difference that decided exceeds 1e-9 |f|"""
    gtol, pgtol = case.tol["gradient_tolerance"], case.tol["preconditioned_gradient_tolerance"]
    FX, seen = margins["FX"], margins["seen"]
    fallback = gtol >= 1e8
    for t in seen:
        if fallback:  # (the f differences that decide are the least f's: below)
            assert t["gn"] < gtol / 10, t
        else:
            assert abs(t["f"] - FX) > 1e-9 * abs(FX), t
            assert t["gn"] > 10 * gtol and t["block"] > 10 * pgtol and t["whole"] > 10 * pgtol, t
    if fallback:
        fs = sorted(t["f"] for t in seen)
        assert fs[1] - fs[0] > 1e-9 * abs(FX) and FX - fs[0] > 1e-9 * abs(FX)
    print("%s r %d: f %.9g -> %s; |rgrad| %.3g, |P grad| whole graph %.3g, block form %.3g" %
          (case.name, case.r, FX, ["%.9g" % t["f"] for t in seen[:3]], seen[0]["gn"], seen[0]["whole"],
           seen[0]["block"]))


# ---- (a) the rule, in one process ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,R,r,tol", [("smallGrid3D", 5, 5, {}), ("tinyGrid3D", 3, 3, {}),
                                          ("smallGrid3D", 5, 5, dict(gradient_tolerance=1e9)),
                                          ("tinyGrid3D", 3, 3, dict(gradient_tolerance=1e9)),
                                          ("range_aided_slam_test_2d", 2, 3, {})])
def test_one_rank_exchange_runs_the_rule_with_the_block_norm(env, cases, name, R, r, tol):
    """the exchange of a one-rank job takes the collective path; gradient_tolerance = 1e9 fails every trial's gradient
    test: 20 trials, then the trial of least f"""
    da, orc = env
    case = cases(name, R, r, **tol)
    fx = case.fx
    s = fx.session(da, r)
    s.reserve_rank(r + 1)
    ex = da.Exchange(s, "a%s" % uuid.uuid4().hex[:12])
    ex.set_X(case.X)
    escaped, info = ex.lift(case.theta, case.v, **case.tol)
    Xl = ex.gather_X()
    assert s.r == r + 1 and Xl.shape == (r + 1, fx.k)
    ex.close()
    s.close()
    h_escaped, h_trials, h_alpha, Xn, margins = block_rule(da, case)
    assert escaped and h_escaped
    assert (info["trials"], info["alpha"]) == (h_trials, h_alpha), (info, h_trials, h_alpha)
    if tol:
        assert info["trials"] == 20
    assert np.abs(Xl - Xn).max() <= 1e-12 * np.abs(Xn).max()
    assert info["f_after"] < info["f_before"]
    assert abs(info["f_before"] - margins["FX"]) <= 1e-11 * abs(margins["FX"])
    Po = orc.Problem(r + 1, fx.d, fx.n, fx.Qo, reg=fx.reg, **fx.kw)
    Xo = Po.escape_saddle(case.X, case.theta, case.v, gtol=case.tol["gradient_tolerance"],
                          pgtol=case.tol["preconditioned_gradient_tolerance"])
    assert Xo is not None and common.rel(Xl, Xo) < 1e-9
    # ... and the single-process lift, which tests with the whole graph's preconditioner, agrees where it must
    assert_cannot_decide_differently(case, margins)
    assert (case.info["trials"], case.info["alpha"]) == (info["trials"], info["alpha"])
    assert np.abs(Xl - case.Xs).max() <= 1e-12 * np.abs(case.Xs).max()


# ---- (b), (c) ranks against one process -----------------------------------------------------------------------------------
def _ranks_lift_as_one_process(da, case, tmp_path, world, transport):
    """one configuration of ranks and transport against the single-process lift of the case -> the gathered X"""
    assert case.escaped
    res = run_ranks(tmp_path, world, case.cfg(mode="lift"), case.X, case.v, transport=transport)
    escaped, trials, alpha, Xn, margins = block_rule(da, case)
    assert_cannot_decide_differently(case, margins)
    for k, o in enumerate(res):
        assert bool(o["escaped"]) and int(o["r"]) == case.r + 1, k
        assert (int(o["trials"]), float(o["alpha"])) == (case.info["trials"], case.info["alpha"]) == (trials, alpha)
        assert np.array_equal(o["X"], res[0]["X"]), k  # every rank gathers the same X
        assert float(o["f_before"]) == float(res[0]["f_before"]) and float(o["f_after"]) == float(res[0]["f_after"])
        assert np.abs(o["X"] - case.Xs).max() <= 1e-12 * np.abs(case.Xs).max()
        assert float(o["f_after"]) < float(o["f_before"])
    if case.tol["gradient_tolerance"] >= 1e8:
        assert int(res[0]["trials"]) == 20
    return res[0]["X"]


def test_rank_counts_and_transports_lift_to_the_same_bits(env, cases, tmp_path):
    """smallGrid3D at rank 4 on 2 ranks (R = 4) and on 4 ranks (R = 5: rank 3 hosts no agent), each over IPC peer stores
    and over the staged transport: each against the single-process lift, and the four gathered X bit-equal (the
    retraction is the same arithmetic pose by pose, whoever hosts the pose)"""
    da, orc = env
    Xs = {}
    for R, world in ((4, 2), (5, 4)):
        for transport in (None, "staged"):
            Xs[(R, world, transport)] = _ranks_lift_as_one_process(
                da, cases("smallGrid3D", R, 4), tmp_path / ("%d_%s" % (world, transport)), world, transport)
    first = Xs[(4, 2, None)]
    for key, X in Xs.items():
        assert np.array_equal(X, first), key


@pytest.mark.parametrize("name,R,r,world,tol", [
    ("range_aided_slam_test_2d", 2, 3, 2, {}),
    ("range_aided_slam_test_3d", 2, 3, 3, {}),   # two robots on three ranks
    ("smallGrid3D", 5, 5, 2, dict(gradient_tolerance=1e9)),   # (c) the fallback: 20 trials, the least f
    ("tinyGrid3D", 3, 3, 2, dict(gradient_tolerance=1e9)),
])
def test_ranks_lift_as_one_process(env, cases, tmp_path, name, R, r, world, tol):
    da, orc = env
    _ranks_lift_as_one_process(da, cases(name, R, r, **tol), tmp_path, world, None)


# ---- (d) runs as a fresh job ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,R,r,world", [("smallGrid3D", 4, 4, 2), ("range_aided_slam_test_2d", 2, 3, 2)])
def test_lifted_job_runs_as_a_fresh_one(env, cases, tmp_path, name, R, r, world):
    """35 greedy iterations (across the restart at 30), then 3 coloured sweeps with acceleration off, against a fresh
    job created at r + 1 with dcora_exchange_set_X of the gathered lifted X"""
    da, orc = env
    case = cases(name, R, r)
    after = dict(greedy=35, sweeps=3)
    A = run_ranks(tmp_path / "lifted", world, case.cfg(mode="lift", pre=7, **after), case.X, case.v)
    Xl = A[0]["X"]
    fresh = dict(case.cfg(mode="lift", lift=False, **after), r=r + 1, reserve=0)
    B = run_ranks(tmp_path / "fresh", world, fresh, Xl)
    for k in range(world):
        a, b = A[k], B[k]
        assert bool(a["escaped"]) and np.array_equal(b["X"], Xl)
        assert a["g_selected"].size == 35 and np.array_equal(a["g_selected"], b["g_selected"])
        for key in ("g_cost", "g_gradnorm", "c_cost", "c_gradnorm"):
            assert np.array_equal(a[key], b[key]), (k, key, np.max(np.abs(a[key] / b[key] - 1)))
        assert a["c_cost"].size == 3
        assert np.array_equal(a["X_greedy"], b["X_greedy"]) and np.array_equal(a["X_sweeps"], b["X_sweeps"]), k
        assert int(a["launches"]) == int(b["launches"]), k  # the same launches: the same solver forms were picked


# ---- (f) nothing happens when nothing should --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,R,r", [("smallGrid3D", 4, 4), ("range_aided_slam_test_2d", 2, 3)])
def test_no_escape_leaves_the_job_untouched(env, cases, tmp_path, name, R, r):
    """v = 0 on 2 ranks: no trial lowers f; the next 10 iterations are those of a twin job that never called lift (and
    never reserved: the reserve changes nothing of what a job computes or launches), and that twin's launch count is
    the parent commit's"""
    da, orc = env
    case = cases(name, R, r)
    v0 = np.zeros(case.fx.k)
    A = run_ranks(tmp_path / "called", 2, dict(case.cfg(mode="lift", pre=3, reset_after_pre=False, greedy=10), theta=-1.0),
                  case.X, v0)
    B = run_ranks(tmp_path / "twin", 2, dict(case.cfg(mode="lift", lift=False, pre=3, reset_after_pre=False, greedy=10),
                                             reserve=0), case.X)
    for k in range(2):
        a, b = A[k], B[k]
        assert not bool(a["escaped"]) and float(a["alpha"]) == 0 and int(a["trials"]) == 20 and int(a["r"]) == r
        assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["X_greedy"], b["X_greedy"]), k
        for key in ("g_selected", "g_cost", "g_gradnorm"):
            assert a[key].size == 10 and np.array_equal(a[key], b[key]), (k, key)
        assert int(a["launches"]) == int(b["launches"]), k  # reserved and unreserved: the same launch count
        # the unreserved job -- creation, set_X, 3 + 10 iterations -- launches what the parent commit's build launches
        assert int(b["launches_job"]) == PARENT_LAUNCHES[name][k], (k, int(b["launches_job"]))


@pytest.mark.parametrize("name,R,r,reserve,beyond", [("smallGrid3D", 4, 4, 0, UNSUPPORTED),
                                                     ("smallGrid3D", 4, 16, 0, BAD_ARG),
                                                     ("range_aided_slam_test_2d", 2, 3, 3, UNSUPPORTED)])
def test_refusals_are_the_same_on_every_rank(env, cases, tmp_path, name, R, r, reserve, beyond):
    """bad arguments, a lift beyond the reserve (none, or the job is at it; at r = 16 the rank itself is refused), a
    reserve after the exchange exists, the session's own lift: each refused alike on both ranks, and the job still runs
    as its twin that tried nothing"""
    da, orc = env
    case = cases(name, R, 4 if r == 16 else r)
    X = case.X if r != 16 else common.random_point(16, case.fx.d, case.fx.n, 4, orc.project_to_manifold)
    cfg = dict(case.cfg(mode="refusals", greedy=5), r=r, reserve=reserve)
    A = run_ranks(tmp_path / "refused", 2, cfg, X, case.v)
    B = run_ranks(tmp_path / "twin", 2, dict(cfg, mode="lift", lift=False), X)
    for k in range(2):
        a, b = A[k], B[k]
        assert list(a["status"]) == [BAD_ARG] * 5 + [beyond, UNSUPPORTED, UNSUPPORTED], a["status"]
        assert bool(a["unchanged"]) and int(a["r"]) == r
        for key in ("g_selected", "g_cost", "g_gradnorm", "X_greedy"):
            assert np.array_equal(a[key], b[key]), (k, key)
        assert np.array_equal(a["X"], a["X_greedy"])


def test_reserve_rank_arguments(env, cases):
    """d <= r <= r_reserve <= 16, before the exchange exists; beyond the reserve a one-rank exchange refuses too"""
    da, orc = env
    case = cases("smallGrid3D", 4, 4)
    s = case.fx.session(da, 4)
    for bad in (3, 17, 0, -1):
        with pytest.raises(da.DcoraError) as e:
            s.reserve_rank(bad)
        assert e.value.status == BAD_ARG
    s.reserve_rank(4)
    s.reserve_rank(5)
    ex = da.Exchange(s, "q%s" % uuid.uuid4().hex[:12])
    with pytest.raises(da.DcoraError) as e:
        s.reserve_rank(6)
    assert e.value.status == UNSUPPORTED
    ex.set_X(case.X)
    escaped, _ = ex.lift(case.theta, case.v)
    assert escaped and s.r == 5
    X5 = ex.gather_X()
    with pytest.raises(da.DcoraError) as e:
        ex.lift(-1.0, np.ones(case.fx.k))
    assert e.value.status == UNSUPPORTED and "reserve" in str(e.value) and s.r == 5
    assert np.array_equal(ex.gather_X(), X5)
    ex.close()
    s.close()
    with pytest.raises(da.DcoraError) as e:  # the reserved creators check before anything is built
        da.robust_ranked_session(case.fx.ds, "z%s" % uuid.uuid4().hex[:12], num_robots=4, r=4, r_reserve=3)
    assert e.value.status == BAD_ARG


# ---- (e) state survives -------------------------------------------------------------------------------------------------
def _robust_job_keeps_its_state(res, single, mu_step):
    """res: the ranks' records (lift_ranks_worker.py, mode "robust"); single(theta, v) -> the single-process robust
    session's record of the same flow with the same direction"""
    o0 = res[0]
    ref = single(float(o0["theta"]), o0["v"])
    for k, o in enumerate(res):
        assert not bool(o["cert"]) and bool(o["escaped"]) and int(o["r"]) == ref["r"], k
        assert float(o["theta"]) == float(o0["theta"]) and np.array_equal(o["v"], o0["v"])  # one direction on all ranks
        assert np.array_equal(o["X_before"], ref["X_before"]), k
        assert (int(o["trials"]), float(o["alpha"])) == (ref["trials"], ref["alpha"])
        # weights, mu, update count, team parameters and loop-closure counts unchanged by the lift
        assert np.array_equal(o["w_before"], o["w_after"]) and np.array_equal(o["w_after"], ref["w"])
        assert o["mu"][0] == o["mu"][1] == ref["mu"] and list(o["updates"]) == [2, 2]
        assert list(o["team"][0][:2]) == list(o["team"][1][:2]) and int(o["team"][1][2]) == 0
        assert bool(o["params_kept"]) and bool(o["lcs_kept"]) and bool(o["statuses_cleared"])
        assert np.abs(o["X"] - ref["X"]).max() <= 1e-12 * np.abs(ref["X"]).max()
        assert np.array_equal(o["X"], o0["X"])
        # the job goes on as the single-process lifted session does, and its next update gives the same weights
        assert np.array_equal(o["g_selected"], ref["g_selected"])
        assert np.allclose(o["g_cost"], ref["g_cost"], rtol=1e-11, atol=0)
        assert np.array_equal(o["X_run"], ref["X_run"]), (k, np.abs(o["X_run"] - ref["X_run"]).max())
        assert np.array_equal(o["w_next"], ref["w_next"]), k
        assert list(o["counts"]) == ref["counts"]
        assert int(o["updates_next"]) == 3 and float(o["mu_next"]) == ref["mu_next"]
        assert float(o["mu_next"]) == pytest.approx(ref["mu"] * mu_step, rel=1e-12)


def _single_robust_flow(A, X0, tol, theta, v):
    A.set_X(X0)
    for _ in range(2):
        A.run(max_iters=5, rgrad_tol=0.0)
        A.update_weights()
    out = dict(X_before=A.get_X(), w=A.get_weights(), mu=A.robust_info()["mu"])
    escaped, info = A.lift(theta, v, **tol)
    assert escaped
    out.update(r=A.r, trials=info["trials"], alpha=info["alpha"], X=A.get_X())
    g = A.run(max_iters=12, rgrad_tol=0.0)
    c = A.update_weights()
    out.update(g_cost=g["cost"], g_selected=g["selected"], X_run=A.get_X(), w_next=A.get_weights(),
               counts=[c["accepted"], c["rejected"], c["undecided"]], mu_next=A.robust_info()["mu"])
    A.close()
    return out


def test_robust_pose_graph_job_keeps_its_state(env, tmp_path):
    da, orc = env
    from dcora_amd import robust as rb
    from test_session_lift_gpu import GNC, _with_outliers
    R, r = 5, 5
    clean = common.product_dataset("smallGrid3D")
    ds = _with_outliers(da.Dataset, clean, 12, seed=2)
    X0 = np.zeros((r, 4 * ds.n))
    X0[:3] = da.chordal_initialization(clean)
    np.save(os.path.join(str(tmp_path), "ids.npy"), ds.ids)
    np.save(os.path.join(str(tmp_path), "vals.npy"), ds.vals)
    cfg = dict(kind="pgo", name="smallGrid3D", R=R, r=r, reserve=r + 1, d=ds.d, n=ds.n, mode="robust", gnc=GNC,
               team_iters=20, eta=ETA, tol=PGO_TOL)
    res = run_ranks(tmp_path, 2, cfg, X0)

    def single(theta, v):
        A = da.RbcdSession(da.Dataset(ds.d, ds.n, ds.ids.copy(), ds.vals.copy()), num_robots=R, r=r,
                           robust=rb.RobustCostParameters("GNC_TLS", **GNC))
        A.enable_team(max_num_iters=20)
        return _single_robust_flow(A, X0, PGO_TOL, theta, v)
    _robust_job_keeps_its_state(res, single, GNC["GNCMuStep"])


def test_robust_range_aided_job_keeps_its_state(env, tmp_path):
    """the loop-closure variant of tiers the range-aided GNC tests use (ra_loops.GNC_FIXTURE), rank 3 -> 4"""
    da, orc = env
    import ra_loops
    from dcora_amd import robust as rb
    path = ra_loops.write_loops_variant(tmp_path, **ra_loops.GNC_FIXTURE)[0]
    ra = da.RADataset(path)
    r = 3
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    cfg = dict(kind="ra", path=path, r=r, reserve=r + 1, mode="robust", gnc=ra_loops.GNC_PARAMS, team_iters=12, eta=ETA,
               tol=RA_TOL, restart_interval=5)
    res = run_ranks(tmp_path / "job", 2, cfg, X0)

    def single(theta, v):
        A = da.RaRbcdSession(da.RADataset(path), r, restart_interval=5,
                             robust=rb.RobustCostParameters("GNC_TLS", **ra_loops.GNC_PARAMS))
        A.enable_team(max_num_iters=12)
        return _single_robust_flow(A, X0, RA_TOL, theta, v)
    _robust_job_keeps_its_state(res, single, ra_loops.GNC_PARAMS["GNCMuStep"])


# ---- (g) a real staircase across 2 ranks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,R,r_min,seed", [("tinyGrid3D", 3, 3, 21), ("smallGrid3D", 5, 3, 4)])
def test_pose_graph_staircase_across_two_ranks(env, tmp_path, name, R, r_min, seed):
    """tests/test_session_lift_gpu.py::test_pose_graph_staircase_in_one_session's cases through
    driver.multi_robot_staircase_ranks"""
    da, orc = env
    from dcora_amd import driver
    ds, dso = common.product_dataset(name), common.oracle_dataset(name)
    X0 = common.random_point(r_min, ds.d, ds.n, seed, orc.project_to_manifold)
    kw = dict(num_robots=R, r_min=r_min, r_max=r_min + 6, max_iters=400, rgrad_tol=0.05)
    ref = driver.multi_robot_staircase_session(ds, X0, **kw)
    res = run_ranks(tmp_path, 2, dict(kind="pgo", name=name, R=R, r=r_min, reserve=0, mode="staircase", kw=kw), X0)
    print("%s: ranks %s, final 2f %.9g (one session: rank %d, 2f %.9g)" %
          (name, list(res[0]["ranks"]), float(res[0]["cost_2f"]), ref["rank"], ref["levels"][-1]["cost_2f"]))
    f_ref = ref["levels"][-1]["cost_2f"]
    for o in res:
        assert bool(o["certified"]) and ref["certified"]
        assert int(o["rank"]) == ref["rank"] and o["X"].shape == (ref["rank"], (ds.d + 1) * ds.n)
        assert list(o["ranks"]) == list(range(r_min, ref["rank"] + 1)) and bool(np.all(o["escaped"]))
        assert abs(float(o["cost_2f"]) - f_ref) < 1e-3 * abs(f_ref)
        assert np.array_equal(o["X"], res[0]["X"])
    So = orc.dual_certificate(ref["rank"], ds.d, ds.n, res[0]["X"], orc.build_Q_pgo(dso))
    assert orc.fast_verification(So, 1e-3, block=ds.d + 1)[0]


@pytest.mark.parametrize("name", ["range_aided_slam_test_2d", "range_aided_slam_test_3d"])
def test_range_aided_staircase_across_two_ranks(env, tmp_path, name):
    """tests/test_session_lift_gpu.py::test_range_aided_staircase_in_one_session's cases through
    driver.raslam_staircase_ranks"""
    da, orc = env
    from dcora_amd import driver
    ra = da.RADataset(ra_path(name))
    d = ra.d
    rng = np.random.default_rng(12)
    X0 = orc.project_to_manifold(d, d, ra.n, rng.standard_normal((d, ra.k)), l=ra.l, b=ra.b)
    kw = dict(max_iters=300, rgrad_tol=1e-3, r_max=d + 5)
    ref = driver.raslam_staircase_session(ra, X0, **kw)
    res = run_ranks(tmp_path, 2, dict(kind="ra", path=ra_path(name), r=d, reserve=0, mode="staircase", kw=kw), X0)
    print("%s: ranks %s, final 2f %.3g (one session: rank %d)" % (name, list(res[0]["ranks"]),
                                                                  float(res[0]["cost_2f"]), ref["rank"]))
    for o in res:
        assert bool(o["certified"]) and ref["certified"]
        assert int(o["rank"]) == ref["rank"] > d and bool(np.all(o["escaped"]))
        assert float(o["cost_2f"]) < 1e-3
        assert np.array_equal(o["X"], res[0]["X"])
    So = orc.dual_certificate(ref["rank"], d, ra.n, res[0]["X"], orc.CSR.from_scipy(ra.Q.to_scipy()), l=ra.l, b=ra.b)
    assert orc.fast_verification(So, 1e-3, block=1)[0]
