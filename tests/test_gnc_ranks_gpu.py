"""Robust weights updated inside a multi-rank RBCD job (dcora_rbcd_create_robust_ranks, dcora_exchange_update_weights /
_set_weights / _get_weights; Agent::updateMeasurementWeights of every agent on every rank, ref src/Agent.cpp:1397-1441):
several processes (one per rank, all on device 0) must reproduce the single-process robust session -- weights, counts,
selected agents and X bit for bit, costs to rounding (the evaluation sums per agent) -- and reject the injected
outliers.  Refusals are the same on every rank and leave the job as it was."""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

WORKER = os.path.join(common.HERE, "gnc_ranks_worker.py")
GNC = dict(GNCBarc=10.0, GNCMuStep=2.0)  # as tests/test_gnc_distributed.py
FAST = dict(GNCBarc=10.0, GNCMuStep=4.0)  # rejects within a few updates


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    if dcora_amd.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return dcora_amd


def _with_outliers(ds_cls, base, n_out, seed):
    # (as tests/test_gnc_distributed.py builds them)
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


def _problem(da, name, n_out, seed, r=5):
    """the dataset with its outliers and X0 = the chordal initialisation of the clean graph, lifted to rank r"""
    clean = common.product_dataset(name)
    T = da.chordal_initialization(clean)
    X0 = np.zeros((r, (clean.d + 1) * clean.n))
    X0[:clean.d] = T
    return clean, _with_outliers(da.Dataset, clean, n_out, seed), X0


def _copy(da, ds):
    return da.Dataset(ds.d, ds.n, ds.ids.copy(), ds.vals.copy())


def run_ranks(tmp_path, world, ds, X0, cfg, transport=None, fixed=None, X1=None):
    d = str(tmp_path)
    np.save(os.path.join(d, "ids.npy"), ds.ids)
    np.save(os.path.join(d, "vals.npy"), ds.vals)
    np.save(os.path.join(d, "X0.npy"), X0)
    if fixed is not None:
        np.save(os.path.join(d, "fixed.npy"), fixed)
    if X1 is not None:
        np.save(os.path.join(d, "X1.npy"), X1)
    cfg = dict(cfg, d=ds.d, n=ds.n, fixed=fixed is not None)
    with open(os.path.join(d, "job.json"), "w") as f:
        json.dump(cfg, f)
    job = "g%s" % uuid.uuid4().hex[:12]
    env = dict(os.environ)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env.pop("DCORA_EXCHANGE_WAIT", None)
    if transport:
        env["DCORA_EXCHANGE"] = transport
    else:
        env.pop("DCORA_EXCHANGE", None)
    procs = [subprocess.Popen([sys.executable, WORKER, str(k), str(world), job, d], env=env, stdout=subprocess.PIPE,
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


def single_gnc(da, ds, X0, R, r, params, rounds, inner, final, fixed=None):
    """multi_robot_gnc_session's calls with rgrad_tol 0, recording what every update gives"""
    s = da.RbcdSession(ds, num_robots=R, r=r, robust=params, fixed_weight=fixed)
    s.set_X(X0)
    runs, counts, W, info = [], [], [], []
    for _ in range(rounds):
        runs.append(s.run(max_iters=inner, rgrad_tol=0.0))
        c = s.update_weights()
        counts.append([c["accepted"], c["rejected"], c["undecided"]])
        W.append(s.get_weights())
        i = s.robust_info()
        info.append([i["mu"], i["updates"]])
    runs.append(s.run(max_iters=final, rgrad_tol=0.0))
    X = s.get_X()
    s.close()
    cat = lambda key: np.concatenate([q[key] for q in runs])
    return dict(counts=np.array(counts), W=np.array(W), info=np.array(info), cost=cat("cost"),
                gradnorm=cat("gradnorm"), selected=cat("selected"), X=X)


def touching_mask(ds, R, world, rank):
    """the measurements touching an agent of `rank` (consecutive agents share a rank, agents own contiguous poses)"""
    per_pose = ds.n // R
    agent = np.minimum(ds.ids[:, [1, 3]] // per_pose, R - 1)
    per_rank = (R + world - 1) // world
    return np.any(agent // per_rank == rank, axis=1)


CASES = [
    # dataset, outliers, agents, ranks, transport
    ("smallGrid3D", 12, 5, 2, None),
    ("smallGrid3D", 12, 5, 4, None),       # rank 3 hosts no agent
    ("sphere2500", 20, 5, 2, None),        # the dense preconditioner path
    ("torus3D", 20, 8, 4, None),           # sparse partitioned preconditioners, rebuilt through the cache
    ("smallGrid3D", 12, 5, 2, "staged"),   # the shared-host-segment transport
]


@pytest.mark.parametrize("name,n_out,R,world,transport", CASES)
def test_ranks_reproduce_the_single_process(da, tmp_path, name, n_out, R, world, transport):
    from dcora_amd import driver
    from dcora_amd import robust as rb
    r, rounds, inner, final = 5, 6, 8, 10
    clean, ds, X0 = _problem(da, name, n_out, seed=2)
    params = rb.RobustCostParameters("GNC_TLS", **FAST)
    ref = single_gnc(da, _copy(da, ds), X0, R, r, params, rounds, inner, final)
    assert ref["counts"][:, 1].max() > 0, "no update rejected anything: the case shows too little"
    # the driver's own single-process flow lands on the same X
    sess = driver.multi_robot_gnc_session(_copy(da, ds), X0, num_robots=R, r=r, robust=params,
                                          num_weight_updates=rounds, inner_iters=inner, rgrad_tol=0.0,
                                          max_final_iters=final)
    assert np.array_equal(sess["X"], ref["X"]) and np.array_equal(sess["weights"], ref["W"][-1])
    res = run_ranks(tmp_path, world, ds, X0, dict(mode="compare", R=R, r=r, rounds=rounds, inner=inner, final=final,
                                                  gnc=FAST), transport=transport)
    lc = driver.loop_closure_mask(ds, R)
    w_start = ds.vals[:, -1].copy()
    w_start[lc] = 1.0
    for k, o in enumerate(res):
        assert np.array_equal(o["counts"], ref["counts"]), (k, o["counts"], ref["counts"])
        assert np.array_equal(o["W0"], w_start)
        for u in range(rounds):
            assert np.array_equal(o["W"][u], ref["W"][u]), (k, u, np.nanmax(np.abs(o["W"][u] - ref["W"][u])))
        assert np.array_equal(o["selected"], ref["selected"])
        assert np.allclose(o["cost"], ref["cost"], rtol=1e-11, atol=0), (k, np.max(np.abs(o["cost"] / ref["cost"] - 1)))
        assert np.allclose(o["gradnorm"], ref["gradnorm"], rtol=1e-9, atol=0)
        assert np.array_equal(o["X"], ref["X"]), (k, np.max(np.abs(o["X"] - ref["X"])))
        assert np.array_equal(o["info"], ref["info"])
        # this rank's view: every measurement touching one of its agents, NaN elsewhere, the job's bits where set
        mine = touching_mask(ds, R, world, k)
        for u, loc in enumerate([o["local0"]] + list(o["local"])):
            assert np.array_equal(~np.isnan(loc), mine), (k, u)
            assert np.array_equal(loc[mine], ([o["W0"]] + list(o["W"]))[u][mine]), (k, u)
    if world == 4 and R == 5:
        assert not touching_mask(ds, R, world, 3).any()  # (the rank without agents took part all the same)


def test_gnc_across_ranks_rejects_the_injected_outliers(da, tmp_path):
    from dcora_amd import driver
    from dcora_amd import robust as rb
    R, r, world, n_out = 5, 5, 2, 12
    clean, ds, X0 = _problem(da, "smallGrid3D", n_out, seed=2)
    res = run_ranks(tmp_path, world, ds, X0, dict(mode="driver", R=R, r=r, rounds=20, inner=30, final=1000,
                                                  rgrad_tol=0.1, gnc=GNC))
    lc = driver.loop_closure_mask(ds, R)
    m0 = clean.m
    for o in res:
        w = o["weights"]
        assert np.array_equal(o["ds_weights"], w)
        assert np.all(w[m0:] < 1e-8), "every injected closure is rejected"
        assert np.all(w[:m0][lc[:m0]] > 1 - 1e-8), "every original closure is kept"
        assert np.all(w[~lc] == 1.0)
        assert int(o["rejected"][-1]) == n_out
        assert np.array_equal(o["X"], res[0]["X"]) and float(o["cost"]) == float(res[0]["cost"])
        assert np.array_equal(w, res[0]["weights"])
    assert abs(float(res[0]["cost"]) - 1025.398) < 0.05  # the optimum the single-process flow reaches


def test_reset_and_refusals_are_collective(da, tmp_path):
    from dcora_amd import driver
    from dcora_amd import robust as rb
    R, r, world = 5, 5, 2
    clean, ds, X0 = _problem(da, "smallGrid3D", 12, seed=2)
    lc = driver.loop_closure_mask(ds, R)
    fixed = np.zeros(ds.m, bool)
    zero_edge = int(np.nonzero(lc)[0][0])
    fixed[zero_edge] = True
    ds.vals[zero_edge, -1] = 0.0  # a fixed weight 0: not in the sessions' patterns
    X1 = common.random_point(r, ds.d, ds.n, 4, da.manifold_project)
    params = rb.RobustCostParameters("GNC_TLS", **FAST)
    res = run_ranks(tmp_path, world, ds, X0, dict(mode="refusals", R=R, r=r, gnc=FAST, edge=3, zero_edge=zero_edge),
                    fixed=fixed, X1=X1)
    # the single-process reference of what the job did around its refusals
    s = da.RbcdSession(_copy(da, ds), num_robots=R, r=r, robust=params, fixed_weight=fixed)
    s.set_X(X0)
    runs = [s.run(max_iters=7, rgrad_tol=0.0), s.run(max_iters=12, rgrad_tol=0.0)]
    c = s.update_weights()
    W = s.get_weights()
    runs.append(s.run(max_iters=5, rgrad_tol=0.0))
    X_after = s.get_X()
    s.close()
    for k, o in enumerate(res):
        assert list(o["status"]) == [1, 1, 1, 1, 8, 8], (k, o["status"])
        assert bool(o["unchanged"])
        assert list(o["counts"][0]) == [c["accepted"], c["rejected"], c["undecided"]]
        assert np.array_equal(o["W"][0], W)
        assert np.array_equal(o["selected"], np.concatenate([q["selected"] for q in runs]))
        assert np.array_equal(o["X_after"], X_after), k
        assert np.array_equal(o["X_reset"], X1), k
        assert int(o["info"][0][1]) == 2


def test_one_rank_through_the_new_creator_is_the_robust_session(da):
    """world_size 1 through dcora_rbcd_create_robust_ranks: bitwise the session of dcora_rbcd_create_robust over a short
    GNC run (no subprocess); the session-level weight changes are refused, the view and robust_info are the session's"""
    from dcora_amd import capi, driver
    from dcora_amd import robust as rb
    R, r = 5, 5
    clean, ds, X0 = _problem(da, "smallGrid3D", 12, seed=2)
    params = rb.RobustCostParameters("GNC_TLS", **FAST)
    A = da.RbcdSession(_copy(da, ds), num_robots=R, r=r, robust=params)
    B, ex = da.robust_ranked_session(_copy(da, ds), "w1%s" % uuid.uuid4().hex[:10], num_robots=R, r=r, robust=params)
    try:
        A.set_X(X0)
        ex.set_X(X0)
        assert np.array_equal(A.get_weights(), ex.get_weights())
        for _ in range(5):
            a, b = A.run(max_iters=8, rgrad_tol=0.0), B.run(max_iters=8, rgrad_tol=0.0)
            for key in ("cost", "gradnorm", "selected"):
                assert np.array_equal(a[key], b[key]), key
            assert A.update_weights() == ex.update_weights()
            wa = A.get_weights()
            assert np.array_equal(wa, ex.get_weights()) and np.array_equal(wa, B.get_weights())
            assert A.robust_info() == B.robust_info()
            assert np.array_equal(A.get_X(), ex.gather_X())
        for call in (lambda: B.update_weights(), lambda: B.set_weights(wa)):
            with pytest.raises(capi.DcoraError) as e:
                call()
            assert e.value.status == 8 and "dcora_exchange_" in str(e.value)
        ex.set_weights(wa * 0.5)
        A.set_weights(wa * 0.5)
        assert np.array_equal(ex.get_weights(), A.get_weights())
        a, b = A.run(max_iters=6, rgrad_tol=0.0), B.run(max_iters=6, rgrad_tol=0.0)
        assert np.array_equal(a["cost"], b["cost"]) and np.array_equal(A.get_X(), B.get_X())
    finally:
        ex.close()
        B.close()
        A.close()
    # the SPMD driver at one rank against the single-process flow: the same weights and X, costs to rounding
    kw = dict(num_robots=R, r=r, robust=params, num_weight_updates=4, inner_iters=8, rgrad_tol=0.0, max_final_iters=8)
    one = driver.multi_robot_gnc_session(_copy(da, ds), X0, **kw)
    ranks = driver.multi_robot_gnc_ranks(_copy(da, ds), X0, job_name="d1%s" % uuid.uuid4().hex[:10], **kw)
    assert np.array_equal(one["weights"], ranks["weights"]) and np.array_equal(one["X"], ranks["X"])
    assert [q["rejected"] for q in one["rounds"]] == [q["rejected"] for q in ranks["rounds"]]
    assert ranks["final"]["cost_2f"] == pytest.approx(one["final"]["cost_2f"], rel=1e-11, abs=0)


def test_plain_robust_session_still_refuses_ranks(da):
    from dcora_amd import capi
    from dcora_amd import robust as rb
    ds = common.product_dataset("smallGrid3D")
    with pytest.raises(capi.DcoraError) as e:
        da.RbcdSession(ds, num_robots=5, r=5, robust=rb.RobustCostParameters("GNC_TLS", **GNC), world_size=2)
    assert e.value.status == 8 and "dcora_rbcd_create_robust_ranks" in str(e.value)
