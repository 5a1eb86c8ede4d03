"""The certificate of a multi-rank job formed from the matrices its ranks hold on the device, with the job's current
weights (dcora_exchange_certify_live; ref src/DCORA_utils.cpp:1713-1735, 1898-1982, examples/MultiRobotExample.cpp:321-335).
One process per rank (tests/certify_ranks_worker.py), all on device 0 where there is one GPU.

The reference of every comparison is the path the suite pins to the oracle: da.dual_certificate + da.fast_verification on
one GPU with a host Q built from the job's weights, at the gathered X; the worker also calls dcora_exchange_certify with
that Q.  Tolerances: tests/test_exchange_gpu.py::test_certification_across_ranks_matches_one_gpu's and its range-aided
twin's -- |lambda - ref| <= 1e-6 max(1, |ref|), | |v| - 1 | <= 1e-9, |theta - v'S_ref v| <= 1e-9 max(1, |theta|),
|theta - theta_ref| <= 1e-5 max(1, |theta_ref|), v up to its sign within 1e-3, the eigen-residual below
1e-3 max(1, |lambda|) (range-aided: 1e-3 + 1e-4 |A|_1), identical bits on every rank.  eta = 1e-3 everywhere.
(info10: [0] is the symbolic phase's ms and [1] the numeric phase's, as dcora_cert_is_psd_device fills them.)"""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import common
from test_raslam import ra_path
from test_session_certify_gpu import _with_outliers

pytestmark = pytest.mark.gpu

WORKER = os.path.join(common.HERE, "certify_ranks_worker.py")
ETA = 1e-3


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


@pytest.fixture(scope="module")
def grid(env):
    """smallGrid3D, its host Q and the random point of tests/test_session_certify_gpu.py (seed 4); left unchanged"""
    da, orc = env
    ds = common.product_dataset("smallGrid3D")
    return ds, da.build_Q_pgo(ds), common.random_point(5, ds.d, ds.n, 4, orc.project_to_manifold)


def run_ranks(tmp_path, world, scenario, transport=None, **spec):
    np.savez(os.path.join(str(tmp_path), "spec.npz"), **spec)
    job = "c%s" % uuid.uuid4().hex[:12]
    env = dict(os.environ)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env.pop("DCORA_EXCHANGE_WAIT", None)
    if transport:
        env["DCORA_EXCHANGE"] = transport
    else:
        env.pop("DCORA_EXCHANGE", None)
    procs = [subprocess.Popen([sys.executable, WORKER, str(k), str(world), job, scenario, str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for k in range(world)]
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
    res = []
    for k in range(world):  # (read now: a test that runs two jobs uses the directory twice)
        with np.load(os.path.join(str(tmp_path), "rank%d.npz" % k)) as f:
            res.append({key: f[key] for key in f.files})
    return res


def reference(da, r, dims, X, Q, block):
    d, n, l, b = dims
    S = da.dual_certificate(r, d, n, X, Q, l=l, b=b)
    return S, da.fast_verification(S, ETA, block=block)


def check_refused(tag, res, i, S, ref, range_aided=False, distributed=True):
    """record i of every rank against the one-GPU reference (refused), and the ranks against each other"""
    psd, theta, v, lmin = ref
    A = S.to_scipy()
    assert not psd, "the host path accepts this point: the case shows nothing"
    p = "c%d_" % i
    for k, o in enumerate(res):
        lam, th, vv = float(o[p + "lambda"]), float(o[p + "theta"]), o[p + "v"]
        resid = np.linalg.norm(A @ vv + ETA * vv - lam * vv)
        print("%s rank %d: lambda %.12g / ref %.12g, theta %.12g / ref %.12g, |v| - 1 %.3g, theta - v'Sv %.3g, "
              "v up to sign %.3g, residual %.3g, matvecs %d, distributed %d (dcora_exchange_certify: %d, %d), rounds %d, "
              "%.3f ms" %
              (tag, k, lam, lmin, th, theta, np.linalg.norm(vv) - 1, th - vv @ (A @ vv),
               min(np.linalg.norm(vv - v), np.linalg.norm(vv + v)), resid, int(o[p + "matvecs"]),
               int(o[p + "distributed"]), int(o[p + "host_matvecs"]), int(o[p + "host_distributed"]),
               int(o[p + "info10"][8]), float(o[p + "info10"][9])))
        assert not bool(o[p + "ok"])
        assert not bool(o[p + "host_ok"]), "dcora_exchange_certify accepts what certify_live refuses"
        assert int(o[p + "matvecs"]) > 0
        assert abs(lam - lmin) <= 1e-6 * max(1.0, abs(lmin))
        assert abs(np.linalg.norm(vv) - 1) <= 1e-9
        assert abs(th - vv @ (A @ vv)) <= 1e-9 * max(1.0, abs(th))
        assert abs(th - theta) <= 1e-5 * max(1.0, abs(theta))
        assert min(np.linalg.norm(vv - v), np.linalg.norm(vv + v)) < 1e-3
        if range_aided:
            assert resid < 1e-3 + 1e-4 * spla.norm(A, 1)
        else:
            assert resid < 1e-3 * max(1.0, abs(lam))
        # every rank holds the same bits
        assert np.array_equal(vv, res[0][p + "v"]) and lam == float(res[0][p + "lambda"])
        assert th == float(res[0][p + "theta"]) and np.array_equal(o[p + "info10"], res[0][p + "info10"])
        assert np.array_equal(o[p + "X"], res[0][p + "X"])
        assert int(o[p + "matvecs"]) == int(res[0][p + "matvecs"])
    for o in res:
        assert bool(o[p + "distributed"]) == distributed


# ---- 1. refused, pose graph ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,transport", [(1, None), (2, None), (4, "staged")])
def test_refused_point_of_a_pose_graph(env, grid, tmp_path, world, transport):
    da, orc = env
    ds, Q, X0 = grid
    res = run_ranks(tmp_path, world, "refused", transport, name="smallGrid3D", R=5, r=5, iters=6, X0=X0)
    if world > 1:
        assert all(int(o["mode"]) == (2 if transport == "staged" else 1) for o in res)
    assert int(res[0]["c0_info10"][8]) >= 3, "the windows do not cut through the agents' row blocks"
    S, ref = reference(da, 5, (ds.d, ds.n, 0, 0), res[0]["c0_X"], Q, ds.d + 1)
    check_refused("smallGrid3D world %d" % world, res, 0, S, ref)


# ---- 2. accepted ----------------------------------------------------------------------------------------------------------
def test_accepted_certificate_moves_only_the_verdict(env, grid, tmp_path):
    da, orc = env
    ds, Q, _ = grid
    X0 = np.zeros((5, 4 * ds.n))
    X0[:3] = da.chordal_initialization(ds)
    P = da.QuadraticProblem(5, ds.d, ds.n, Q)
    opt = da.QuadraticOptimizer(P, da.ROptParameters(RTR_iterations=100, RTR_tCG_iterations=200, gradnorm_tol=1e-6))
    X = opt.optimize(X0)
    assert opt.getOptResult()["gradNormOpt"] < 1e-6
    P.close()
    S, ref = reference(da, 5, (ds.d, ds.n, 0, 0), X, Q, ds.d + 1)
    assert ref[0], "the host path must accept this point, or the case shows nothing"
    res = run_ranks(tmp_path, 2, "accepted", name="smallGrid3D", R=5, r=5, iters=0, X0=X)
    for o in res:
        print("optimum: ok %s, info10 %s" % (bool(o["c0_ok"]), o["c0_info10"]))
        assert np.array_equal(o["c0_X"], X)
        assert bool(o["c0_ok"]) and bool(o["c0_host_ok"])
        assert int(o["c0_matvecs"]) == 0
        assert float(o["c0_info10"][1]) > 0, "no numeric phase was reported"
        assert np.array_equal(o["c0_info10"], res[0]["c0_info10"])


# ---- 3. the job's current weights ----------------------------------------------------------------------------------------
def test_current_weights_of_a_robust_job(env, tmp_path):
    da, orc = env
    from dcora_amd import driver
    R, r = 5, 5
    ds = _with_outliers(da.Dataset, common.product_dataset("smallGrid3D"), 12, seed=2)
    lc = driver.loop_closure_mask(ds, R)
    X0 = common.random_point(r, ds.d, ds.n, 4, orc.project_to_manifold)
    rng = np.random.default_rng(11)
    w2 = ds.vals[:, -1].copy()
    w2[lc] = 1.0
    kind = rng.integers(0, 3, int(lc.sum()))
    w2[lc] = np.where(kind == 0, 0.0, np.where(kind == 1, rng.uniform(0.2, 0.9, kind.size), 1.0))
    assert np.any(w2[lc] == 0) and np.any(w2[lc] == 1) and np.any((w2[lc] > 0) & (w2[lc] < 1))
    res = run_ranks(tmp_path, 2, "weights", name="smallGrid3D", R=R, r=r, iters=0, X0=X0, ids=ds.ids, vals=ds.vals, w2=w2)
    assert np.array_equal(res[0]["w1"], w2)
    for i in (0, 1):
        with_w = da.Dataset(ds.d, ds.n, ds.ids.copy(), ds.vals.copy())
        with_w.vals[:, -1] = res[0]["w%d" % i]
        S, ref = reference(da, r, (ds.d, ds.n, 0, 0), res[0]["c%d_X" % i], da.build_Q_pgo(with_w), ds.d + 1)
        check_refused("robust job, weights %d" % i, res, i, S, ref)
    assert float(res[0]["c0_theta"]) != float(res[0]["c1_theta"])  # (stale values would repeat the first)


# ---- 4. entries of Lambda absent from Q's pattern ---------------------------------------------------------------------
def test_entries_of_lambda_absent_from_the_pattern_of_Q(env, tmp_path):
    da, orc = env
    ds = common.product_dataset("sphere2500")
    Q = da.build_Q_pgo(ds)
    X0 = common.random_point(5, ds.d, ds.n, 4, orc.project_to_manifold)
    res = run_ranks(tmp_path, 2, "refused", name="sphere2500", R=5, r=5, iters=0, X0=X0)
    S, ref = reference(da, 5, (ds.d, ds.n, 0, 0), res[0]["c0_X"], Q, ds.d + 1)
    assert int(S.rp[-1]) > int(Q.rp[-1])
    check_refused("sphere2500", res, 0, S, ref)


# ---- 5. range-aided ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r,iters,transport", [
    ("range_aided_slam_test_3d", 4, 6, None),
    ("range_aided_slam_test_2d", 3, 6, "staged"),
    ("tiers", 3, 4, None),  # the row-block runs do not converge: the eigenpair is rank 0's, on the downloaded values
])
def test_range_aided_jobs(env, tmp_path, name, r, iters, transport):
    """On tiers the eigenpair is rank 0's, from its shift-and-invert run on the downloaded values (distributed == 0):
    eta / lambda_max is 5e-10 there, and certify_live follows the one-GPU rule (device_min_eig) of not attempting the
    spectrum-shifted row-block run on such a spectrum."""
    da, orc = env
    ra = da.RADataset(ra_path(name))
    if name == "tiers":
        X0 = np.zeros((r, ra.k))
        X0[:ra.d] = ra.X_odom
    else:
        X0 = da.manifold_project(r, ra.d, ra.n, np.random.default_rng(7).standard_normal((r, ra.k)), l=ra.l, b=ra.b)
    res = run_ranks(tmp_path, 2, "ra", transport, name=name, R=0, r=r, iters=iters, X0=X0)
    S, ref = reference(da, r, (ra.d, ra.n, ra.l, ra.b), res[0]["c0_X"], ra.Q, 1)
    check_refused(name, res, 0, S, ref, range_aided=True, distributed=name != "tiers")


# ---- 6. across a lift -----------------------------------------------------------------------------------------------------
def test_certificate_across_a_lift(env, tmp_path):
    da, orc = env
    ds = common.product_dataset("smallGrid3D")
    Q = da.build_Q_pgo(ds)
    X0 = common.random_point(4, ds.d, ds.n, 4, orc.project_to_manifold)
    res = run_ranks(tmp_path, 2, "lift", name="smallGrid3D", R=5, r=4, iters=6, X0=X0)
    assert all(bool(o["escaped"]) and int(o["r_after"]) == 5 for o in res)
    assert res[0]["c0_X"].shape[0] == 4 and res[0]["c1_X"].shape[0] == 5
    for i, r in ((0, 4), (1, 5)):
        S, ref = reference(da, r, (ds.d, ds.n, 0, 0), res[0]["c%d_X" % i], Q, ds.d + 1)
        check_refused("smallGrid3D at r = %d" % r, res, i, S, ref)


# ---- 7. the job is left alone -------------------------------------------------------------------------------------------
def test_certify_live_leaves_the_job_alone(env, grid, tmp_path):
    ds, Q, X0 = grid
    a = run_ranks(tmp_path, 2, "alone", name="smallGrid3D", R=5, r=5, iters=0, X0=X0)
    b = run_ranks(tmp_path, 2, "alone_plain", name="smallGrid3D", R=5, r=5, iters=0, X0=X0)
    for o, q in zip(a, b):
        assert bool(o["refused"]) and bool(o["same_bits"]), "two calls in a row returned different bits"
        for key in ("X", "cost", "selected"):
            assert o[key].shape == q[key].shape and np.array_equal(o[key], q[key]), key
        assert o["cost"].size == 16


# ---- 8. usage errors ----------------------------------------------------------------------------------------------------------
def test_usage_errors_are_refused_everywhere_and_leave_the_job_usable(env, grid, tmp_path):
    da, orc = env
    ds, Q, X0 = grid
    res = run_ranks(tmp_path, 2, "usage", name="smallGrid3D", R=5, r=5, iters=6, X0=X0)
    for o in res:
        assert list(o["codes"]) == [1, 1, 1], "DCORA_ERR_BAD_ARG expected for certified NULL, eta nan, eta < 0"
        assert bool(o["finite_after"])
    S, ref = reference(da, 5, (ds.d, ds.n, 0, 0), res[0]["c0_X"], Q, ds.d + 1)
    check_refused("after the refusals", res, 0, S, ref)


# ---- 9. the analysis cache ---------------------------------------------------------------------------------------------
def test_analysis_cache_is_shared_with_cert_prepare(env, grid, tmp_path):
    ds, Q, X0 = grid
    res = run_ranks(tmp_path, 2, "cache", name="smallGrid3D", R=5, r=5, iters=6, X0=X0)
    i10 = res[0]["c0_info10"]
    print("after cert_prepare on rank 0: symbolic %.3f ms, numeric %.3f ms" % (i10[0], i10[1]))
    assert i10[0] == 0
    assert i10[1] > 0


# ---- 10. the driver ---------------------------------------------------------------------------------------------------------
def test_staircase_driver_with_the_live_certificate(env, tmp_path):
    da, orc = env
    ds = common.product_dataset("smallGrid3D")
    X0 = common.random_point(3, ds.d, ds.n, 4, orc.project_to_manifold)
    res = run_ranks(tmp_path, 2, "driver", name="smallGrid3D", R=5, r=3, iters=400, rgrad_tol=0.05, X0=X0)
    for o in res:
        print("host: ranks %s certified %s 2f %.12g; live: ranks %s certified %s 2f %.12g" %
              (list(o["host_ranks"]), bool(o["host_certified"]), float(o["host_cost_2f"]), list(o["live_ranks"]),
               bool(o["live_certified"]), float(o["live_cost_2f"])))
        assert int(o["live_rank"]) == int(o["host_rank"])
        assert bool(o["live_certified"]) == bool(o["host_certified"]) is True
        assert abs(float(o["live_cost_2f"]) - float(o["host_cost_2f"])) <= 1e-9 * abs(float(o["host_cost_2f"]))
