"""Projection of a multi-rank RBCD job to rank d on the device, collectively (dcora_exchange_project:
k_gram_blocks_mfma, k_gram_blocks_finish, Exchange::project; ref examples/SingleRobotExample_RASLAM.cpp:220-234,
projectSolutionRASLAM src/DCORA_utils.cpp:1984-2031).

Inputs and rules are those of tests/session_project_inputs.py and tests/test_session_project_gpu.py (_check_gram,
_check_spectrum, |P^T P - host-fed| <= 1e-10); tests/test_project_ranks_cpu.py holds the inputs to the two conditioning
rules without a GPU.  No tolerance of its own: between ranks, rank counts and transports everything is the same sum of
the same per-agent matrices in agent order and the same kernels block by block -- bit-equal; a projected job against a
fresh one at rank d is bit-equal as tests/test_session_project_gpu.py has it for sessions.
One process per rank, all on device 0, at most 4 ranks.

(e) The range-aided reflect family cannot be spread over two robots: dcora_radataset_create gives every state to robot
0.  The test therefore feeds the family's poses -- rotation blocks and translations of spi.reflect_case, in the SE
ordering -- to a pose-graph chain of 9 poses on two agents, one per rank (project_ranks_worker.reflect_chain_case)."""
import ctypes as C
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import block_factors as bf
import common
import project_ranks_worker as prw
import ra_loops
import session_project_inputs as spi
import session_round_inputs as sri
from test_raslam import ra_path
from test_session_project_gpu import (EXTRA_KEYS, GNC, PARENT_KEYS, ROUND_KEYS, _check_gram, _check_spectrum,
                                      _debug_gram, _driver_checks, _odometry_start, _with_outliers)

pytestmark = pytest.mark.gpu

WORKER = os.path.join(common.HERE, "project_ranks_worker.py")
EPS = bf.EPS
BAD_ARG = 1
ETA = 1e-3
FACTS = ("gram", "basis", "sigma", "positive_dets", "reflected", "projected", "cost_2f", "gradnorm", "X")
# dcora_debug_launch_count of ranks 0 and 1 of the twin job of test_rank_d_job_is_passed_through -- creation, set_X and
# 3 + 5 greedy iterations of smallGrid3D, 4 agents at rank 3 on 2 ranks, from the seed-4 point -- taken with a build of
# the commit before dcora_exchange_project existed
PARENT_LAUNCHES = (222, 140)


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


def run_ranks(tmp_path, world, cfg, X0, transport=None, files=None):
    d = str(tmp_path)
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "X0.npy"), X0)
    for name, arr in (files or {}).items():
        np.save(os.path.join(d, name), arr)
    with open(os.path.join(d, "job.json"), "w") as f:
        json.dump(cfg, f)
    job = "p%s" % uuid.uuid4().hex[:12]
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


def _same_on_every_rank(res, keys=FACTS):
    for k, o in enumerate(res[1:], 1):
        for key in keys:
            assert np.array_equal(o[key], res[0][key]), (k, key)


def _as_out(o):
    return dict(sigma=o["sigma"], projected=bool(o["projected"]), basis=o["basis"], gram=o["gram"])


def _check_against_reference(da, o, d, n, l, b, se, tag, lifted=False):
    """(b)'s checks on one rank's result -> the ratios observed.  lifted: the point is a lifted rank-d one (spi's), whose
    truncated blocks all have the same handedness"""
    X, P = o["X_before"], o["X"]
    r = X.shape[0]
    g = _check_gram(o["gram"], X, tag)
    rat = _check_spectrum(_as_out(o), X, d, tag)
    assert int(o["r"]) == d and bool(o["projected"]) and P.shape == (d, X.shape[1]), tag
    R = spi.rotation_blocks(P, d, n, l, se)
    assert (np.linalg.det(R) > 1 - 64 * EPS).all(), (tag, np.linalg.det(R).min())
    if se:
        H = da.project_solution_raslam(spi.ra_from_se(X, d, n), r, d, n, 0, 0)
        Pr = spi.ra_from_se(P, d, n)
    else:
        H, Pr = da.project_solution_raslam(X, r, d, n, l, b), P
    e_h = float(np.abs(Pr.T @ Pr - H.T @ H).max())
    assert e_h <= 1e-10, (tag, e_h)
    assert bool(o["reflected"]) == (int(o["positive_dets"]) < n // 2), tag
    assert not lifted or int(o["positive_dets"]) in (0, n), tag
    return g, rat, e_h


# ---- (a) the kernel pair ------------------------------------------------------------------------------------------------------
def _debug_gram_blocks(r, blocks):
    from dcora_amd import capi
    ks = np.array([B.shape[1] for B in blocks], np.int64)
    X = np.concatenate([capi.F(B) for B in blocks]) if ks.sum() else np.zeros(1)
    G, chunk = np.zeros(len(blocks) * r * r), C.c_int()
    capi.check(capi.lib().dcora_debug_project_gram_blocks(r, len(blocks), ks.ctypes.data_as(C.c_void_p),
                                                          np.ascontiguousarray(X), G, C.byref(chunk)))
    return [capi.unF(G[i * r * r:(i + 1) * r * r], r, r) for i in range(len(blocks))], chunk.value


@pytest.mark.parametrize("d", spi.DIMS)
def test_block_list_gram_equals_the_single_block_kernels(env, d):
    """every block's matrix is bit for bit dcora_debug_project_gram of that block alone -- wherever it stands in the
    list --, symmetric, NaN-free (every entry written), the same on a second call and within the (k + 2) eps bound"""
    chunk = _debug_gram(np.ones((2, 3)))[1]
    sizes = [1, 3, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 7]
    lists = [sizes, sizes[::-1], [chunk + 1, 1, 2 * chunk + 7, 5, chunk, 3, chunk - 1], [chunk + 1, 0, 5], [0, 3, 0],
             [2 * chunk + 7], [1]]
    worst = 0.0
    for r in spi.ranks_of(d):
        for li, ks in enumerate(lists):
            rng = np.random.default_rng(1000 * r + li)
            blocks = [rng.standard_normal((r, k)) for k in ks]
            Gs, ch = _debug_gram_blocks(r, blocks)
            assert ch == chunk
            again, _ = _debug_gram_blocks(r, blocks)
            for bi, (B, G) in enumerate(zip(blocks, Gs)):
                tag = (d, r, li, bi, B.shape[1])
                assert np.array_equal(G, again[bi]), tag
                if B.shape[1] == 0:
                    assert np.array_equal(G, np.zeros((r, r))), tag
                    continue
                assert np.array_equal(G, _debug_gram(B)[0]), tag
                worst = max(worst, _check_gram(G, B, tag))
    print("RATIO k_gram_blocks_mfma d=%d chunk %d: %.3f of the (k + 2) eps bound" % (d, chunk, worst))


# ---- (b) ranks against the reference --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_runs(env, tmp_path_factory):
    """every chain case once, shared between (b) and (c)"""
    made = {}

    def get(d, n, R, world, r):
        key = (d, n, R, world, r)
        if key not in made:
            cfg = dict(prw.chain_cfg(d, n, R, r), mode="project")
            made[key] = run_ranks(tmp_path_factory.mktemp("chain"), world, cfg, prw.chain_point(d, r, n))
        return made[key]
    return get


@pytest.mark.parametrize("d,n,R,world", prw.CHAIN_CASES)
@pytest.mark.parametrize("r", prw.CHAIN_RANKS)
def test_chain_jobs_against_the_reference(env, chain_runs, d, n, R, world, r):
    da, _ = env
    res = chain_runs(d, n, R, world, r)
    assert len(res) == world
    X0 = prw.chain_point(d, r, n)
    for k, o in enumerate(res):
        assert np.array_equal(o["X_before"], X0), k
        g, rat, e_h = _check_against_reference(da, o, d, n, 0, 0, True, (d, n, R, world, r, k), lifted=True)
        assert float(o["cost_2f"]) == float(o["eval_after"]), k
    _same_on_every_rank(res)
    print("RATIO project ranks d=%d n=%d R=%d world=%d r=%d: gram %.3f, sigma^2 %.3f, orthogonality %.3f, residual %.3f "
          "of their bounds; |P^T P - host-fed| %.2e (bound 1e-10)" % (d, n, R, world, r, g, rat[0], rat[1], rat[2], e_h))


# ---- (c) hosting does not matter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", prw.CHAIN_RANKS)
def test_chain_job_on_two_and_on_four_ranks(env, chain_runs, r):
    a, b = chain_runs(2, 9, 5, 2, r)[0], chain_runs(2, 9, 5, 4, r)[0]
    for key in FACTS:
        assert np.array_equal(a[key], b[key]), key


def test_rank_counts_and_transports_give_the_same_bits(env, tmp_path):
    """smallGrid3D, 4 agents at rank 5: 2 ranks over IPC, over the staged transport and with the per-agent matrices
    travelling through the segment's sums, and a one-rank exchange in this process"""
    da, orc = env
    ds = common.product_dataset("smallGrid3D")
    X0 = common.random_point(5, ds.d, ds.n, 4, orc.project_to_manifold)
    cfg = dict(kind="pgo", name="smallGrid3D", R=4, r=5, mode="project")
    ipc = run_ranks(tmp_path / "ipc", 2, cfg, X0)
    staged = run_ranks(tmp_path / "staged", 2, cfg, X0, transport="staged")
    sums = run_ranks(tmp_path / "sums", 2, dict(cfg, sums=1), X0)
    s = da.RbcdSession(ds, num_robots=4, r=5)
    ex = da.Exchange(s, "p%s" % uuid.uuid4().hex[:12])
    ex.set_X(X0)
    one = ex.project()
    one["X"] = ex.gather_X()
    assert s.r == ds.d and one["cost_2f"] == ex.evaluate()[0]
    ex.close()
    s.close()
    for res in (ipc, staged, sums):
        _same_on_every_rank(res)
        _check_against_reference(da, res[0], ds.d, ds.n, 0, 0, True, "smallGrid3D")
        for key in ("gram", "basis", "sigma", "positive_dets", "X"):
            assert np.array_equal(res[0][key], one[key]), key
        assert float(res[0]["cost_2f"]) == pytest.approx(one["cost_2f"], rel=1e-12)


def test_one_agent_job_equals_the_single_process_session(env):
    """R = 1: the agent's block is the mirror, so the collective path gives the session's own bits"""
    da, orc = env
    ds = common.product_dataset("smallGrid3D")
    X0 = common.random_point(5, ds.d, ds.n, 4, orc.project_to_manifold)
    a = da.RbcdSession(ds, num_robots=1, r=5)
    a.set_X(X0)
    ref = a.project()
    Xa = a.get_X()
    a.close()
    s = da.RbcdSession(ds, num_robots=1, r=5)
    ex = da.Exchange(s, "p%s" % uuid.uuid4().hex[:12])
    ex.set_X(X0)
    out = ex.project()
    Xb = ex.gather_X()
    ex.close()
    s.close()
    for key in ("gram", "basis", "sigma"):
        assert np.array_equal(out[key], ref[key]), key
    assert out["positive_dets"] == ref["positive_dets"] and out["reflected"] == ref["reflected"]
    assert np.array_equal(Xa, Xb)


# ---- (d) range-aided --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["range_aided_slam_test_2d", "range_aided_slam_test_3d"])
def test_range_aided_job(env, tmp_path, name):
    """two robots on 2 ranks at r = d + 2, from the odometry start after 3 iterations"""
    da, _ = env
    ra = da.RADataset(ra_path(name))
    d, n, l, b, r = ra.d, ra.n, ra.l, ra.b, ra.d + 2
    res = run_ranks(tmp_path, 2, dict(kind="ra", path=ra_path(name), r=r, mode="project", pre=3), _odometry_start(ra, r))
    _same_on_every_rank(res)
    o = res[0]
    X, P = o["X_before"], o["X"]
    assert spi.eig_gap(X, d) >= spi.GAP and spi.block_sigma_min(X, d, n, l, False) >= spi.BLOCK_SIGMA_MIN
    for k, q in enumerate(res):
        g, rat, e_h = _check_against_reference(da, q, d, n, l, b, False, (name, k))
    assert np.abs(np.linalg.norm(P[:, d * n:d * n + l], axis=0) - 1).max() <= 8 * EPS
    ref_c, cb = sri.cost_reference(P, ra.Q.to_scipy(), d)
    assert abs(float(ref_c) - float(o["cost_2f"])) <= float(cb)
    assert float(o["cost_2f"]) == float(o["eval_after"])
    print("RATIO project ranks %s: gram %.3f, sigma^2 %.3f of their bounds; |P^T P - host-fed| %.2e; 2f %.9g" %
          (name, g, rat[0], e_h, float(o["cost_2f"])))


# ---- (e) the reflect decision across ranks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", spi.DIMS)
def test_reflect_decision_across_ranks(env, tmp_path, d):
    """see the module's docstring: the family's poses on a pose-graph chain, agent 0 (poses 0-3) on rank 0 and agent 1
    (poses 4-8) on rank 1, so that the count is a sum over the ranks"""
    n, r = spi.REFLECT_DIMS["n"], spi.REFLECT_DIMS["r"]
    ms = spi.REFLECT_KEEP + spi.REFLECT_FLIP
    cases = [prw.reflect_chain_case(d, m) for m in ms]
    cfg = dict(kind="chain", d=d, n=n, R=2, r=r, seed=sri.seed_of(d, r, n), mode="reflect")
    res = run_ranks(tmp_path, 2, cfg, np.concatenate([X for _, X in cases], axis=0))
    for i, (m, (Xd, _)) in enumerate(zip(ms, cases)):
        keys = ["%s_%d" % (key, i) for key in FACTS]
        _same_on_every_rank(res, keys)
        o = res[0]
        npos, reflected, P = int(o["positive_dets_%d" % i]), bool(o["reflected_%d" % i]), o["X_%d" % i]
        assert bool(o["projected_%d" % i]) and P.shape == (d, (d + 1) * n)
        assert npos in (m, n - m), (m, npos)
        assert reflected == (npos < n // 2), (m, npos)
        kept, flipped = (spi.project_blocks(Xd, d, n, 0, True, f) for f in (False, True))
        want = m > n - m
        G = P.T @ P
        dist = {False: np.abs(G - kept.T @ kept).max(), True: np.abs(G - flipped.T @ flipped).max()}
        print("reflect ranks d=%d m=%d: npos %d reflected %d; |G - G_kept| %.2e  |G - G_reflected| %.2e" %
              (d, m, npos, reflected, dist[False], dist[True]))
        assert dist[want] <= 1e-10, (m, dist)
        assert dist[not want] > 1e-3, (m, dist)
        assert (np.linalg.det(spi.rotation_blocks(P, d, n, 0, True)) > 1 - 64 * EPS).all()


# ---- (f) r == d, (i) a refused call ------------------------------------------------------------------------------------------
def test_rank_d_job_is_passed_through(env, tmp_path):
    """the reference passes X through at r == d: the job is untouched and its next iterations are its twin's, which
    never called (and which was first handed a call without a handle: DCORA_ERR_BAD_ARG)"""
    da, orc = env
    ds = common.product_dataset("smallGrid3D")
    d = ds.d
    X0 = common.random_point(d, d, ds.n, 4, orc.project_to_manifold)
    cfg = dict(kind="pgo", name="smallGrid3D", R=4, r=d, mode="project", pre=3, greedy=5)
    A = run_ranks(tmp_path / "called", 2, cfg, X0)
    B = run_ranks(tmp_path / "twin", 2, dict(cfg, project=False), X0)
    N = run_ranks(tmp_path / "refused", 2, dict(cfg, project=False, null_call=1), X0)
    _same_on_every_rank(A, ("gram", "sigma", "cost_2f", "gradnorm", "X"))
    for k in range(2):
        a, b, c = A[k], B[k], N[k]
        assert not bool(a["projected"]) and a["basis"].size == 0 and int(a["r"]) == d
        assert np.array_equal(a["X"], a["X_before"])
        assert float(a["cost_2f"]) == float(a["eval_after"])
        _check_gram(a["gram"], a["X"], k)
        _check_spectrum(_as_out(a), a["X"], d, k)
        assert int(c["null_status"]) == BAD_ARG
        for o in (a, c):
            assert np.array_equal(o["X"], b["X"])
            for key in ("g_selected", "g_cost", "g_gradnorm", "X_greedy"):
                assert np.array_equal(o[key], b[key]), (k, key)
            assert b["g_cost"].size == 5
            assert int(o["launches"]) == int(b["launches"]), k
        print("launches of the twin, rank %d: job %d, its 5 iterations %d" % (k, int(b["launches_job"]), int(b["launches"])))
        # a job that never projects launches what the parent commit's build launches
        assert int(b["launches_job"]) == PARENT_LAUNCHES[k], (k, int(b["launches_job"]))


# ---- (g) the projected job is a fresh job -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["smallGrid3D", "range_aided_slam_test_2d"])
def test_projected_job_runs_as_a_fresh_one(env, tmp_path, name):
    """after 7 iterations the job projects; then 35 greedy iterations (across the restart at 30) and 3 coloured sweeps
    with acceleration off, against a fresh job created at rank d and handed the gathered projected X"""
    da, orc = env
    if name.startswith("range_aided"):
        ra = da.RADataset(ra_path(name))
        d, r = ra.d, ra.d + 2
        base = dict(kind="ra", path=ra_path(name))
        X0 = _odometry_start(ra, r)
    else:
        ds = common.product_dataset(name)
        d, r = ds.d, 5
        base = dict(kind="pgo", name=name, R=4)
        X0 = common.random_point(r, d, ds.n, 4, orc.project_to_manifold)
    A = run_ranks(tmp_path / "projected", 2, dict(base, r=r, mode="project", pre=7, greedy=35, sweeps=3), X0)
    Xp = A[0]["X"]
    assert Xp.shape[0] == d and bool(A[0]["projected"])
    B = run_ranks(tmp_path / "fresh", 2, dict(base, r=d, mode="project", project=False, evaluate=1, greedy=35, sweeps=3), Xp)
    for k in range(2):
        a, b = A[k], B[k]
        assert np.array_equal(a["X"], b["X"]), k
        assert float(a["cost_2f"]) == float(b["eval_after"]), k
        for key in ("g_selected", "g_cost", "g_gradnorm"):
            assert a[key].size == 35 and np.array_equal(a[key], b[key]), (k, key)
        for key in ("c_cost", "c_gradnorm"):
            assert a[key].size == 3 and np.array_equal(a[key], b[key]), (k, key)
        assert np.array_equal(a["X_greedy"], b["X_greedy"]) and np.array_equal(a["X_sweeps"], b["X_sweeps"]), k
        assert int(a["launches"]) == int(b["launches"]), k


# ---- (h) state survives -----------------------------------------------------------------------------------------------------
def _robust_job_keeps_its_state(tmp_path, cfg, X0, d, mu_step, files=None):
    A = run_ranks(tmp_path / "projected", 2, cfg, X0, files=files)
    _same_on_every_rank(A, ("gram", "basis", "sigma", "X", "w_after", "w_next", "v"))
    a = A[0]
    w, Xp = a["w_before"], a["X"]
    zeros = bool(np.any(w == 0.0))
    extra = dict(files or {}, **{"w.npy": w})
    fresh_cfg = dict(cfg, r=d, fresh=True)
    if zeros:
        extra["X_run.npy"] = a["X_run"]
        fresh_cfg["X_sync"] = "X_run.npy"
    B = run_ranks(tmp_path / "fresh", 2, fresh_cfg, Xp, files=extra)
    for k in range(2):
        a, b = A[k], B[k]
        assert bool(a["projected"]) and int(a["r"]) == d
        assert np.array_equal(a["w_after"], w) and list(a["updates"]) == [2, 2] and a["mu"][0] == a["mu"][1]
        assert list(a["team"][0][:2]) == list(a["team"][1][:2]) and int(a["team"][1][2]) == 0
        assert bool(a["params_kept"]) and bool(a["lcs_kept"]) and bool(a["statuses_cleared"])
        assert np.array_equal(a["lcs"], b["lcs"]) and np.array_equal(b["w_before"], w)
        assert a["mu"][1] == b["mu"][1] and list(b["updates"]) == [2, 2]
        assert np.array_equal(a["g_selected"], b["g_selected"]), k
        if zeros:  # explicit zeros on the live job's patterns: tests/test_session_project_gpu.py's bounds
            assert np.allclose(a["g_cost"], b["g_cost"], rtol=1e-9, atol=0)
            assert common.rel(a["X_run"], b["X_run"]) < 1e-7
        else:
            assert np.array_equal(a["g_cost"], b["g_cost"]) and np.array_equal(a["X_run"], b["X_run"])
        assert int(a["updates_next"]) == 3 and float(a["mu_next"]) == pytest.approx(float(a["mu"][0]) * mu_step, rel=1e-12)
        assert np.array_equal(a["w_next"], b["w_next"]) and list(a["counts"]) == list(b["counts"])
        # the certificate of the matrices the ranks hold, then a lift from rank d
        assert bool(a["cert"]) == bool(b["cert"]) and float(a["theta"]) == float(b["theta"])
        assert np.array_equal(a["v"], b["v"])
        if not bool(a["cert"]):
            assert int(a["r_lifted"]) == d + int(bool(a["lift_escaped"]))


def test_robust_pose_graph_job_keeps_its_state(env, tmp_path):
    da, _ = env
    R, r = 5, 5
    clean = common.product_dataset("smallGrid3D")
    ds = _with_outliers(da.Dataset, clean, 12, seed=2)
    X0 = np.zeros((r, 4 * ds.n))
    X0[:3] = da.chordal_initialization(clean)
    files = {"ids.npy": ds.ids, "vals.npy": ds.vals}
    cfg = dict(kind="pgo", name="smallGrid3D", R=R, r=r, d=ds.d, n=ds.n, mode="robust", gnc=GNC, team_iters=20, eta=ETA,
               tol=dict(gradient_tolerance=1e-6, preconditioned_gradient_tolerance=1e-6))
    _robust_job_keeps_its_state(tmp_path, cfg, X0, ds.d, GNC["GNCMuStep"], files)


def test_robust_range_aided_job_keeps_its_state(env, tmp_path):
    """the loop-closure variant of tiers the range-aided GNC tests use (ra_loops.GNC_FIXTURE), rank 4 -> 2"""
    da, _ = env
    path = ra_loops.write_loops_variant(tmp_path, **ra_loops.GNC_FIXTURE)[0]
    ra = da.RADataset(path)
    r = ra.d + 2
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    cfg = dict(kind="ra", path=path, r=r, mode="robust", gnc=ra_loops.GNC_PARAMS, team_iters=20, eta=ETA,
               restart_interval=5, tol=dict(gradient_tolerance=1e-4, preconditioned_gradient_tolerance=1e-4))
    _robust_job_keeps_its_state(tmp_path / "job", cfg, X0, ra.d, ra_loops.GNC_PARAMS["GNCMuStep"])


# ---- (j) drivers ------------------------------------------------------------------------------------------------------------
def _driver_results(tmp_path, base, X0, kw):
    """the plain rank driver against its _projected sibling (projection, refinement and rounding on the device)"""
    plain = run_ranks(tmp_path / "plain", 2, dict(base, mode="staircase", kw=kw), X0)
    res = run_ranks(tmp_path / "device", 2, dict(base, mode="staircase", projected=True, kw=kw), X0)
    for pair in (plain, res):
        for key in pair[0].files:
            assert np.array_equal(pair[0][key], pair[1][key]), key  # identical on both ranks
    p, q = plain[0], res[0]
    assert set(p["keys"]) == PARENT_KEYS
    assert set(q["keys"]) >= PARENT_KEYS | EXTRA_KEYS and set(q["keys"]) <= PARENT_KEYS | EXTRA_KEYS | ROUND_KEYS
    as_dict = lambda o: dict({key: (o[key] if o[key].ndim else o[key].item()) for key in o.files},
                             suboptimality_gap_f=(o["suboptimality_gap_f"].item() if "suboptimality_gap_f" in o.files
                                                  else None),
                             levels=[dict(cost_2f=c) for c in o["level_costs"]])
    return as_dict(p), as_dict(q)


def test_pose_graph_driver_projects_across_two_ranks(env, tmp_path):
    da, orc = env
    ds = common.product_dataset("smallGrid3D")
    d, n = ds.d, ds.n
    X0 = common.random_point(3, d, n, 4, orc.project_to_manifold)
    kw = dict(num_robots=5, r_min=3, r_max=9, max_iters=400, rgrad_tol=0.05)
    plain, res = _driver_results(tmp_path, dict(kind="pgo", name="smallGrid3D", R=5, r=3), X0, kw)
    X = res["X"]
    H = sri.se_from_ra(da.project_solution_raslam(spi.ra_from_se(X, d, n), X.shape[0], d, n, 0, 0), d, n, 0)
    _driver_checks(plain, res, da.build_Q_pgo(ds).to_scipy(), H, d, 1e-3, "smallGrid3D on 2 ranks")
    assert res["trajectory"].shape == (d, (d + 1) * n)


def test_raslam_driver_projects_across_two_ranks(env, tmp_path):
    da, orc = env
    name = "range_aided_slam_test_3d"
    ra = da.RADataset(ra_path(name))
    d = ra.d
    rng = np.random.default_rng(12)
    X0 = orc.project_to_manifold(d, d, ra.n, rng.standard_normal((d, ra.k)), l=ra.l, b=ra.b)
    kw = dict(max_iters=300, rgrad_tol=1e-3, r_max=d + 5)
    plain, res = _driver_results(tmp_path, dict(kind="ra", path=ra_path(name), r=d), X0, kw)
    X = res["X"]
    H = da.project_solution_raslam(X, X.shape[0], d, ra.n, ra.l, ra.b)
    _driver_checks(plain, res, ra.Q.to_scipy(), H, d, 1e-3, name + " on 2 ranks")
    assert res["trajectory"].shape == (d, (d + 1) * ra.n)
