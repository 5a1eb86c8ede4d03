"""Robust weights updated across the ranks of a range-aided RBCD job (dcora_ra_rbcd_create_robust_ranks,
dcora_exchange_update_weights / _set_weights / _get_weights on its exchange; Agent::updateMeasurementWeights of every
agent of a RangeAidedSLAMGraph on every rank, ref src/Agent.cpp:1332-1441): several processes (one per rank, all on
device 0) must reproduce the one-process robust session -- weights, counts, selected agents and X bit for bit, costs to
the rounding the plain range-aided exchange test allows (the evaluation sums per agent) -- and reject the injected
outliers.  A rank's view holds the pose-pose measurements touching its agents; refusals are the same on every rank and
leave the job as it was.

The parameters of the comparison cases were chosen on the one-process session so that some update rejects a closure
and some update leaves a fractional weight (asserted on the reference run of every case):
  range_aided_slam_test_3d  its four closures are consistent (residuals 0.011 .. 0.029 after four iterations from the
                            start used here), so the cost is made tight around them: GNCBarc 0.014 with mu starting
                            at 1 rejects above 0.0198 and accepts below 0.0099 at the first update
  the GNC fixture           GNCBarc 10 as everywhere, GNCMuStep 8: the six outliers are rejected at the fourth update,
                            every closure is fractional after the first
  the sparse variant        two updates only, so mu starts at 0.05 (GNCMuStep 4): outliers above sqrt(21) GNCBarc go
                            at the first update"""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import common
import ra_loops
from test_raslam import ra_path

pytestmark = pytest.mark.gpu

WORKER = os.path.join(common.HERE, "ra_gnc_ranks_worker.py")
P_SPARSE = 673  # every agent of the variant takes the sparse partitioned inverse (tests/test_ra_gnc_session_gpu.py)
K_DENSE_MAX = 2200
TIGHT = dict(GNCBarc=0.014, GNCInitMu=1.0, GNCMuStep=2.0)
STEP8 = dict(GNCBarc=10.0, GNCMuStep=8.0)
FROM_005 = dict(GNCBarc=10.0, GNCInitMu=0.05, GNCMuStep=4.0)


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    if dcora_amd.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return dcora_amd


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    """name -> (path, info): the loop-closure variants of tiers the tests share, written once"""
    d = tmp_path_factory.mktemp("ra_loops")
    return {"gnc": ra_loops.write_loops_variant(d, **ra_loops.GNC_FIXTURE),
            "sparse": ra_loops.write_loops_variant(d, P=P_SPARSE, seed=3, per_pair=3, intra=2, outliers=4)}


def _path(variants, name):
    return variants[name][0] if name in variants else ra_path(name)


def _start(da, ra, r, seed=5):
    if ra.n > 100:  # the variants: the CORA driver's odometry start lifted to rank r
        X0 = np.zeros((r, ra.k))
        X0[:ra.d] = ra.X_odom
        return X0
    rng = np.random.default_rng(seed)
    lift = np.linalg.qr(rng.standard_normal((r, ra.d)))[0]
    return da.manifold_project(r, ra.d, ra.n, lift @ ra.gt + 0.05 * rng.standard_normal((r, ra.k)), l=ra.l, b=ra.b)


def run_ranks(tmp_path, world, path, X0, cfg, transport=None, w_file=None, fixed=None, X1=None):
    d = str(tmp_path)
    np.save(os.path.join(d, "X0.npy"), X0)
    for name, a in (("w_file", w_file), ("fixed", fixed), ("X1", X1)):
        if a is not None:
            np.save(os.path.join(d, name + ".npy"), a)
    cfg = dict(cfg, path=str(path), w_file=w_file is not None, fixed=fixed is not None)
    with open(os.path.join(d, "job.json"), "w") as f:
        json.dump(cfg, f)
    job = "rg%s" % uuid.uuid4().hex[:12]
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


def single_gnc(da, path, X0, r, params, rounds, inner, final):
    """the worker's calls on a one-process robust session, recording what every update gives"""
    ra = da.RADataset(path)
    s = da.RaRbcdSession(ra, r, robust=params)
    s.set_X(X0)
    runs, counts, W, info = [], [], [], []
    W0 = s.get_weights()
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
    return dict(counts=np.array(counts), W0=W0, W=np.array(W), info=np.array(info), cost=cat("cost"),
                gradnorm=cat("gradnorm"), selected=cat("selected"), X=X)


def touching_mask(ra, world, rank):
    """the pose-pose measurements touching an agent of `rank`, from the ownership of the poses alone: agents are the
    robots with poses in id order, consecutive agents share a rank"""
    robots = sorted(set(ra.pose_robot.tolist()))
    agent = np.searchsorted(robots, ra.pose_robot)
    per_rank = (len(robots) + world - 1) // world
    ids, _ = ra.pose_pose()
    return np.any(agent[ids[:, :2]] // per_rank == rank, axis=1)


def inter_robot(ra):
    ids, _ = ra.pose_pose()
    return ra.pose_robot[ids[:, 0]] != ra.pose_robot[ids[:, 1]]


CASES = [
    # fixture, r, ranks, robust parameters, rounds, inner, final, transport
    ("range_aided_slam_test_3d", 4, 2, TIGHT, 3, 4, 4, None),  # one robot per rank: every inter-robot closure is shared
    ("gnc", 3, 2, STEP8, 4, 8, 8, None),                       # four robots, two per rank, dense inverses
    ("gnc", 3, 4, STEP8, 4, 8, 8, None),                       # one robot per rank
    ("gnc", 3, 2, STEP8, 4, 8, 8, "staged"),                   # the shared-host-segment transport
    ("sparse", 3, 2, FROM_005, 2, 4, 4, None),                 # sparse partitioned inverses rebuilt through the cache; the hub
]


@pytest.mark.parametrize("name,r,world,gnc,rounds,inner,final,transport", CASES)
def test_ranks_reproduce_the_one_process_robust_session(da, variants, tmp_path, name, r, world, gnc, rounds, inner, final,
                                                        transport):
    from dcora_amd import robust as rb
    path = _path(variants, name)
    ra = da.RADataset(path)
    ks = [len(ra.agent_columns[q][1]) for q in ra.robots]
    assert (min(ks) > K_DENSE_MAX) if name == "sparse" else (max(ks) <= K_DENSE_MAX), ks
    X0 = _start(da, ra, r)
    params = rb.RobustCostParameters("GNC_TLS", **gnc)
    ref = single_gnc(da, path, X0, r, params, rounds, inner, final)
    lc = ra.loop_closures()
    frac = [(w[lc] >= 1e-8) & (w[lc] <= 1 - 1e-8) for w in ref["W"]]
    print("counts per update (accepted, rejected, undecided):", ref["counts"].tolist())
    assert ref["counts"][:, 1].max() > 0, "no update rejected a closure: the case shows too little"
    assert max(int(f.sum()) for f in frac) > 0, "no update left a fractional weight: the case shows too little"
    # two fresh one-process runs agree with each other: otherwise the comparison below is not well posed
    again = single_gnc(da, path, X0, r, params, rounds, inner, final)
    for key in ref:
        assert np.array_equal(ref[key], again[key]), key
    res = run_ranks(tmp_path, world, path, X0, dict(mode="compare", r=r, cost="GNC_TLS", robust=gnc, rounds=rounds,
                                                    inner=inner, final=final), transport=transport)
    w_start = np.ones(ra.num_pose_pose)
    assert np.array_equal(ref["W0"], w_start)
    for k, o in enumerate(res):
        assert int(o["mode"]) == (2 if transport == "staged" else 1)
        assert np.array_equal(o["counts"], ref["counts"]), (k, o["counts"], ref["counts"])
        assert np.array_equal(o["W0"], w_start)
        for u in range(rounds):
            assert np.array_equal(o["W"][u], ref["W"][u]), (k, u, np.abs(o["W"][u] - ref["W"][u]).max())
        assert np.array_equal(o["info"], ref["info"])
        assert np.array_equal(o["selected"], ref["selected"]), (k, o["selected"], ref["selected"])
        assert np.array_equal(o["X"], ref["X"]), (k, np.abs(o["X"] - ref["X"]).max())
        assert np.allclose(o["cost"], ref["cost"], rtol=1e-9, atol=1e-12), (k, np.abs(o["cost"] / ref["cost"] - 1).max())
        assert np.allclose(o["gradnorm"], ref["gradnorm"], rtol=1e-6, atol=1e-9)
        # this rank's view: every pose-pose measurement touching one of its agents, NaN elsewhere, the job's bits where set
        mine = touching_mask(ra, world, k)
        for u, loc in enumerate([o["local0"]] + list(o["local"])):
            assert np.array_equal(~np.isnan(loc), mine), (k, u)
            assert np.array_equal(loc[mine], ([o["W0"]] + list(o["W"]))[u][mine]), (k, u)
        if name == "gnc" and world == 2:
            assert (~mine).any(), "every measurement touches rank %d: the view shows nothing" % k
    if len(ra.robots) == world:  # one robot per rank: every inter-robot closure is weighted by both of its ranks
        inter = inter_robot(ra)
        assert inter.any() and np.all(sum(touching_mask(ra, world, k).astype(int) for k in range(world))[inter] == 2)


def test_a_shared_closure_is_weighted_alike_on_both_ranks(da, tmp_path):
    """the GM cost gives every closure a weight strictly inside (0, 1): both ranks of the two-robot fixture compute the
    weight of every inter-robot closure, from mirror columns that are equal bit for bit"""
    r = 4
    path = ra_path("range_aided_slam_test_3d")
    ra = da.RADataset(path)
    inter = inter_robot(ra)
    assert inter.any() and np.all(ra.loop_closures()[inter])
    res = run_ranks(tmp_path, 2, path, _start(da, ra, r), dict(mode="compare", r=r, cost="GM", robust={}, rounds=1,
                                                               inner=4, final=2))
    a, b = res[0]["local"][0], res[1]["local"][0]
    assert np.all((a[inter] > 0) & (a[inter] < 1)), a[inter]
    assert np.array_equal(a[inter], b[inter]) and np.array_equal(a[inter], res[0]["W"][0][inter])
    assert np.array_equal(res[0]["W"][0], res[1]["W"][0])


def test_reset_and_refusals_are_collective(da, tmp_path):
    from dcora_amd import robust as rb
    r, world = 4, 2
    path = ra_path("range_aided_slam_test_3d")
    ra = da.RADataset(path)
    m = ra.num_pose_pose
    lc = ra.loop_closures()
    zero_edge = int(np.nonzero(lc)[0][0])
    fixed = np.zeros(m, bool)
    fixed[zero_edge] = True
    w_file = np.ones(m)
    w_file[zero_edge] = 0.0  # a fixed weight 0: not in the sessions' patterns
    ra.set_pose_pose_weights(w_file)
    X0, X1 = _start(da, ra, r, 3), _start(da, ra, r, 4)
    res = run_ranks(tmp_path, world, path, X0, dict(mode="refusals", r=r, cost="GNC_TLS", robust=TIGHT, edge=2,
                                                    zero_edge=zero_edge), w_file=w_file, fixed=fixed, X1=X1)
    # the one-process reference of what the job did around its refusals
    s = da.RaRbcdSession(ra, r, robust=rb.RobustCostParameters("GNC_TLS", **TIGHT), fixed_weight=fixed)
    s.set_X(X0)
    runs = [s.run(max_iters=5, rgrad_tol=0.0), s.run(max_iters=6, rgrad_tol=0.0)]
    c = s.update_weights()
    W = s.get_weights()
    runs.append(s.run(max_iters=5, rgrad_tol=0.0))
    X_after = s.get_X()
    s.close()
    assert W[zero_edge] == 0.0
    for k, o in enumerate(res):
        # NaN, negative, inf, the zero edge made nonzero: BAD_ARG; the session-level calls and the team: UNSUPPORTED
        assert list(o["status"]) == [1, 1, 1, 1, 8, 8, 8], (k, o["status"])
        assert bool(o["names_the_collective"])
        assert bool(o["unchanged"])
        assert np.array_equal(o["W0"], w_file)
        assert list(o["counts"][0]) == [c["accepted"], c["rejected"], c["undecided"]]
        assert np.array_equal(o["W"][0], W)
        assert np.array_equal(o["selected"], np.concatenate([q["selected"] for q in runs]))
        assert np.array_equal(o["X_after"], X_after), k
        assert np.array_equal(o["X_reset"], X1), k
        assert int(o["updates"]) == 2


def test_one_rank_through_the_new_creator_is_the_robust_session(da, variants):
    """world_size 1 through dcora_ra_rbcd_create_robust_ranks: bitwise the session of dcora_ra_rbcd_create_robust over a
    short GNC run (no subprocess); the session-level weight changes are refused, the view and robust_info are the
    session's"""
    from dcora_amd import capi, driver
    from dcora_amd import robust as rb
    r = 3
    path = variants["gnc"][0]
    ra = da.RADataset(path)
    X0 = _start(da, ra, r)
    params = rb.RobustCostParameters("GNC_TLS", **STEP8)
    A = da.RaRbcdSession(ra, r, robust=params)
    B, ex = da.ra_robust_ranked_session(ra, "w1%s" % uuid.uuid4().hex[:10], r, robust=params)
    try:
        A.set_X(X0)
        ex.set_X(X0)
        assert np.array_equal(A.get_weights(), ex.get_weights())
        for _ in range(4):
            a, b = A.run(max_iters=8, rgrad_tol=0.0), B.run(max_iters=8, rgrad_tol=0.0)
            for key in ("cost", "gradnorm", "selected"):
                assert np.array_equal(a[key], b[key]), key
            assert A.update_weights() == ex.update_weights()
            wa = A.get_weights()
            assert np.array_equal(wa, ex.get_weights()) and np.array_equal(wa, B.get_weights())
            assert A.robust_info() == B.robust_info()
            assert np.array_equal(A.get_X(), ex.gather_X())
        assert np.any(wa < 1e-8)
        for call in (lambda: B.update_weights(), lambda: B.set_weights(wa)):
            with pytest.raises(capi.DcoraError) as e:
                call()
            assert e.value.status == 8 and "dcora_exchange_" in str(e.value)
        with pytest.raises(capi.DcoraError) as e:  # the team protocol stays refused on a range-aided exchange
            ex.enable_team()
        assert e.value.status == 8
        ex.set_weights(wa * 0.5)
        A.set_weights(wa * 0.5)
        assert np.array_equal(ex.get_weights(), A.get_weights()) and np.array_equal(B.get_weights(), wa * 0.5)
        a, b = A.run(max_iters=6, rgrad_tol=0.0), B.run(max_iters=6, rgrad_tol=0.0)
        assert np.array_equal(a["cost"], b["cost"]) and np.array_equal(A.get_X(), B.get_X())
    finally:
        ex.close()
        B.close()
        A.close()
    # the SPMD driver at one rank against the one-session flow: the same weights and X, costs to rounding
    kw = dict(robust=params, num_weight_updates=4, inner_iters=8, rgrad_tol=0.0, max_final_iters=8)
    one = driver.gnc_ra_session(da.RADataset(path), X0, r, **kw)
    ra2 = da.RADataset(path)
    ranks = driver.gnc_ra_ranks(ra2, X0, r, job_name="d1%s" % uuid.uuid4().hex[:10], **kw)
    assert np.array_equal(one["weights"], ranks["weights"]) and np.array_equal(one["X"], ranks["X"])
    assert np.array_equal(ra2.pose_pose_weights, ranks["weights"])
    assert [q["rejected"] for q in one["rounds"]] == [q["rejected"] for q in ranks["rounds"]]
    assert ranks["final"]["cost_2f"] == pytest.approx(one["final"]["cost_2f"], rel=1e-9, abs=1e-12)


def test_gnc_across_ranks_rejects_the_injected_outliers(da, variants, tmp_path):
    r, world = 3, 2
    path, info = variants["gnc"]
    ra = da.RADataset(path)
    inl, outl = ra_loops.closure_masks(info)
    res = run_ranks(tmp_path, world, path, _start(da, ra, r),
                    dict(mode="driver", r=r, cost="GNC_TLS", robust=ra_loops.GNC_PARAMS, rounds=12, inner=30, final=100,
                         rgrad_tol=0.1))
    for o in res:
        w = o["weights"]
        assert np.array_equal(o["loop_closures"], inl | outl)
        assert np.array_equal(o["ra_weights"], w)
        assert np.all(w[outl] < 1e-8), "every injected outlier is rejected"
        assert np.all(w[inl] >= 1e-8), "no ground-truth closure is rejected"
        assert np.all(w[~(inl | outl)] == 1.0)
        assert np.array_equal(w, res[0]["weights"])
        assert np.array_equal(o["X"], res[0]["X"]) and float(o["cost"]) == float(res[0]["cost"])


def test_plain_robust_session_still_refuses_ranks(da):
    from dcora_amd import capi
    from dcora_amd import robust as rb
    ra = da.RADataset(ra_path("range_aided_slam_test_3d"))
    with pytest.raises(capi.DcoraError) as e:
        da.RaRbcdSession(ra, 4, robust=rb.RobustCostParameters("GNC_TLS"), world_size=2)
    assert e.value.status == 8 and "dcora_ra_rbcd_create_robust_ranks" in str(e.value)
