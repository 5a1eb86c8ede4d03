"""The team protocol across the ranks of a range-aided job (dcora_exchange_team_enable_ra, then _agent_status,
_loop_closure_stats, _should_terminate, _should_update_weights, _team_info, _run_team on an exchange of
dcora_exchange_create_ra or dcora_ra_rbcd_create_robust_ranks; the reference's agents run Agent::iterate's status block,
shouldTerminate and shouldUpdateMeasurementWeights on a RangeAidedSLAMGraph as on a pose graph, ref src/Agent.cpp:558-586,
1123-1156, 1280-1330, 1417-1424): several processes (one per rank, all on device 0) must hold, on every rank, the
statuses and decisions of the one-process RaRbcdSession that called dcora_ra_rbcd_team_enable -- integers, statuses (the
relative change included), weights and X bit for bit, costs and gradient norms to the rounding
tests/test_ra_gnc_ranks_gpu.py grants (the ranks sum the evaluation per agent).  Modelled on tests/test_team_ranks_gpu.py.

The parameters were chosen on the one-process session (its figures are asserted on the reference run of every case):
  the L2 team          default parameters; agent 0 is ready to terminate in rounds 20 and 30 of 30, no round asks for an
                       update
  the robust run loop  GNCBarc 10, GNCMuStep 8, four updates after at most 10 rounds each, one reset: updates in rounds
                       10, 20, 30, 40, the six outliers rejected, all_ready after 57 rounds
  the sparse variant   mu from 0.05 (GNCMuStep 4), two updates after 4 rounds each: stopped by its cap of 12 rounds with
                       four closures rejected"""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import common
import ra_loops
import team_ranks_worker as tw
from ra_ring import write_ring_variant
from test_ra_team_cpu import stats_numpy
from test_raslam import ra_path

pytestmark = pytest.mark.gpu

WORKER = os.path.join(common.HERE, "ra_team_ranks_worker.py")
P_SPARSE = 673  # every agent of the variant takes the sparse partitioned inverse (tests/test_ra_gnc_ranks_gpu.py)
K_DENSE_MAX = 2200
STEP8 = dict(GNCBarc=10.0, GNCMuStep=8.0)  # as tests/test_ra_gnc_ranks_gpu.py
FROM_005 = dict(GNCBarc=10.0, GNCInitMu=0.05, GNCMuStep=4.0)
TEAM = dict(max_num_iters=120, robust_opt_num_weight_updates=4, robust_opt_inner_iters=10, robust_opt_num_resets=1)
# at most 16 squares summed in index order and one square root: about 18 roundings of 2^-53 (2e-15), FMA or not
# (the bound of tests/test_ra_team_status_gpu.py: the reduction is the same code)
RTOL_KERNEL = 1e-14
R_GNC = 3  # relaxation rank of the cases on the tiers variants


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    if dcora_amd.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return dcora_amd


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    """the run-time variants of tiers the tests share, written once: gnc, sparse -> (path, info), ring -> path"""
    d = tmp_path_factory.mktemp("ra_team_ranks")
    return {"gnc": ra_loops.write_loops_variant(d, **ra_loops.GNC_FIXTURE),
            "sparse": ra_loops.write_loops_variant(d, P=P_SPARSE, seed=3, per_pair=3, intra=2, outliers=4),
            "ring": write_ring_variant(d)[0]}


def _odom_start(ra, r):
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    return X0


def _lifted_start(da, ra, r, seed=5):  # as tests/test_ra_gnc_ranks_gpu.py
    rng = np.random.default_rng(seed)
    lift = np.linalg.qr(rng.standard_normal((r, ra.d)))[0]
    return da.manifold_project(r, ra.d, ra.n, lift @ ra.gt + 0.05 * rng.standard_normal((r, ra.k)), l=ra.l, b=ra.b)


def run_ranks(tmp_path, world, path, X0, cfg, transport=None):
    d = str(tmp_path)
    np.save(os.path.join(d, "X0.npy"), X0)
    with open(os.path.join(d, "job.json"), "w") as f:
        json.dump(dict(cfg, path=str(path)), f)
    job = "rt%s" % uuid.uuid4().hex[:12]
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
    res = [np.load(os.path.join(d, "rank%d.npz" % k)) for k in range(world)]
    for o in res:
        if "transport" in o:
            assert int(o["transport"]) == (2 if transport == "staged" else 1)
    return res


EXACT_VIEW = ("status", "decide", "info", "lc")


def _same_run(o, ref, k, keys):
    for key in keys:
        assert np.array_equal(o[key], ref[key]), (k, key, o[key], ref[key])
    assert np.allclose(o["cost"], ref["cost"], rtol=1e-9, atol=1e-12), (k, np.max(np.abs(o["cost"] / ref["cost"] - 1)))
    assert np.allclose(o["gradnorm"], ref["gradnorm"], rtol=1e-6, atol=1e-9), k


def _single_greedy(da, path, X0, r, rounds, enable=True, gather=False, **session):
    """tw.greedy_rounds on the one-process session; gather: X after every round as well"""
    s = da.RaRbcdSession(da.RADataset(path), r, **session)
    if enable:
        s.enable_team()
    s.set_X(X0)
    if gather:
        recs = []
        for _ in range(rounds):
            sel = recs[-1]["next"] if recs else 0
            rec = _one_round(s, sel)
            recs.append(rec)
        ref = {k: np.array([q[k] for q in recs]) for k in recs[0]}
    else:
        ref = tw.greedy_rounds(s, s if enable else None, s.R, rounds)
    ref["X"] = s.get_X()
    s.close()
    return ref


def _one_round(s, sel):
    c2, g, _, nxt = s.iterate(sel)
    v = tw.team_view(s, s.R)
    return dict(v, cost=c2, gradnorm=g, selected=sel, next=nxt, Xs=s.get_X())


# ---- 1. an L2 team on greedy iterations -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def l2_reference(da, variants):
    path = variants["gnc"][0]
    X0 = _odom_start(da.RADataset(path), R_GNC)
    return path, X0, _single_greedy(da, path, X0, R_GNC, 30)


@pytest.mark.parametrize("world", [2, 4, 3])  # 3 ranks: ceil(4 / 3) = 2 agents per rank, the last rank hosts none
def test_l2_team_holds_the_one_process_statuses_on_every_rank(da, tmp_path, l2_reference, world):
    path, X0, ref = l2_reference
    assert ref["status"].shape == (30, 4, 7)
    assert ref["status"][:, :, 5].any(), "no status is ever ready to terminate: the case shows too little"
    assert not ref["decide"][:, 1].any()  # the L2 rules never ask for an update
    res = run_ranks(tmp_path, world, path, X0, dict(mode="greedy", r=R_GNC, rounds=30))
    if world == 3:
        assert res[2]["hosted"].size == 0
    for k, o in enumerate(res):
        _same_run(o, ref, k, EXACT_VIEW + ("selected", "X"))


# ---- 2. where the ranked kernel reads and where it stores -----------------------------------------------------------
def test_the_ranked_kernel_takes_the_agents_pose_translations_into_its_slot(da, tmp_path):
    r, rounds = 4, 8
    path = ra_path("range_aided_slam_test_3d")
    ra = da.RADataset(path)
    assert ra.d == 3 and ra.l > 0 and ra.b > 0 and len(ra.robots) == 2  # toff = d n_a + l_a matters; one robot per rank
    X0 = _lifted_start(da, ra, r)
    ref = _single_greedy(da, path, X0, r, rounds, gather=True)
    res = run_ranks(tmp_path, 2, path, X0, dict(mode="greedy", r=r, rounds=rounds, gather=True))
    assert set(ref["selected"].tolist()) == {0, 1}, "both agents optimise, the second rank's one too"
    for k, o in enumerate(res):
        assert np.array_equal(o["selected"], ref["selected"])
        before = X0
        for t in range(rounds):
            q = int(o["selected"][t])
            after = o["Xs"][t]
            cols = ra.d * ra.n + ra.l + np.flatnonzero(ra.pose_robot == ra.robots[q])  # the agent's pose translations
            D = after[:, cols] - before[:, cols]
            sq = np.zeros(D.shape[1])
            for i in range(r):  # the squares in index order
                sq += D[i] * D[i]
            want = np.sqrt(sq).max()
            got = o["status"][t][q, 6]
            print("rank %d round %d agent %d: relative change %.17g, numpy %.17g" % (k, t + 1, q, got, want))
            assert o["status"][t][q, 0] == 1 and o["status"][t][q, 4] == t + 1
            assert want > 0 and abs(got - want) <= RTOL_KERNEL * want, (k, t, got, want)
            assert got == ref["status"][t][q, 6], (k, t)
            before = after
        for key in EXACT_VIEW:
            assert np.array_equal(o[key], ref[key]), (k, key)


# ---- 3-5. the run loop of a robust team -----------------------------------------------------------------------------
RUN_KEYS = ("iters", "selected", "updated", "weight_updates", "stop", "final_status", "final_decide", "final_info",
            "final_lc", "W", "X")

_refs = {}


def _single_run_team(da, path, X0, gnc, team):
    from dcora_amd import robust as rb
    s = da.RaRbcdSession(da.RADataset(path), R_GNC, robust=rb.RobustCostParameters("GNC_TLS", **gnc))
    s.enable_team(**team)
    s.set_X(X0)
    ref = tw.run_team_record(s, s.R, s.get_weights, s.get_X)
    ref["robots"] = s.robots
    s.close()
    return ref


def _run_team_case(da, variants, tmp_path, name, gnc, world, team, transport=None):
    path = variants[name][0]
    ra = da.RADataset(path)
    X0 = _odom_start(ra, R_GNC)
    key = (name, tuple(sorted(team.items())))
    if key not in _refs:  # (2 and 4 ranks and the staged transport share one reference)
        _refs[key] = _single_run_team(da, path, X0, gnc, team)
    ref = _refs[key]
    print("reference: %d rounds, updates in rounds %s, stop %d, %d closures rejected" % (
        ref["iters"], np.flatnonzero(ref["updated"]).tolist(), ref["stop"], int(np.sum(ref["W"] == 0.0))))
    # the counts of every agent are those of the dataset carrying the run's final weights
    ra.set_pose_pose_weights(ref["W"])
    want = [stats_numpy(ra, robot) for robot in ref["robots"]]
    assert ref["final_lc"].tolist() == [[c["accepted"], c["rejected"], c["total"]] for c in want]
    res = run_ranks(tmp_path, world, path, X0, dict(mode="run_team", r=R_GNC, gnc=gnc, team=team), transport=transport)
    for k, o in enumerate(res):
        _same_run(o, ref, k, RUN_KEYS)
    return ref


@pytest.mark.parametrize("world,transport", [(2, None), (4, None), (2, "staged")])
def test_robust_run_team_equals_the_one_process_run(da, variants, tmp_path, world, transport):
    ref = _run_team_case(da, variants, tmp_path, "gnc", STEP8, world, TEAM, transport)
    # (so that the case cannot pass empty)
    assert int(ref["weight_updates"]) >= 1 and int(ref["final_info"][3]) == 1
    assert np.any(ref["W"] < 1e-8), "no closure was rejected"
    assert int(ref["stop"]) == tw.STOP["all_ready"] and ref["final_status"][:, 5].all()


def test_run_team_stopped_by_the_cap(da, variants, tmp_path):
    ref = _run_team_case(da, variants, tmp_path, "gnc", STEP8, 2, dict(TEAM, max_num_iters=25))
    assert int(ref["stop"]) == tw.STOP["max_iters"] and int(ref["iters"]) == 25


def test_run_team_on_the_sparse_path(da, variants, tmp_path):
    ra = da.RADataset(variants["sparse"][0])
    assert min(len(ra.agent_columns[q][1]) for q in ra.robots) > K_DENSE_MAX
    ref = _run_team_case(da, variants, tmp_path, "sparse", FROM_005, 2,
                         dict(max_num_iters=12, robust_opt_num_weight_updates=2, robust_opt_inner_iters=4))
    assert int(ref["weight_updates"]) == 2 and np.any(ref["W"] == 0.0)  # both fired by the inner-iteration cap


# ---- 6. coloured ticks ----------------------------------------------------------------------------------------------
def test_ticks_carry_the_statuses_of_their_colour(da, variants, tmp_path):
    path = variants["ring"]
    ra = da.RADataset(path)
    X0 = _odom_start(ra, R_GNC)
    s = da.RaRbcdSession(ra, R_GNC, acceleration=False)
    s.enable_team()
    s.set_X(X0)
    ref = tw.tick_sweeps(s, s.iterate_set, s, s.R, 3)
    ref["X"] = s.get_X()
    s.close()
    col = ref["colours"]
    nc = int(col.max()) + 1
    assert 2 <= nc < len(col), "some colour has more than one agent"
    for t in range(len(ref["status"])):  # the colour's agents are known after its tick, the others untouched
        mine = col == t % nc
        assert ref["status"][t][mine, 0].all() and np.all(ref["status"][t][mine, 4] == t + 1)
        assert np.all(ref["status"][t][mine, 6] > 0)
        if t:
            assert np.array_equal(ref["status"][t][~mine], ref["status"][t - 1][~mine])
    res = run_ranks(tmp_path, 2, path, X0, dict(mode="ticks", r=R_GNC, sweeps=3, accel=False))
    for k, o in enumerate(res):
        for key in EXACT_VIEW + ("colours", "X"):
            assert np.array_equal(o[key], ref[key]), (k, key)


# ---- 7. enabling changes no iterate ---------------------------------------------------------------------------------
def test_enabling_the_team_changes_no_iterate_and_adds_one_launch_where_the_agent_lives(da, variants, tmp_path):
    path = variants["gnc"][0]
    X0 = _odom_start(da.RADataset(path), R_GNC)
    rounds = 12
    res = {}
    for enable in (False, True):
        sub = tmp_path / ("on" if enable else "off")
        sub.mkdir()
        res[enable] = run_ranks(sub, 2, path, X0, dict(mode="greedy", r=R_GNC, rounds=rounds, enable=enable, count=True))
    hosts = set()
    for k in range(2):
        off, on = res[False][k], res[True][k]
        for key in ("X", "cost", "gradnorm", "selected"):
            assert np.array_equal(off[key], on[key]), (k, key)
        here = np.isin(on["selected"], on["hosted"])
        hosts |= {k} if here.any() else set()
        assert np.all(off["launches"] > 0)
        assert np.array_equal(on["launches"] - off["launches"], here.astype(int)), (k, on["launches"], off["launches"])
    assert hosts == {0, 1}, "agents of both ranks were selected"


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_are_collective_and_harmless(da, variants, tmp_path):
    from dcora_amd import capi
    from dcora_amd import robust as rb
    path = variants["gnc"][0]
    ra = da.RADataset(path)
    X0 = _odom_start(ra, R_GNC)
    s = da.RaRbcdSession(ra, R_GNC, robust=rb.RobustCostParameters("GNC_TLS", **STEP8))
    s.set_X(X0)
    first = tw.greedy_rounds(s, None, s.R, 6)
    s.enable_team()  # (what the job does after its refused calls: six rounds, enable, two more)
    more = tw.greedy_rounds(s, s, s.R, 2)
    s.close()
    res = run_ranks(tmp_path, 2, path, X0, dict(mode="refusals", r=R_GNC, gnc=STEP8, rounds=6))
    for k, o in enumerate(res):
        # dcora_ra_rbcd_team_enable on a rank and the foreign exchange: DCORA_ERR_UNSUPPORTED; that exchange iterates
        assert list(o["refused"]) == [8, 8, 0], (k, o["refused"])
        assert np.array_equal(o["selected"], first["selected"])
        assert np.allclose(o["cost"], first["cost"], rtol=1e-9, atol=1e-12)
        for key in EXACT_VIEW + ("selected",):
            assert np.array_equal(o["more_" + key], more[key]), (k, key)
        assert np.allclose(o["more_cost"], more["cost"], rtol=1e-9, atol=1e-12)
    # one rank: the exchange's entry after the session's own
    own = da.RaRbcdSession(ra, R_GNC)
    ex = da.Exchange(own, "rto%s" % uuid.uuid4().hex[:10])
    twin = da.RaRbcdSession(ra, R_GNC)
    try:
        own.enable_team()
        with pytest.raises(capi.DcoraError) as e:
            ex.enable_team_ra()
        assert e.value.status == 8 and "dcora_ra_rbcd_team_enable" in str(e.value)
        with pytest.raises(capi.DcoraError) as e:  # the pose-graph entry keeps refusing a range-aided exchange
            ex.enable_team()
        assert e.value.status == 8 and "dcora_exchange_team_enable_ra" in str(e.value)
        with pytest.raises(capi.DcoraError) as e:
            ex.should_terminate()
        assert e.value.status == 1  # DCORA_ERR_BAD_ARG: the exchange has no team
        ex.set_X(X0)
        twin.set_X(X0)
        a, b = ex.iterate(0), twin.iterate(0)
        assert a[3] == b[3] and a[0] == pytest.approx(b[0], rel=1e-9, abs=1e-12)
        assert np.array_equal(ex.gather_X(), twin.get_X())
        assert own.agent_status(0) is not None  # the session's own team goes on
    finally:
        ex.close()
        own.close()
        twin.close()
    # ... and the range-aided entry refuses a pose-graph exchange
    ds = common.product_dataset("smallGrid3D")
    ps = da.RbcdSession(ds, num_robots=5, r=5)
    pex = da.Exchange(ps, "rtp%s" % uuid.uuid4().hex[:10])
    try:
        with pytest.raises(capi.DcoraError) as e:
            pex.enable_team_ra()
        assert e.value.status == 8
        pex.enable_team()  # its own entry serves it afterwards
        assert pex.agent_status(0) is None
    finally:
        pex.close()
        ps.close()


# ---- 9. a plain exchange without a team ------------------------------------------------------------------------------
def test_a_plain_exchange_without_a_team_is_unchanged(da, variants, tmp_path):
    path = variants["gnc"][0]
    X0 = _odom_start(da.RADataset(path), R_GNC)
    ref = _single_greedy(da, path, X0, R_GNC, 10, enable=False)
    res = run_ranks(tmp_path, 2, path, X0, dict(mode="greedy", r=R_GNC, rounds=10, enable=False))
    for k, o in enumerate(res):
        _same_run(o, ref, k, ("selected", "X"))


# ---- 10. one rank, no subprocess ------------------------------------------------------------------------------------
def test_one_rank_through_the_exchange_is_the_session(da, variants):
    from dcora_amd import robust as rb
    path = variants["gnc"][0]
    ra = da.RADataset(path)
    X0 = _odom_start(ra, R_GNC)
    # an L2 team on a plain exchange
    ref = _single_greedy(da, path, X0, R_GNC, 12)
    s = da.RaRbcdSession(ra, R_GNC)
    ex = da.Exchange(s, "rt1%s" % uuid.uuid4().hex[:10])
    try:
        ex.enable_team_ra()
        ex.set_X(X0)
        got = tw.greedy_rounds(ex, ex, s.R, 12)
        got["X"] = ex.gather_X()
    finally:
        ex.close()
        s.close()
    _same_run(got, ref, 0, EXACT_VIEW + ("selected", "X"))
    # the robust run loop
    ref = _single_run_team(da, path, X0, STEP8, TEAM)
    s, ex = da.ra_robust_ranked_session(ra, "rt2%s" % uuid.uuid4().hex[:10], R_GNC,
                                        robust=rb.RobustCostParameters("GNC_TLS", **STEP8))
    try:
        ex.enable_team_ra(**TEAM)
        ex.set_X(X0)
        got = tw.run_team_record(ex, s.R, ex.get_weights, ex.gather_X)
    finally:
        ex.close()
        s.close()
    _same_run(got, ref, 0, RUN_KEYS)


# ---- 11. the driver across two ranks --------------------------------------------------------------------------------
def test_the_team_driver_across_ranks_rejects_exactly_the_injected_outliers(da, variants, tmp_path):
    from dcora_amd import driver
    from dcora_amd import robust as rb
    path, info = variants["gnc"]
    ra = da.RADataset(path)
    X0 = _odom_start(ra, R_GNC)
    inl, outl = ra_loops.closure_masks(info)
    assert int(outl.sum()) == 6
    team = dict(robust_opt_num_weight_updates=6, max_num_iters=200)
    one = driver.ra_team_session(ra, X0, R_GNC, robust=rb.RobustCostParameters("GNC_TLS", **STEP8),
                                 team=da.team_params(**team))
    print("one process: stop %s after %d rounds, %d updates" % (one["final"]["stop_reason"], one["final"]["iterations"],
                                                               one["final"]["weight_updates"]))
    res = run_ranks(tmp_path, 2, path, X0, dict(mode="driver", r=R_GNC, gnc=STEP8, team=team))
    for k, o in enumerate(res):
        w = o["weights"]
        assert np.array_equal(o["loop_closures"], inl | outl) and np.array_equal(o["ra_weights"], w)
        assert np.all(w[outl] == 0.0), "every injected outlier is rejected"
        assert np.all(w[inl] == 1.0), "no ground-truth closure is rejected"
        assert np.all(w[~(inl | outl)] == 1.0)
        # the record's integer fields are the one-process driver's
        assert int(o["iters"]) == one["final"]["iterations"] and int(o["weight_updates"]) == one["final"]["weight_updates"]
        assert int(o["stop"]) == tw.STOP[one["final"]["stop_reason"]]
        assert np.array_equal(o["selected"], one["run"]["selected"]) and np.array_equal(o["updated"], one["run"]["updated"])
        assert o["ready"].tolist() == [bool(st and st["ready_to_terminate"]) for st in one["statuses"]]
        assert o["lc"].tolist() == [[c["accepted"], c["rejected"], c["total"]] for c in one["loop_closure_stats"]]
        assert np.array_equal(w, one["weights"]) and np.array_equal(o["X"], one["X"])
