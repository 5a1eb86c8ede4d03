"""The team protocol across the ranks of a job (dcora_exchange_team_enable, _agent_status, _loop_closure_stats,
_should_terminate, _should_update_weights, _team_info, _run_team; Agent::iterate's status block, shouldTerminate,
shouldUpdateMeasurementWeights, ref src/Agent.cpp:558-586, 1123-1156, 1280-1330): several processes (one per rank, all
on device 0) must hold, on every rank, the statuses and decisions of the single-process session that called
dcora_rbcd_team_enable -- integers, statuses (the relative change included), weights and X bit for bit, costs to
rounding (the evaluation sums per agent) -- on greedy iterations, ticks, and the run loop that re-weights and stops by
the rules."""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import common
import team_ranks_worker as tw

pytestmark = pytest.mark.gpu

WORKER = os.path.join(common.HERE, "team_ranks_worker.py")
FAST = dict(GNCBarc=10.0, GNCMuStep=4.0)  # as tests/test_gnc_ranks_gpu.py
R, RANK = 5, 5
TEAM = dict(max_num_iters=120, robust_opt_num_weight_updates=4, robust_opt_inner_iters=10, robust_opt_num_resets=1)


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    if dcora_amd.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return dcora_amd


def _with_outliers(ds_cls, base, n_out, seed):
    # (as tests/test_gnc_ranks_gpu.py builds them)
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


def _problem(da, name, n_out, seed=2, r=RANK):
    """the dataset with its outliers and X0 = the chordal initialisation of the clean graph, lifted to rank r"""
    clean = common.product_dataset(name)
    T = da.chordal_initialization(clean)
    X0 = np.zeros((r, (clean.d + 1) * clean.n))
    X0[:clean.d] = T
    return clean, _with_outliers(da.Dataset, clean, n_out, seed), X0


def _copy(da, ds):
    return da.Dataset(ds.d, ds.n, ds.ids.copy(), ds.vals.copy())


def run_ranks(tmp_path, world, ds, X0, cfg, transport=None):
    d = str(tmp_path)
    np.save(os.path.join(d, "ids.npy"), ds.ids)
    np.save(os.path.join(d, "vals.npy"), ds.vals)
    np.save(os.path.join(d, "X0.npy"), X0)
    with open(os.path.join(d, "job.json"), "w") as f:
        json.dump(dict(cfg, d=ds.d, n=ds.n), f)
    job = "t%s" % uuid.uuid4().hex[:12]
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


EXACT_VIEW = ("status", "decide", "info", "lc")


def _same_run(o, ref, k, keys):
    for key in keys:
        assert np.array_equal(o[key], ref[key]), (k, key, o[key], ref[key])
    assert np.allclose(o["cost"], ref["cost"], rtol=1e-11, atol=0), (k, np.max(np.abs(o["cost"] / ref["cost"] - 1)))
    assert np.allclose(o["gradnorm"], ref["gradnorm"], rtol=1e-9, atol=0)


# ---- 1. an L2 team on greedy iterations -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def l2_reference(da):
    ds = common.product_dataset("smallGrid3D")
    X0 = common.random_point(RANK, ds.d, ds.n, 3, da.manifold_project)
    s = da.RbcdSession(ds, num_robots=R, r=RANK)
    s.enable_team()
    s.set_X(X0)
    ref = tw.greedy_rounds(s, s, R, 40)
    ref["X"] = s.get_X()
    s.close()
    return ds, X0, ref


@pytest.mark.parametrize("world", [2, 4])  # 4 ranks: rank 3 hosts no agent
def test_l2_team_holds_the_single_sessions_statuses_on_every_rank(da, tmp_path, l2_reference, world):
    ds, X0, ref = l2_reference
    assert ref["status"][-1, :, 0].any()
    assert not ref["decide"][:, 1].any()  # the L2 rules never ask for an update
    res = run_ranks(tmp_path, world, ds, X0, dict(mode="greedy", R=R, r=RANK, rounds=40))
    for k, o in enumerate(res):
        _same_run(o, ref, k, EXACT_VIEW + ("selected", "X"))


# ---- 2-4, 6. the run loop of a robust team --------------------------------------------------------------------------
def _single_run_team(da, ds, X0, team):
    from dcora_amd import robust as rb
    s = da.RbcdSession(_copy(da, ds), num_robots=R, r=RANK, robust=rb.RobustCostParameters("GNC_TLS", **FAST))
    s.enable_team(**team)
    s.set_X(X0)
    ref = tw.run_team_record(s, R, s.get_weights, s.get_X)
    s.close()
    return ref


RUN_KEYS = ("iters", "selected", "updated", "weight_updates", "stop", "final_status", "final_decide", "final_info",
            "final_lc", "W", "X")

_refs = {}


def _run_team_case(da, tmp_path, name, n_out, world, team, transport=None):
    clean, ds, X0 = _problem(da, name, n_out)
    key = (name, tuple(sorted(team.items())))
    if key not in _refs:  # (2 and 4 ranks and the staged transport share one reference)
        _refs[key] = _single_run_team(da, ds, X0, team)
    ref = _refs[key]
    res = run_ranks(tmp_path, world, ds, X0, dict(mode="run_team", R=R, r=RANK, gnc=FAST, team=team),
                    transport=transport)
    for k, o in enumerate(res):
        _same_run(o, ref, k, RUN_KEYS)
    return ref


@pytest.mark.parametrize("world,transport", [(2, None), (4, None), (2, "staged")])
def test_robust_run_team_equals_the_single_process(da, tmp_path, world, transport):
    ref = _run_team_case(da, tmp_path, "smallGrid3D", 12, world, TEAM, transport)
    # (so that the case cannot pass empty) at least two weight updates, the first with a reset
    assert int(ref["weight_updates"]) >= 2 and int(ref["final_info"][3]) == 1


def test_run_team_stopped_by_the_cap(da, tmp_path):
    ref = _run_team_case(da, tmp_path, "smallGrid3D", 12, 2, dict(TEAM, max_num_iters=25))
    assert int(ref["stop"]) == tw.STOP["max_iters"] and int(ref["iters"]) == 25


def test_run_team_on_the_dense_path(da, tmp_path):
    ref = _run_team_case(da, tmp_path, "sphere2500", 20, 2, dict(TEAM, robust_opt_inner_iters=4, max_num_iters=14))
    assert int(ref["weight_updates"]) >= 2 and int(ref["final_info"][3]) == 1  # fired by the inner-iteration cap


# ---- 5. ticks -------------------------------------------------------------------------------------------------------
def test_ticks_carry_the_statuses_of_their_colour(da, tmp_path):
    ds = common.product_dataset("smallGrid3D")
    X0 = common.random_point(RANK, ds.d, ds.n, 3, da.manifold_project)
    s = da.RbcdSession(ds, num_robots=R, r=RANK, acceleration=False)
    s.enable_team()
    s.set_X(X0)
    ref = tw.tick_sweeps(s, s.iterate_set, s, R, 3)
    ref["X"] = s.get_X()
    s.close()
    col = ref["colours"]
    nc = int(col.max()) + 1
    assert nc >= 2
    for t in range(len(ref["status"])):  # the colour's agents are known after its tick, the others untouched
        mine = col == t % nc
        assert ref["status"][t][mine, 0].all() and np.all(ref["status"][t][mine, 4] == t + 1)
        if t:
            assert np.array_equal(ref["status"][t][~mine], ref["status"][t - 1][~mine])
    res = run_ranks(tmp_path, 2, ds, X0, dict(mode="ticks", R=R, r=RANK, sweeps=3, accel=False))
    for k, o in enumerate(res):
        for key in EXACT_VIEW + ("colours", "X"):
            assert np.array_equal(o[key], ref[key]), (k, key)


# ---- 7. enabling changes no iterate ---------------------------------------------------------------------------------
def test_enabling_the_team_changes_no_iterate_and_adds_one_launch_per_round(da, tmp_path):
    ds = common.product_dataset("smallGrid3D")
    X0 = common.random_point(RANK, ds.d, ds.n, 3, da.manifold_project)
    rounds = 20
    res = {}
    for enable in (False, True):
        sub = tmp_path / ("on" if enable else "off")
        sub.mkdir()
        res[enable] = run_ranks(sub, 2, ds, X0, dict(mode="greedy", R=R, r=RANK, rounds=rounds, enable=enable))
    for k in range(2):
        for key in ("X", "cost", "gradnorm", "selected"):
            assert np.array_equal(res[False][k][key], res[True][k][key]), (k, key)
    launches = {e: sum(int(o["launches"]) for o in res[e]) for e in res}
    assert launches[False] > 0 and launches[True] - launches[False] == rounds, launches


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_are_collective_and_harmless(da, tmp_path):
    from dcora_amd import capi
    ds = common.product_dataset("smallGrid3D")
    X0 = common.random_point(RANK, ds.d, ds.n, 3, da.manifold_project)
    s = da.RbcdSession(ds, num_robots=R, r=RANK)
    s.set_X(X0)
    tw.greedy_rounds(s, None, R, 6)
    s.enable_team()  # (what the job does after its refused calls: enable, two more rounds)
    more = tw.greedy_rounds(s, s, R, 2)
    s.close()
    res = run_ranks(tmp_path, 2, ds, X0, dict(mode="refusals", R=R, r=RANK, rounds=6))
    for k, o in enumerate(res):
        assert list(o["refused"]) == [1] * 6 + [1], (k, o["refused"])  # DCORA_ERR_BAD_ARG
        assert np.array_equal(o["status"], more["status"]) and np.array_equal(o["decide"], more["decide"])
        assert np.array_equal(o["selected"], more["selected"])
        assert np.allclose(o["cost"], more["cost"], rtol=1e-11, atol=0)
    # a range-aided job has no team
    from test_raslam import ra_path
    ra = da.RADataset(ra_path("range_aided_slam_test_2d"))
    rs = da.RaRbcdSession(ra, 3)
    ex = da.Exchange(rs, "tra%s" % uuid.uuid4().hex[:10])
    try:
        with pytest.raises(capi.DcoraError) as e:
            ex.enable_team()
        assert e.value.status == 8  # DCORA_ERR_UNSUPPORTED
    finally:
        ex.close()
        rs.close()
    # ... and a session of a job is still pointed to its exchange
    ranked = da.RbcdSession(ds, num_robots=R, r=RANK, rank=0, world_size=2)
    with pytest.raises(capi.DcoraError) as e:
        ranked.enable_team()
    assert e.value.status == 8 and "dcora_exchange_team_enable" in str(e.value)
    ranked.close()


# ---- 9. one rank, no subprocess -------------------------------------------------------------------------------------
def test_one_rank_through_the_exchange_is_the_session(da):
    from dcora_amd import driver
    from dcora_amd import robust as rb
    clean, ds, X0 = _problem(da, "smallGrid3D", 12)
    params = rb.RobustCostParameters("GNC_TLS", **FAST)
    ref = _single_run_team(da, ds, X0, TEAM)
    s, ex = da.robust_ranked_session(_copy(da, ds), "t1%s" % uuid.uuid4().hex[:10], num_robots=R, r=RANK, robust=params)
    try:
        ex.enable_team(**TEAM)
        ex.set_X(X0)
        got = tw.run_team_record(ex, R, ex.get_weights, ex.gather_X)
    finally:
        ex.close()
        s.close()
    _same_run(got, ref, 0, RUN_KEYS)
    team = da.team_params(**TEAM)
    one = driver.multi_robot_team_session(_copy(da, ds), X0, num_robots=R, r=RANK, robust=params, team=team)
    ranks = driver.multi_robot_team_ranks(_copy(da, ds), X0, num_robots=R, r=RANK, robust=params, team=team,
                                          job_name="d1%s" % uuid.uuid4().hex[:10])
    assert np.array_equal(one["weights"], ranks["weights"]) and np.array_equal(one["X"], ranks["X"])
    assert ranks["final"]["cost_2f"] == pytest.approx(one["final"]["cost_2f"], rel=1e-11, abs=0)
    assert one["statuses"] == ranks["statuses"] and one["final"]["stop_reason"] == ranks["final"]["stop_reason"]


# ---- 10. the driver across two ranks --------------------------------------------------------------------------------
def test_the_team_driver_across_ranks_rejects_the_injected_outliers(da, tmp_path):
    from dcora_amd import driver
    clean, ds, X0 = _problem(da, "smallGrid3D", 12)
    res = run_ranks(tmp_path, 2, ds, X0, dict(mode="driver", R=R, r=RANK, gnc=FAST,
                                              team=dict(robust_opt_num_weight_updates=20)))
    lc = driver.loop_closure_mask(ds, R)
    m0 = clean.m
    for o in res:
        w = o["weights"]
        assert np.array_equal(o["ds_weights"], w)
        assert np.all(w[~lc] == 1.0)
        assert np.all(w[m0:] < 1e-8), "every injected closure is rejected"
        assert np.all(w[:m0][lc[:m0]] > 1 - 1e-8), "every original closure is kept"
        assert np.array_equal(o["X"], res[0]["X"]) and np.array_equal(w, res[0]["weights"])
        assert int(o["iters"]) == int(res[0]["iters"]) and int(o["stop"]) == int(res[0]["stop"])
