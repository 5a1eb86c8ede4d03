"""Agent status, team termination and weight-update decisions in a range-aided session (dcora_ra_rbcd_team_enable and the
entries around it; the reference's agents run Agent::iterate's status block, shouldTerminate,
shouldUpdateMeasurementWeights and the bookkeeping of updateMeasurementWeights on a RangeAidedSLAMGraph as on a pose
graph, ref src/Agent.cpp:558-586, 1123-1156, 1280-1330, 1417-1424): the RA form of the relative-change kernel against
numpy and, bit for bit, against the pose-graph form; the status a session stores on every path that optimises an agent;
no perturbation of a run; the decisions forced branch by branch through parameters; the run loop against the same loop
made of the entries; the driver's flow on the GNC fixture; refusals.  Modelled on tests/test_team_status_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import ra_loops
import team_rules_ref as ref
from ra_ring import write_ring_variant
from test_ra_team_cpu import stats_numpy
from test_raslam import ra_path

pytestmark = pytest.mark.gpu

# at most 16 squares summed in index order and one square root: about 18 roundings of 2^-53 (2e-15), FMA or not
# (the bound of tests/test_team_status_gpu.py: the reduction is the same code)
RTOL = 1e-14


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the run-time variants the tests share, written once: gnc -> (path, info), ring -> path"""
    d = tmp_path_factory.mktemp("ra_team_status")
    return {"gnc": ra_loops.write_loops_variant(d, **ra_loops.GNC_FIXTURE), "ring": write_ring_variant(d)[0]}


def _norms(D):
    s = np.zeros(D.shape[1])
    for k in range(D.shape[0]):  # the squares in index order
        s += D[k] * D[k]
    return np.sqrt(s)


def np_ra_translation_distances(X, Y, d, n, l):
    return _norms(np.asarray(X)[:, d * n + l:d * n + l + n] - np.asarray(Y)[:, d * n + l:d * n + l + n])


def _close(got, want):
    assert want > 0 and abs(got - want) <= RTOL * want, (got, want)


def _lifted_start(orc, ra, r, seed=5, noise=0.05):  # as tests/test_ra_session.py
    rng = np.random.default_rng(seed)
    lift = np.linalg.qr(rng.standard_normal((r, ra.d)))[0]
    M = lift @ ra.gt + noise * rng.standard_normal((r, ra.k))
    return orc.project_to_manifold(r, ra.d, ra.n, M, l=ra.l, b=ra.b)


def _odom_start(ra, r):
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    return X0


# ---- 1. the kernel against numpy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,r", [(2, 2), (3, 3), (3, 5), (3, 16)])
def test_kernel_equals_numpy_on_planted_maxima(env, d, r):
    da, _ = env
    rng = np.random.default_rng(100 * d + r)
    for n, l, b in ((1, 0, 0), (25, 3, 2), (65, 0, 7), (1025, 5, 0), (2500, 4, 4)):
        k = (d + 1) * n + l + b
        t0 = d * n + l  # column of the first translation
        X = rng.standard_normal((r, k))
        base = X + 1e-3 * rng.standard_normal(X.shape)
        for pos in sorted({0, n - 1} | {p for p in (63, 64, 65, 255, 256, 1024) if p < n}):
            Y = base.copy()
            Y[:, t0 + pos] += 3.0 + rng.uniform(0, 1, r)  # the translation of pose `pos` moves furthest of the poses
            Y[:, d * pos] += 50.0                          # a rotation column, ...
            if l:
                Y[:, d * n + pos % l] += 60.0              # ... a unit sphere ...
            if b:
                Y[:, t0 + n + pos % b] += 70.0             # ... and a landmark move further still: they never count
            per_pose = np_ra_translation_distances(X, Y, d, n, l)
            assert int(np.argmax(per_pose)) == pos
            got = da.ra_max_translation_distance(X, Y, d, n, l, b)
            _close(got, per_pose.max())
            assert da.ra_max_translation_distance(X, Y, d, n, l, b) == got  # the same bits on the same input
            if l == 0 and b == 0:  # the pose-graph form's bits on the same data in the SE ordering
                Xse, Yse = np.zeros_like(X), np.zeros_like(Y)
                for A, Ase in ((X, Xse), (Y, Yse)):
                    for c in range(d):
                        Ase[:, c::d + 1] = A[:, c:d * n:d]
                    Ase[:, d::d + 1] = A[:, d * n:]
                assert da.max_translation_distance(Xse, Yse, d) == got
        assert da.ra_max_translation_distance(X, X, d, n, l, b) == 0.0


def test_kernel_entry_refuses_bad_arguments(env):
    da, _ = env
    from dcora_amd import capi
    X = np.zeros((3, 4 * 2 + 1 + 1))
    out = C.c_double()
    f = capi.lib().dcora_ra_max_translation_distance
    for r, d, n, l, b in ((1, 2, 2, 1, 1), (17, 3, 2, 1, 1), (3, 4, 2, 1, 1), (2, 3, 2, 1, 1), (3, 3, 0, 1, 1),
                          (3, 3, 2, -1, 1), (3, 3, 2, 1, -1)):
        assert f(r, d, n, l, b, da.F(X), da.F(X), C.byref(out)) == 1  # DCORA_ERR_BAD_ARG


# ---- 2. the status a session stores ---------------------------------------------------------------------------------
def np_agent_relative_change(ra, agent, robots, X, Xprev):
    """over the agent's poses only: global columns d n + l + p of the poses p its robot owns"""
    poses = np.flatnonzero(ra.pose_robot == robots[agent])
    cols = ra.d * ra.n + ra.l + poses
    return _norms(X[:, cols] - Xprev[:, cols]).max()


def _check_round(s, ra, p, sel, rnd, step, seen, robust=False):
    """step() runs one round in which agent(s) `sel` optimise; their status against numpy on get_X before / after"""
    sel = [int(q) for q in np.atleast_1d(sel)]
    before = s.get_X()
    step()
    after = s.get_X()
    for q in sel:
        st = s.agent_status(q)
        assert st is not None
        _close(st["relative_change"], np_agent_relative_change(ra, q, s.robots, after, before))
        assert st["agent_id"] == q and st["state"] == ref.INITIALIZED and st["instance_number"] == 0
        assert st["iteration_number"] == rnd
        c = s.loop_closure_stats(q)
        assert bool(st["ready_to_terminate"]) == ref.ready_to_terminate(
            p, robust, 0, True, st["relative_change"], c["accepted"], c["rejected"], c["total"])
        seen.add(q)
    for q in range(s.R):
        assert (s.agent_status(q) is not None) == (q in seen)
    return after


def test_status_on_the_session_loop_across_a_restart(env):
    da, orc = env
    ra = da.RADataset(ra_path("range_aided_slam_test_3d"))
    assert ra.l > 0 and ra.b > 0  # the translation offset d n_a + l_a matters
    s = da.RaRbcdSession(ra, 4, acceleration=True, restart_interval=4)
    p = s.enable_team()
    s.set_X(_lifted_start(orc, ra, 4))
    seen = set()
    for it in range(9):  # two restart rounds included
        _check_round(s, ra, p, it % 2, it + 1, lambda: s.iterate(it % 2), seen)
    # the run loop stores them too: agent_status after run() is the status of the agent's last optimisation
    X8 = s.get_X()
    out = s.run(max_iters=1, rgrad_tol=0.0)
    q = int(out["selected"][0])
    st = s.agent_status(q)
    assert st["iteration_number"] == 10
    _close(st["relative_change"], np_agent_relative_change(ra, q, s.robots, s.get_X(), X8))
    s.close()


def test_status_on_ticks_of_two_agents_and_on_the_coloured_run(env, files):
    da, _ = env
    ra = da.RADataset(files["ring"])
    r = 3
    X0 = _odom_start(ra, r)
    A = da.RaRbcdSession(ra, r, acceleration=False)
    B = da.RaRbcdSession(ra, r, acceleration=False)
    p = A.enable_team()
    B.enable_team()
    A.set_X(X0)
    B.set_X(X0)
    col, nc = A.colours()
    assert col.tolist() == [0, 1, 0, 1] and nc == 2
    sets = [np.flatnonzero(col == c).astype(np.int32) for c in range(nc)]
    # every agent has more poses than one pass of a workgroup (256 threads)
    assert min(int(np.sum(ra.pose_robot == q)) for q in ra.robots) > 256
    seen = set()
    _check_round(A, ra, p, sets[0], 1, lambda: A.iterate_set(sets[0]), seen)
    _check_round(A, ra, p, sets[1], 2, lambda: A.iterate_set(sets[1]), seen)
    # dcora_ra_rbcd_run_coloured is that sweep: the same statuses, bit for bit
    B.run_coloured(max_sweeps=1, rgrad_tol=0.0)
    assert np.array_equal(A.get_X(), B.get_X())
    assert [A.agent_status(q) for q in range(A.R)] == [B.agent_status(q) for q in range(B.R)]
    assert not A.should_update_weights()
    # set_X restarts the bookkeeping; a tick of one colour leaves the other colour's agents unknown
    A.set_X(X0)
    assert all(A.agent_status(q) is None for q in range(A.R))
    seen = set()
    _check_round(A, ra, p, sets[1], 1, lambda: A.iterate_set(sets[1]), seen)
    # ---- 3. no perturbation: three coloured sweeps, enabled and plain
    plain = da.RaRbcdSession(ra, r, acceleration=False)
    outs, Xs = [], []
    for s in (plain, B):
        s.set_X(X0)
        outs.append(s.run_coloured(max_sweeps=3, rgrad_tol=0.0))
        Xs.append(s.get_X())
    assert all(B.agent_status(q)["iteration_number"] == 5 + q % 2 for q in range(B.R))
    for key in ("cost", "gradnorm"):
        assert np.array_equal(outs[0][key], outs[1][key]), key
    assert np.array_equal(Xs[0], Xs[1])
    for s in (A, B, plain):
        s.close()


def test_an_enabled_session_runs_the_same_bits(env):
    da, orc = env
    ra = da.RADataset(ra_path("range_aided_slam_test_3d"))
    X0 = _lifted_start(orc, ra, 4)
    outs, Xs = [], []
    for enabled in (False, True):
        s = da.RaRbcdSession(ra, 4, restart_interval=5)
        if enabled:
            s.enable_team()
        s.set_X(X0)
        outs.append(s.run(max_iters=12, rgrad_tol=0.0))
        Xs.append(s.get_X())
        if enabled:
            assert any(s.agent_status(q) is not None for q in range(s.R))
        s.close()
    for key in ("selected", "cost", "gradnorm"):
        assert np.array_equal(outs[0][key], outs[1][key]), key
    assert np.array_equal(Xs[0], Xs[1])


# ---- 4. decisions, forced by parameters and not by data -------------------------------------------------------------
def test_l2_termination_by_readiness_and_by_the_iteration_cap(env):
    da, orc = env
    ra = da.RADataset(ra_path("range_aided_slam_test_3d"))
    X0 = _lifted_start(orc, ra, 4)
    s = da.RaRbcdSession(ra, 4)  # a plain session: an L2 team
    s.enable_team(rel_change_tol=1e9)  # every optimised agent is ready (its loop closures all carry weight 1)
    s.set_X(X0)
    for q in range(s.R):
        c = s.loop_closure_stats(q)
        assert c == stats_numpy(ra, s.robots[q]) and c["accepted"] == c["total"] > 0
    assert not s.should_terminate() and not s.should_update_weights()
    for it, sel in enumerate([1, 1, 0, 1]):  # the second agent optimises in round 3
        s.iterate(sel)
        assert s.should_terminate() == (it + 1 >= 3), it
        assert not s.should_update_weights()  # L2: never
    s.enable_team(rel_change_tol=0.0, max_num_iters=5)  # nobody is ever ready: only the cap ends the run
    s.set_X(X0)
    for it in range(7):
        s.iterate(it % 2)
        assert s.should_terminate() == (it + 1 >= 5), it
        assert all(not s.agent_status(q)["ready_to_terminate"] for q in range(min(it + 1, s.R)))
    assert s.team_info() == dict(inner_iter=0, latest_weight_update_iteration=0, weight_updates=0, resets=0)
    s.close()


def _robust_session(da, files, cost="GNC_TLS", r=3, **team):
    from dcora_amd import robust as rb
    path, info = files["gnc"]
    ra = da.RADataset(path)
    kw = dict(ra_loops.GNC_PARAMS) if cost == "GNC_TLS" else {}
    s = da.RaRbcdSession(ra, r, robust=rb.RobustCostParameters(cost, **kw))
    p = s.enable_team(**team)
    s.set_X(_odom_start(ra, r))
    return ra, info, s, p


def _session_stats_numpy(da, files, s):
    """the CPU test's counter on the file with the session's current pose-pose weights"""
    ra = da.RADataset(files["gnc"][0])
    ra.set_pose_pose_weights(s.get_weights())
    return [stats_numpy(ra, robot) for robot in s.robots]


def test_the_bookkeeping_of_weight_updates_set_weights_and_set_X(env, files):
    da, _ = env
    ra, info, s, p = _robust_session(da, files, robust_opt_inner_iters=3)
    R = s.R
    assert R == 4
    assert s.team_info() == dict(inner_iter=0, latest_weight_update_iteration=0, weight_updates=0, resets=0)
    assert [s.loop_closure_stats(q) for q in range(R)] == _session_stats_numpy(da, files, s)
    for it in range(3):  # the other agents never get a status: only the inner-iteration cap can fire
        s.iterate(2)
        assert s.team_info()["inner_iter"] == it + 1
        assert s.should_update_weights() == (it + 1 >= 3), it
        assert not s.should_terminate()
    assert [s.agent_status(q) is not None for q in range(R)] == [False, False, True, False]
    # update_weights: the bookkeeping of ref src/Agent.cpp:1417-1424
    s.update_weights()
    assert all(s.agent_status(q) is None for q in range(R))
    assert s.team_info() == dict(inner_iter=0, latest_weight_update_iteration=3, weight_updates=1, resets=0)
    assert [s.loop_closure_stats(q) for q in range(R)] == _session_stats_numpy(da, files, s)
    assert not s.should_update_weights()
    s.iterate(1)
    assert s.agent_status(1)["iteration_number"] == 4 and s.team_info()["inner_iter"] == 1
    # set_weights only refreshes the counts
    st, ti = [s.agent_status(q) for q in range(R)], s.team_info()
    before = [s.loop_closure_stats(q) for q in range(R)]
    w = s.get_weights()
    lc = np.flatnonzero(ra.loop_closures())
    w[lc[0]], w[lc[1]] = 0.5, 0.0
    s.set_weights(w)
    after = [s.loop_closure_stats(q) for q in range(R)]
    assert after == _session_stats_numpy(da, files, s) and after != before
    assert [s.agent_status(q) for q in range(R)] == st and s.team_info() == ti
    # set_X and set_acceleration restart the bookkeeping with the rounds
    for restart in (lambda: s.set_X(_odom_start(ra, 3)), lambda: s.set_acceleration(True)):
        s.iterate(0)
        assert s.agent_status(0) is not None and s.team_info()["inner_iter"] > 0
        restart()
        assert all(s.agent_status(q) is None for q in range(R))
        assert s.team_info() == dict(inner_iter=0, latest_weight_update_iteration=0, weight_updates=1, resets=0)
        assert [s.loop_closure_stats(q) for q in range(R)] == after
        s.iterate(3)
        assert s.agent_status(3)["iteration_number"] == 1
    s.close()


def test_an_undecided_shared_closure_holds_back_exactly_its_two_agents(env, files):
    da, _ = env
    # (the L2 cost in a session with robust state: set_weights works, and the tolerance is the parameter throughout)
    ra, info, s, p = _robust_session(da, files, cost="L2", rel_change_tol=1e9, robust_opt_min_convergence_ratio=1.0)
    R = s.R
    ids = ra.pose_pose()[0]
    e = info["n_odometry"] + info["kind"].index("inter")
    touched = {s.robots.index(int(ra.pose_robot[ids[e, 0]])), s.robots.index(int(ra.pose_robot[ids[e, 1]]))}
    assert len(touched) == 2
    for q in range(R):  # the fixture's condition: nothing but the planted weight holds anybody back
        c = s.loop_closure_stats(q)
        assert c["accepted"] == c["total"] > 0
    for q in range(R):
        s.iterate(q)
    assert all(s.agent_status(q)["ready_to_terminate"] for q in range(R)) and s.should_terminate()
    w = s.get_weights()
    w[e] = 0.5
    w[info["n_odometry"] + info["kind"].index("intra")] = 0.0  # a rejected closure is a decided one: it holds nobody back
    s.set_weights(w)
    stats = [s.loop_closure_stats(q) for q in range(R)]
    assert stats == _session_stats_numpy(da, files, s)
    for q in range(R):  # every other agent's ratio is still 1
        assert (stats[q]["accepted"] + stats[q]["rejected"] == stats[q]["total"]) == (q not in touched)
    assert all(s.agent_status(q)["ready_to_terminate"] for q in range(R))  # setMeasurementWeight touches no status
    for q in range(R):
        s.iterate(q)
    assert {q for q in range(R) if not s.agent_status(q)["ready_to_terminate"]} == touched
    assert not s.should_terminate()
    s.close()


# ---- 5. the run loop ------------------------------------------------------------------------------------------------
def test_run_team_is_the_callers_loop_over_the_entries(env, files):
    da, _ = env
    team = dict(max_num_iters=60, robust_opt_num_weight_updates=3, robust_opt_inner_iters=8)
    _, _, A, p = _robust_session(da, files, **team)
    _, _, B, _ = _robust_session(da, files, **team)
    R = A.R
    out = A.run_team()
    cost, gn, sel, upd = [], [], [], []
    selected = rnd = 0
    while True:
        statuses = [B.agent_status(q) for q in range(R)]
        info = B.team_info()
        stop = B.should_terminate()
        assert stop == ref.should_terminate(p, True, rnd, info["weight_updates"], statuses)
        if stop:
            break
        update = B.should_update_weights()
        assert update == ref.should_update_weights(p, True, info["weight_updates"], info["inner_iter"],
                                                   info["latest_weight_update_iteration"], statuses)
        if update:
            B.update_weights(reset_to_initial=info["resets"] < p.robust_opt_num_resets)
        c2, g, _, nxt = B.iterate(selected)
        rnd += 1
        cost.append(c2), gn.append(g), sel.append(selected), upd.append(int(update))
        selected = nxt
    assert out["iters"] == len(cost) <= p.max_num_iters
    assert np.array_equal(out["cost"], np.array(cost)) and np.array_equal(out["gradnorm"], np.array(gn))
    assert np.array_equal(out["selected"], np.array(sel)) and np.array_equal(out["updated"], np.array(upd))
    assert np.array_equal(A.get_weights(), B.get_weights()) and np.array_equal(A.get_X(), B.get_X())
    assert out["weight_updates"] == sum(upd) == A.team_info()["weight_updates"]
    assert 1 <= out["weight_updates"] <= p.robust_opt_num_weight_updates
    final = [A.agent_status(q) for q in range(R)]
    assert final == [B.agent_status(q) for q in range(R)]
    if out["stop_reason"] == "max_iters":
        assert rnd == p.max_num_iters
    else:
        assert out["stop_reason"] == "all_ready" and rnd < p.max_num_iters
        assert all(st is not None and st["ready_to_terminate"] for st in final)
        assert out["weight_updates"] == p.robust_opt_num_weight_updates
    A.close()
    B.close()


# ---- 6. the driver --------------------------------------------------------------------------------------------------
def test_the_team_driver_rejects_exactly_the_injected_outliers(env, files):
    da, _ = env
    from dcora_amd import driver
    from dcora_amd import robust as rb
    r = 3
    path, info = files["gnc"]
    ra = da.RADataset(path)
    inl, outl = ra_loops.closure_masks(info)
    team = da.team_params(robust_opt_num_weight_updates=20, max_num_iters=1000)
    out = driver.ra_team_session(ra, _odom_start(ra, r), r,
                                 robust=rb.RobustCostParameters("GNC_TLS", **ra_loops.GNC_PARAMS), team=team)
    w, fin = out["weights"], out["final"]
    print("stop %s after %d rounds, %d updates; outlier weights <= %.3g, closure weights >= %.3g, final 2f %.6g" % (
        fin["stop_reason"], fin["iterations"], fin["weight_updates"], w[outl].max(), w[inl].min(), fin["cost_2f"]))
    assert np.array_equal(out["loop_closures"], inl | outl)
    assert np.array_equal(ra.pose_pose_weights, w)
    # every update comes after at most robust_opt_inner_iters = 30 rounds and nothing stops the team before the last:
    # all 20 are made by round 600 of 1000
    assert fin["weight_updates"] == 20 and fin["iterations"] <= 1000
    if fin["stop_reason"] == "all_ready":
        assert all(st is not None and st["ready_to_terminate"] for st in out["statuses"])
    else:
        assert fin["stop_reason"] == "max_iters" and fin["iterations"] == 1000
    assert np.all(w[~(inl | outl)] == 1.0)
    assert np.all((w[inl | outl] == 0.0) | (w[inl | outl] == 1.0)), "every non-fixed closure is decided"
    assert np.all(w[outl] == 0.0), "every injected outlier is rejected"
    assert np.all(w[inl] == 1.0), "no ground-truth closure is rejected"
    assert out["loop_closure_stats"] == [stats_numpy(ra, robot) for robot in ra.robots]


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_refusals(env):
    da, orc = env
    from dcora_amd import capi
    ra = da.RADataset(ra_path("range_aided_slam_test_3d"))
    s = da.RaRbcdSession(ra, 4)
    X0 = _lifted_start(orc, ra, 4)
    s.set_X(X0)
    s.iterate(0)
    X1 = s.get_X()
    s.team = da.team_params()
    for call in (lambda: s.agent_status(0), lambda: s.loop_closure_stats(0), s.should_terminate,
                 s.should_update_weights, s.team_info, s.run_team):
        with pytest.raises(capi.DcoraError) as e:
            call()
        assert e.value.status == 1  # DCORA_ERR_BAD_ARG
    assert np.array_equal(s.get_X(), X1)
    s.enable_team(max_num_iters=4, rel_change_tol=0.0)  # nobody is ever ready: only the cap ends a run
    for call in (lambda: s.agent_status(s.R), lambda: s.agent_status(-1), lambda: s.loop_closure_stats(s.R)):
        with pytest.raises(capi.DcoraError) as e:
            call()
        assert e.value.status == 1
    assert np.array_equal(s.get_X(), X1) and all(s.agent_status(q) is None for q in range(s.R))
    # the session is as it was: it goes on like a twin that was never asked
    twin = da.RaRbcdSession(ra, 4)
    twin.set_X(X0)
    twin.iterate(0)
    assert s.iterate(1)[:2] == twin.iterate(1)[:2] and np.array_equal(s.get_X(), twin.get_X())
    # run_team without traces: rounds 3 and 4 up to the cap
    it, nupd, why = C.c_int(), C.c_int(), C.c_int()
    capi.check(capi.lib().dcora_ra_rbcd_run_team(s.h, C.byref(it), None, None, None, None, C.byref(nupd),
                                                 C.byref(why)))
    assert (it.value, nupd.value, why.value) == (2, 0, capi.TEAM_STOP_MAX_ITERS)
    assert s.should_terminate()
    s.close()
    twin.close()
    ranked = da.RaRbcdSession(ra, 4, rank=0, world_size=2)
    with pytest.raises(capi.DcoraError) as e:
        ranked.enable_team()
    assert e.value.status == 8  # DCORA_ERR_UNSUPPORTED
    ranked.close()
