"""Agent status, team termination and weight-update decisions in a session (dcora_rbcd_team_enable and the entries
around it; Agent::iterate's status block, shouldTerminate, shouldUpdateMeasurementWeights and the bookkeeping of
updateMeasurementWeights, ref src/Agent.cpp:558-586, 1123-1156, 1280-1330, 1417-1424): the kernel of the relative
change against numpy, the status a session stores on every path that optimises an agent, no perturbation of a run, the
decisions forced branch by branch through parameters, and the run loop that follows them against the same loop made of
the C entries."""
import os
import subprocess

import numpy as np
import pytest

import common
import team_rules_ref as ref

pytestmark = pytest.mark.gpu

GNC = dict(GNCBarc=10.0, GNCMuStep=2.0)  # as tests/test_gnc_session_gpu.py
R, RANK = 5, 5
# at most 16 squares summed in index order and one square root: about 18 roundings of 2^-53 (2e-15), FMA or not
RTOL = 1e-14


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    if dcora_amd.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return dcora_amd


def np_max_translation_distance(X, Y, d):
    D = np.asarray(X)[:, d::d + 1] - np.asarray(Y)[:, d::d + 1]
    s = np.zeros(D.shape[1])
    for k in range(D.shape[0]):  # the squares in index order
        s += D[k] * D[k]
    return np.sqrt(s)


def _close(got, want):
    assert want > 0 and abs(got - want) <= RTOL * want, (got, want)


def _start(da, ds, r=RANK, seed=3):
    return common.random_point(r, ds.d, ds.n, seed, da.manifold_project)


def _with_outliers(da, base, n_out=12, seed=2):
    # (as tests/test_gnc_session_gpu.py)
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
    return da.Dataset(d, n, np.vstack(ids), np.vstack(vals))


def _robust_session(da, cost="GNC_TLS", chordal=False, **team):
    """smallGrid3D + 12 outliers; the start point is a random one, or the clean graph's chordal initialisation"""
    from dcora_amd import robust as rb
    clean = common.product_dataset("smallGrid3D")
    ds = _with_outliers(da, clean)
    kw = dict(GNC) if cost == "GNC_TLS" else {}
    s = da.RbcdSession(ds, num_robots=R, r=RANK, robust=rb.RobustCostParameters(cost, **kw))
    p = s.enable_team(**team)
    if chordal:
        X0 = np.zeros((RANK, (ds.d + 1) * ds.n))
        X0[:ds.d] = da.chordal_initialization(clean)
    else:
        X0 = _start(da, ds)
    s.set_X(X0)
    return ds, s, p


# ---- 1. the kernel against numpy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,r", [(2, 2), (3, 3), (3, 5), (3, 7), (3, 16)])
def test_kernel_equals_numpy_on_planted_maxima(da, d, r):
    rng = np.random.default_rng(100 * d + r)
    for n in (1, 25, 65, 1025, 2500):
        X = rng.standard_normal((r, (d + 1) * n))
        base = X + 1e-3 * rng.standard_normal(X.shape)
        for pos in sorted({0, n - 1} | {p for p in (63, 64, 65, 255, 256, 1024) if p < n}):
            Y = base.copy()
            Y[:, (d + 1) * pos + d] += 3.0 + rng.uniform(0, 1, r)  # the translation of pose `pos` moves furthest
            Y[:, (d + 1) * pos] += 50.0                            # a rotation column never counts
            per_pose = np_max_translation_distance(X, Y, d)
            assert int(np.argmax(per_pose)) == pos
            got = da.max_translation_distance(X, Y, d)
            _close(got, per_pose.max())
            assert da.max_translation_distance(X, Y, d) == got  # the same bits on the same input
    assert da.max_translation_distance(X, X, d) == 0.0


# ---- 2. the status a session stores ---------------------------------------------------------------------------------
def _check_round(da, s, p, sel, rnd, step, seen, robust=False):
    """step() runs one round in which agent(s) `sel` optimise; their status against numpy on agent_get_X before/after"""
    sel = list(np.atleast_1d(sel))
    before = {q: s.agent_get_X(q) for q in sel}
    step()
    d = s.ds.d
    for q in sel:
        st = s.agent_status(q)
        assert st is not None
        _close(st["relative_change"], np_max_translation_distance(s.agent_get_X(q), before[q], d).max())
        assert st["agent_id"] == q and st["state"] == ref.INITIALIZED and st["instance_number"] == 0
        assert st["iteration_number"] == rnd == s.agent_info(q)["iteration_number"]
        c = s.loop_closure_stats(q)
        assert bool(st["ready_to_terminate"]) == ref.ready_to_terminate(
            p, robust, 0, True, st["relative_change"], c["accepted"], c["rejected"], c["total"])
        seen.add(q)
    for q in range(s.R):
        assert (s.agent_status(q) is not None) == (q in seen)


def test_status_on_the_session_loop_across_a_restart(da):
    ds = common.product_dataset("smallGrid3D")
    s = da.RbcdSession(ds, num_robots=R, r=RANK, acceleration=True, restart_interval=30)
    p = s.enable_team()
    s.set_X(_start(da, ds))
    seen = set()
    for it in range(35):  # the restart step of round 30 included
        _check_round(da, s, p, it % R, it + 1, lambda: s.iterate(it % R), seen)
    s.close()


def test_status_on_one_tick_of_a_colour(da):
    ds = common.product_dataset("smallGrid3D")
    s = da.RbcdSession(ds, num_robots=R, r=RANK, acceleration=False)
    p = s.enable_team()
    s.set_X(_start(da, ds))
    col, nc = s.colours()
    sets = [np.nonzero(col == c)[0] for c in range(nc)]
    big = max(sets, key=len)
    assert len(big) >= 2, "smallGrid3D / 5 agents has a colour of several agents"
    seen = set()
    _check_round(da, s, p, big, 1, lambda: s.iterate_set(big), seen)
    _check_round(da, s, p, big, 2, lambda: s.iterate_set(big), seen)
    s.close()


@pytest.mark.parametrize("accel", [True, False])
def test_status_on_the_per_agent_calls(da, accel):
    ds = common.product_dataset("smallGrid3D")
    s = da.RbcdSession(ds, num_robots=R, r=RANK, acceleration=accel)
    p = s.enable_team()
    s.set_X(_start(da, ds))
    seen = set()

    def step(sel):
        for q in [q for q in range(R) if q != sel] + [sel]:
            s.agent_iterate(q, q == sel)

    for it in range(7):
        _check_round(da, s, p, it % R, it + 1, lambda: step(it % R), seen)
    s.close()


def test_status_with_more_poses_than_one_pass_of_a_workgroup(da):
    ds = common.product_dataset("sphere2500")  # 500 poses per agent, 256 threads per workgroup
    s = da.RbcdSession(ds, num_robots=R, r=RANK)
    p = s.enable_team()
    s.set_X(_start(da, ds))
    seen = set()
    for it in range(3):
        _check_round(da, s, p, it, it + 1, lambda: s.iterate(it), seen)
    s.close()


# ---- 3. no perturbation ---------------------------------------------------------------------------------------------
def test_an_enabled_session_runs_the_same_bits(da):
    ds = common.product_dataset("smallGrid3D")
    X0 = _start(da, ds)
    outs, Xs = [], []
    for enabled in (False, True):
        s = da.RbcdSession(ds, num_robots=R, r=RANK)
        if enabled:
            s.enable_team()
        s.set_X(X0)
        outs.append(s.run(max_iters=35, rgrad_tol=0.0))
        Xs.append(s.get_X())
        if enabled:
            assert any(s.agent_status(q) is not None for q in range(R))
        s.close()
    for key in ("selected", "cost", "gradnorm"):
        assert np.array_equal(outs[0][key], outs[1][key]), key
    assert np.array_equal(Xs[0], Xs[1])


# ---- 4. decisions, forced by parameters and not by data -------------------------------------------------------------
def test_l2_termination_by_readiness_and_by_the_iteration_cap(da):
    ds = common.product_dataset("smallGrid3D")
    X0 = _start(da, ds)
    s = da.RbcdSession(ds, num_robots=R, r=RANK)
    s.enable_team(rel_change_tol=1e9)  # every optimised agent is ready (its loop closures all carry weight 1)
    s.set_X(X0)
    assert not s.should_terminate() and not s.should_update_weights()
    order = [3, 3, 0, 1, 0, 4, 2, 2]  # the fifth distinct agent optimises in round 7
    for it, sel in enumerate(order):
        s.iterate(sel)
        assert s.should_terminate() == (it + 1 >= 7), it
        assert not s.should_update_weights()  # L2: never
    s.enable_team(rel_change_tol=0.0, max_num_iters=7)  # nobody is ever ready: only the cap ends the run
    s.set_X(X0)
    for it in range(9):
        s.iterate(it % R)
        assert s.should_terminate() == (it + 1 >= 7), it
        assert all(not s.agent_status(q)["ready_to_terminate"] for q in range(min(it + 1, R)))
    s.close()


def test_the_inner_iteration_cap_fires_the_weight_update(da):
    ds, s, p = _robust_session(da, robust_opt_inner_iters=3)
    assert s.team_info() == dict(inner_iter=0, latest_weight_update_iteration=0, weight_updates=0, resets=0)
    for it in range(3):  # the other agents never get a status: only the cap can fire
        s.iterate(2)
        assert s.team_info()["inner_iter"] == it + 1
        assert s.should_update_weights() == (it + 1 >= 3), it
        assert not s.should_terminate()
    assert [s.agent_status(q) is not None for q in range(R)] == [False, False, True, False, False]
    s.close()


def test_update_weights_clears_the_statuses_and_the_rules_follow_the_update_count(da):
    ds, s, p = _robust_session(da, rel_change_tol=1e9, robust_opt_min_convergence_ratio=0.0,
                               robust_opt_inner_iters=1000, robust_opt_num_weight_updates=2)
    rnd = 0
    for updates in (0, 1, 2):
        if updates:
            s.update_weights()
            # (c) the bookkeeping of ref src/Agent.cpp:1417-1424
            assert all(s.agent_status(q) is None for q in range(R))
            assert s.team_info() == dict(inner_iter=0, latest_weight_update_iteration=rnd, weight_updates=updates,
                                         resets=0)
        for k, sel in enumerate([1, 3, 0, 3, 4, 2]):  # the fifth distinct agent optimises in the sixth round
            s.iterate(sel)
            rnd += 1
            all_in = k == 5
            if updates == 0:
                # before the first update the tolerance is the reference's 5, not the parameter: readiness is the
                # data's; only (e) is forced -- no termination below the number of updates
                assert not s.should_terminate()
                continue
            assert all(s.agent_status(q)["ready_to_terminate"] for q in (1, 3, 0, 3, 4, 2)[:k + 1])
            assert s.should_update_weights() == (all_in and updates < 2), (updates, k)  # (c)
            assert s.should_terminate() == (all_in and updates >= 2), (updates, k)      # (e)
            assert s.team_info()["inner_iter"] == k + 1
    s.close()


def test_an_undecided_shared_closure_holds_back_exactly_its_two_agents(da):
    from dcora_amd import driver
    # (the L2 cost in a session with robust state: set_weights works, and the tolerance is the parameter throughout)
    ds, s, p = _robust_session(da, cost="L2", rel_change_tol=1e9, robust_opt_min_convergence_ratio=1.0)
    per = ds.n // R
    rob = np.minimum(ds.ids[:, [1, 3]] // per, R - 1)
    lc = driver.loop_closure_mask(ds, R)
    shared = np.nonzero(lc & (rob[:, 0] != rob[:, 1]))[0]
    e = int(shared[len(shared) // 2])
    touched = set(int(q) for q in rob[e])
    assert len(touched) == 2

    def stats_np(w):
        out = []
        for q in range(R):
            mine = lc & ((rob[:, 0] == q) | (rob[:, 1] == q))
            out.append(dict(accepted=int(np.sum(w[mine] == 1)), rejected=int(np.sum(w[mine] == 0)),
                            total=int(mine.sum())))
        return out

    assert [s.loop_closure_stats(q) for q in range(R)] == stats_np(s.get_weights())
    for q in range(R):
        s.iterate(q)
    assert all(s.agent_status(q)["ready_to_terminate"] for q in range(R)) and s.should_terminate()
    w = s.get_weights()
    w[e] = 0.5
    w[int(np.nonzero(lc)[0][0])] = 0.0  # a rejected closure is a decided one: it holds nobody back
    s.set_weights(w)
    assert [s.loop_closure_stats(q) for q in range(R)] == stats_np(s.get_weights())
    assert all(s.agent_status(q)["ready_to_terminate"] for q in range(R))  # setMeasurementWeight touches no status
    for q in range(R):
        s.iterate(q)
    assert {q for q in range(R) if not s.agent_status(q)["ready_to_terminate"]} == touched
    assert not s.should_terminate()
    s.close()


# ---- 5. the run loop ------------------------------------------------------------------------------------------------
def test_run_team_is_the_callers_loop_over_the_entries(da):
    team = dict(max_num_iters=120, robust_opt_num_weight_updates=4, robust_opt_inner_iters=10)
    dsA, A, p = _robust_session(da, chordal=True, **team)
    dsB, B, _ = _robust_session(da, chordal=True, **team)
    out = A.run_team()
    cost, gn, sel, upd = [], [], [], []
    selected = 0
    while True:
        statuses = [B.agent_status(q) for q in range(R)]
        info, rnd = B.team_info(), B.agent_info(0)["iteration_number"]
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
        assert A.agent_info(0)["iteration_number"] == p.max_num_iters
    else:
        assert out["stop_reason"] == "all_ready" and A.agent_info(0)["iteration_number"] < p.max_num_iters
        assert all(st is not None and st["ready_to_terminate"] for st in final)
        assert out["weight_updates"] == p.robust_opt_num_weight_updates
    A.close()
    B.close()


def test_the_team_driver_runs_the_robust_flow_by_the_rules(da):
    from dcora_amd import driver
    from dcora_amd import robust as rb
    clean = common.product_dataset("smallGrid3D")
    ds = _with_outliers(da, clean)
    T = da.chordal_initialization(clean)
    X0 = np.zeros((RANK, (clean.d + 1) * clean.n))
    X0[:clean.d] = T
    team = da.team_params(robust_opt_num_weight_updates=20, max_num_iters=1000)
    out = driver.multi_robot_team_session(ds, X0, num_robots=R, r=RANK, robust=rb.RobustCostParameters("GNC_TLS", **GNC),
                                          team=team)
    assert np.array_equal(ds.vals[:, -1], out["weights"])
    # every update comes after at most robust_opt_inner_iters rounds: all 20 are made well before the cap
    assert out["final"]["weight_updates"] == 20 and out["final"]["iterations"] <= 1000
    lc, w, m0 = out["loop_closures"], out["weights"], clean.m
    assert np.all(w[~lc] == 1.0)
    assert np.all(w[m0:] < 1e-8), "every injected closure is rejected"
    assert np.all(w[:m0][lc[:m0]] > 1 - 1e-8), "every original closure is kept"
    if out["final"]["stop_reason"] == "all_ready":
        assert all(st["ready_to_terminate"] for st in out["statuses"])


# ---- 6. refusals ----------------------------------------------------------------------------------------------------
def test_refusals(da):
    from dcora_amd import capi
    ds = common.product_dataset("smallGrid3D")
    s = da.RbcdSession(ds, num_robots=R, r=RANK)
    s.team = da.team_params()
    for call in (lambda: s.agent_status(0), lambda: s.loop_closure_stats(0), s.should_terminate,
                 s.should_update_weights, s.team_info, s.run_team):
        with pytest.raises(capi.DcoraError) as e:
            call()
        assert e.value.status == 1  # DCORA_ERR_BAD_ARG
    s.enable_team()
    with pytest.raises(capi.DcoraError) as e:
        s.agent_status(R)
    assert e.value.status == 1
    s.close()
    ranked = da.RbcdSession(ds, num_robots=R, r=RANK, rank=0, world_size=2)
    with pytest.raises(capi.DcoraError) as e:
        ranked.enable_team()
    assert e.value.status == 8  # DCORA_ERR_UNSUPPORTED
    ranked.close()


# ---- the facade -----------------------------------------------------------------------------------------------------
def test_cpp_agent_status_facade(built):
    """DCORA::Agent::getStatus / shouldTerminate / shouldUpdateMeasurementWeights / hasNeighborStatus / getNeighborStatus
    (dcora_amd/include/DCORA/Agent.h) over the session's status and dcora_team_decide"""
    exe = os.path.join(common.HERE, "cpp", "_build", "test_agent_status_facade")
    assert os.path.exists(exe), "build() compiles tests/cpp/test_agent_status_facade.cpp"
    p = subprocess.run([exe, common.plain_path("smallGrid3D")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
