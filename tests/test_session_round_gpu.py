"""Rounding of a live RBCD session on the device (dcora_rbcd_round / dcora_ra_rbcd_round: k_round_states, k_round_points,
SessionCore::round; ref examples/MultiRobotExample.cpp:341-347, src/Agent.cpp:1014-1033) and the rounded cost through
the central problem's own evaluation.

The rule for rotations is tests/test_block_factors_gpu.py's: per group, device error <= 8 max(oracle_err_g, eps cond_g),
orthogonality <= 8 oracle_orth; translations, unit spheres and landmarks <= 8 eps (|p| + |p_anchor|) per column against
longdouble (tests/session_round_inputs.py, whose inputs and references tests/test_session_round_cpu.py checks).  The
rounded cost is held to 8 (max row nnz + r) eps sum |Z| |Q| |Z^T| against longdouble <Z Q, Z> of the RETURNED states.
Anchor forms, repeated calls and the session's next iterates are compared bit for bit.

Largest device error / max(oracle_err_g, eps cond_g) observed on an MI355X (bound: 8):
  fixture blocks  1.58 (d=2 r=5 det>0, close pair), 1.41 at r = d (d=2, det<0, sigma_min=1e-9); orthogonality 1.01 x
                  oracle_orth at most (bound: 8); exact rank d-1 blocks: error 0
  sizes           1.75 against longdouble (d=3 r=5); against the host-fed k_align_poses every rotation block is
                  bit-equal (hipcc contracts that kernel's sums into the same fma chain); translations 0.17 of their
                  bound at most
  range-aided     rotations below 0.005 (the fixtures' iterates from the odometry start keep exact rotations),
                  translations 0.03, unit spheres and landmarks 0.04 of their bounds at most
  rounded cost    |device - longdouble| <= 0.0018 bounds (range_aided_slam_test_3d), 0.0017 on smallGrid3D; the cost at
                  rotated instead of normalised sphere columns lies 5.4e11 bounds away on the random iterates
  driver          trajectory bit-equal to the host-fed rounding of the returned X; rounded 2f 1025.39805 against the
                  relaxation's 1025.40114 with a gap of 0.563 (smallGrid3D, r_min = 3)
"""
import numpy as np
import pytest

import block_factors as bf
import common
import session_round_inputs as sri
from test_raslam import ra_path

pytestmark = pytest.mark.gpu

EPS = bf.EPS
UNSUPPORTED, BAD_ARG = 8, 1
GNC = dict(GNCBarc=10.0, GNCMuStep=2.0)
RA_NAMES = ["range_aided_slam_test_2d", "range_aided_slam_test_3d"]


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


def _chain_session(da, d, r, n, X, robots=None):
    ds = sri.chain_dataset(da.Dataset, d, n, sri.seed_of(d, r, n))
    s = da.RbcdSession(ds, num_robots=sri.robots_of(n) if robots is None else robots, r=r)
    s.set_X(X)
    return s


def _status(call):
    from dcora_amd import capi
    with pytest.raises(capi.DcoraError) as e:
        call()
    return e.value.status


# ---- a. the fixture's blocks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,r", bf.SO_DR)
def test_fixture_blocks_through_a_session(env, d, r):
    """both determinant signs, sigma_min down to 1e-9, the close pair and (r = d) the exact rank d - 1 blocks, as the
    poses of a chain of two agents, against the explicit anchor [R0 | 0]"""
    da, _ = env
    fx = bf.load()
    groups = bf.so_groups(fx, d, r)
    Yin = np.concatenate([g.inp for g in groups])
    nb = len(Yin)
    T = 10 * np.random.default_rng(60 + r * 10 + d).standard_normal((r, nb))
    anchor = bf.so_anchor(fx, d, r)
    X = bf.se_matrix(Yin, T)
    s = _chain_session(da, d, r, nb, X, robots=2)
    out = s.round(anchor=anchor)["trajectory"]
    s.close()
    assert out.shape == (d, (d + 1) * nb)
    R, t = sri.traj_blocks(out, d)
    if r == d:
        assert np.array_equal(t, T)  # R0 = I, t0 = 0: every sum is one term and zeros
    _, t_ref = sri.frame_blocks_ld(X, anchor, d)
    assert (np.abs(t - t_ref).max(axis=0) <= sri.translation_bound(X, anchor, d)).all()
    assert (np.linalg.det(R) > 1 - 64 * EPS).all(), np.linalg.det(R).min()
    rows = [(g.name, err, g.tol()) for g, err in bf.so_group_errors(groups, R)]
    for name, err, tol in rows:
        print("k_round_states %-34s device %.3e  oracle-or-eps-cond %.3e  ratio %.2f" % (name, err, tol, err / tol))
    orth = float(bf.orth_err(R).max())
    worst = max(rows, key=lambda x: x[1] / x[2])
    print("RATIO k_round_states fixture d=%d r=%d max %.2f (%s); orthogonality %.2f x oracle_orth" %
          (d, r, worst[1] / worst[2], worst[0], orth / float(fx["oracle_orth"])))
    assert all(err <= 8 * tol for _, err, tol in rows), [x for x in rows if not x[1] <= 8 * x[2]]
    assert orth <= 8 * float(fx["oracle_orth"])


# ---- b. sizes, c. anchor forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,r", [(d, r) for d in sri.DIMS for r in sri.ranks_of(d)])
def test_sizes_where_the_lane_map_can_go_wrong(env, d, r):
    """n around the 16 poses of a wave and the 64 of a workgroup, one agent to three, anchor 0 and n - 1: against numpy
    longdouble and against the host-fed rounding of get_X(); the anchor named equals the anchor passed, and two calls
    agree, bit for bit"""
    da, _ = env
    fx = bf.load()
    worst = dict(ld=0.0, host=0.0, t=0.0)
    for n in sri.SIZES:
        X = sri.lifted_point(d, r, n, sri.seed_of(d, r, n))
        s = _chain_session(da, d, r, n, X)
        Xs = s.get_X()
        assert np.array_equal(Xs, X)
        for j in sorted({0, n - 1}):
            anchor = sri.anchor_of(X, d, j)
            out = s.round(anchor_pose=j)["trajectory"]
            assert np.array_equal(out, s.round(anchor_pose=j)["trajectory"]), (n, j)      # c. two calls
            assert np.array_equal(out, s.round(anchor=anchor)["trajectory"]), (n, j)      # c. named == passed
            ref, t_ref = sri.round_reference(X, anchor, d)
            tol = sri.oracle_tolerance(X, anchor, d)
            R, t = sri.traj_blocks(out, d)
            e_ld = float(bf.block_err(R.astype(sri.LD), ref).max())
            host = da.align_lifted_trajectory_to_frame(Xs, anchor, d, n, True)
            e_host = float(bf.block_err(R, sri.traj_blocks(host, d)[0]).max())
            tb = sri.translation_bound(X, anchor, d)
            e_t = float((np.abs(t - t_ref).max(axis=0) / tb).max())
            print("k_round_states d=%d r=%d n=%d anchor %d: vs longdouble %.2f, vs host-fed %.2f (x tol %.2e); "
                  "translations %.2f of their bound" % (d, r, n, j, e_ld / tol, e_host / tol, tol, e_t))
            worst = dict(ld=max(worst["ld"], e_ld / tol), host=max(worst["host"], e_host / tol), t=max(worst["t"], e_t))
            assert e_ld <= 8 * tol and e_host <= 8 * tol, (n, j, e_ld, e_host, tol)
            assert e_t <= 1, (n, j, e_t)
            assert float(bf.orth_err(R).max()) <= 8 * float(fx["oracle_orth"])
            assert (np.linalg.det(R) > 1 - 64 * EPS).all()
        s.close()
    print("RATIO k_round_states sizes d=%d r=%d: %.2f vs longdouble, %.2f vs host-fed, translations %.2f" %
          (d, r, worst["ld"], worst["host"], worst["t"]))


# ---- d. range-aided ----------------------------------------------------------------------------------------------------------
def _ra_session(da, ra, r, X0, iters=3, **kw):
    s = da.RaRbcdSession(ra, r, **kw)
    s.set_X(X0)
    if iters:
        s.run(max_iters=iters, rgrad_tol=0.0)
    return s


def _odometry_start(ra, r):
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    return X0


def _ra_cost_check(s, ra, Q, out, label):
    """f. <Z Q, Z> of the returned states (sphere columns normalised) against the device's 2 f -> (error / bound,
    |cost with rotated spheres - device| / bound)"""
    d, n = ra.d, ra.n
    T, S, Lm = out["trajectory"], out["unit_spheres"], out["landmarks"]
    ref, bound = sri.cost_reference(sri.ra_point(T, S, Lm, d, n, True), Q, s.r)
    rot, _ = sri.cost_reference(sri.ra_point(T, S, Lm, d, n, False), Q, s.r)
    err, gap = abs(float(ref) - out["cost_2f"]) / float(bound), abs(float(rot) - out["cost_2f"]) / float(bound)
    print("rounded cost %s: device %.12g longdouble %.12g bound %.3e: error %.4f bounds; rotated spheres %.3g bounds away"
          % (label, out["cost_2f"], float(ref), float(bound), err, gap))
    assert err <= 1, (label, out["cost_2f"], float(ref), float(bound))
    assert np.isfinite(out["gradnorm"]) and out["gradnorm"] >= 0
    return err, gap


@pytest.mark.parametrize("name", RA_NAMES)
def test_range_aided_states_and_the_point_behind_the_cost(env, name):
    da, orc = env
    fx = bf.load()
    ra = da.RADataset(ra_path(name))
    d, n, l, b, r = ra.d, ra.n, ra.l, ra.b, ra.d + 2
    Q = ra.Q.to_scipy()
    # the states: 3 iterations from the odometry start
    s = _ra_session(da, ra, r, _odometry_start(ra, r))
    X = s.get_X()
    Xse = sri.se_from_ra(X, d, n, l)
    for j in (0, n - 1):
        anchor = sri.anchor_of(Xse, d, j)
        out = s.round(anchor_pose=j, cost=True)
        again = s.round(anchor=anchor, cost=True)
        for key in ("trajectory", "unit_spheres", "landmarks"):
            assert np.array_equal(out[key], again[key]), (key, j)
        assert out["cost_2f"] == again["cost_2f"]
        ref, t_ref = sri.round_reference(Xse, anchor, d)
        tol = sri.oracle_tolerance(Xse, anchor, d)
        R, t = sri.traj_blocks(out["trajectory"], d)
        ratio = float(bf.block_err(R.astype(sri.LD), ref).max()) / tol
        pa = np.linalg.norm(anchor[:, d])
        e_t = float((np.abs(t - t_ref).max(axis=0) / sri.translation_bound(Xse, anchor, d)).max())
        Sx, Lx = X[:, d * n:d * n + l], X[:, d * n + l + n:]
        e_s = np.abs(out["unit_spheres"] - sri.points_reference(Sx, anchor, d, False)).max(axis=0) / \
            (8 * EPS * np.linalg.norm(Sx, axis=0))
        e_l = np.abs(out["landmarks"] - sri.points_reference(Lx, anchor, d, True)).max(axis=0) / \
            (8 * EPS * (np.linalg.norm(Lx, axis=0) + pa))
        e_p = float(max(e_s.max() if l else 0, e_l.max() if b else 0))
        print("RATIO k_round_states %s anchor %d: rotations %.2f (x tol %.2e), translations %.2f, spheres / landmarks "
              "%.2f of their bounds" % (name, j, ratio, tol, e_t, e_p))
        assert ratio <= 8 and e_t <= 1 and e_p <= 1
        assert float(bf.orth_err(R).max()) <= 8 * float(fx["oracle_orth"])
        _ra_cost_check(s, ra, Q, out, "%s odometry iterate, anchor %d" % (name, j))
    s.close()
    # the point behind the cost has unit sphere columns: an iterate off the rank-d subspace (3 iterations from a random
    # point; from [X_odom; 0] every R0^T s is a unit vector already), where the two readings are far apart
    rng = np.random.default_rng(4)
    X0 = orc.project_to_manifold(r, d, n, rng.uniform(-1, 1, (r, ra.k)), l=l, b=b)
    s = _ra_session(da, ra, r, X0)
    out = s.round(cost=True)
    s.close()
    assert l > 0 and np.abs(np.linalg.norm(out["unit_spheres"], axis=0) - 1).max() > 1e-3  # returned: rotated only
    _, gap = _ra_cost_check(s, ra, Q, out, "%s random iterate" % name)
    assert gap > 1, "the cost at rotated sphere columns must lie outside the bound"


# ---- e. the session is left as it was -------------------------------------------------------------------------------------
def _next_iterates(s, before):
    before(s)
    g = s.run(max_iters=5, rgrad_tol=0.0)
    X = s.get_X()
    s.close()
    return X, g["cost"], g["gradnorm"], g["selected"]


@pytest.mark.parametrize("kind", ["pgo", "ra"])
def test_a_run_after_round_equals_the_run_without_it(env, kind):
    da, orc = env
    if kind == "pgo":
        ds = common.product_dataset("smallGrid3D")
        X0 = common.random_point(5, ds.d, ds.n, 4, orc.project_to_manifold)
        make = lambda: da.RbcdSession(ds, num_robots=5, r=5)
    else:
        ra = da.RADataset(ra_path(RA_NAMES[0]))
        X0 = _odometry_start(ra, ra.d + 2)
        make = lambda: da.RaRbcdSession(ra, ra.d + 2)

    def start(s, rounds):
        s.set_X(X0)
        s.run(max_iters=3, rgrad_tol=0.0)
        if rounds:
            s.round(cost=True)
            s.round(anchor_pose=1, anchor=None)
            s.round(anchor=np.eye(s.r, s._round_dims()[0] + 1))
    a = _next_iterates(make(), lambda s: start(s, True))
    b = _next_iterates(make(), lambda s: start(s, False))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- f. the rounded cost ------------------------------------------------------------------------------------------------
def test_rounded_cost_of_a_pose_graph_session_with_its_current_weights(env):
    """smallGrid3D, 5 agents, r = 5, robust: the cost on the creation weights (1 on every loop closure), then after
    set_weights with zeros and fractions -- each against longdouble <Z Q, Z> with the host Q of those weights"""
    da, orc = env
    from dcora_amd import driver, robust as rb
    ds = common.product_dataset("smallGrid3D")
    d, n, r = ds.d, ds.n, 5
    X0 = common.random_point(r, d, n, 4, orc.project_to_manifold)
    s = da.RbcdSession(da.Dataset(d, n, ds.ids.copy(), ds.vals.copy()), num_robots=5, r=r,
                       robust=rb.RobustCostParameters("GNC_TLS", **GNC))
    s.set_X(X0)
    s.run(max_iters=3, rgrad_tol=0.0)
    w1 = s.get_weights()
    lc = np.flatnonzero(driver.loop_closure_mask(ds, 5))
    w2 = w1.copy()
    w2[lc[::3]], w2[lc[1::3]] = 0.0, 0.3
    w2[lc[2::3]] = 0.7
    costs = []
    for label, w in (("creation weights", w1), ("zeros and fractions", w2)):
        if w is not w1:
            s.set_weights(w)
        out = s.round(cost=True)
        vals = ds.vals.copy()
        vals[:, -1] = w
        Q = da.build_Q_pgo(ds, vals=vals).to_scipy()
        ref, bound = sri.cost_reference(out["trajectory"], Q, r)
        err = abs(float(ref) - out["cost_2f"]) / float(bound)
        print("rounded cost smallGrid3D %s: device %.12g longdouble %.12g bound %.3e: error %.4f bounds; |rgrad| %.3g"
              % (label, out["cost_2f"], float(ref), float(bound), err, out["gradnorm"]))
        assert err <= 1
        costs.append(out["cost_2f"])
        # the evaluation is the central problem's own: the same call gives the same bits
        assert s.round(cost=True)["cost_2f"] == out["cost_2f"]
    s.close()
    assert costs[1] < costs[0]  # weights only went down


def test_rounded_cost_of_a_range_aided_session_with_its_current_weights(env):
    da, orc = env
    from dcora_amd import robust as rb
    name = RA_NAMES[0]
    ra = da.RADataset(ra_path(name))
    r = ra.d + 2
    rng = np.random.default_rng(4)
    X0 = orc.project_to_manifold(r, ra.d, ra.n, rng.uniform(-1, 1, (r, ra.k)), l=ra.l, b=ra.b)
    s = _ra_session(da, ra, r, X0, robust=rb.RobustCostParameters("GNC_TLS", **GNC))
    w1 = s.get_weights()
    lc = np.flatnonzero(ra.loop_closures())
    assert lc.size >= 1
    w2 = w1.copy()
    w2[lc[::2]], w2[lc[1::2]] = 0.0, 0.4
    for label, w in (("creation weights", w1), ("zeros and fractions", w2)):
        host = da.RADataset(ra_path(name))
        host.set_pose_pose_weights(w)
        if w is not w1:
            s.set_weights(w)
        _ra_cost_check(s, ra, host.Q.to_scipy(), s.round(cost=True), "%s %s" % (name, label))
    s.close()


# ---- g. refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pgo", "ra"])
def test_refusals_leave_the_session_as_it_was(env, kind):
    da, orc = env
    from dcora_amd import capi
    import ctypes as C
    if kind == "pgo":
        ds = common.product_dataset("smallGrid3D")
        d, n, r = ds.d, ds.n, 5
        X0 = common.random_point(r, d, n, 4, orc.project_to_manifold)
        make = lambda **kw: da.RbcdSession(ds, num_robots=5, r=r, **kw)
    else:
        ra = da.RADataset(ra_path(RA_NAMES[0]))
        d, n, r = ra.d, ra.n, ra.d + 2
        X0 = _odometry_start(ra, r)
        make = lambda **kw: da.RaRbcdSession(ra, r, **kw)

    def start(s, calls):
        s.set_X(X0)
        s.run(max_iters=3, rgrad_tol=0.0)
        calls(s)

    def refused(s):
        bad = np.eye(r, d + 1)
        for v in (np.nan, np.inf):
            bad[r - 1, d] = v
            assert _status(lambda: s.round(anchor=bad)) == BAD_ARG
        bad = np.eye(r, d + 1)
        bad[0, 0] = -np.inf
        assert _status(lambda: s.round(anchor=bad, cost=True)) == BAD_ARG
        for j in (-1, n, n + 7):
            assert _status(lambda: s.round(anchor_pose=j)) == BAD_ARG
        # trajectory NULL, through the C entry
        extra = (None, None) if kind == "ra" else ()
        rc = getattr(capi.lib(), s._prefix + "round")(s.h, 0, None, None, *extra, None, None)
        assert rc == BAD_ARG
    a = _next_iterates(make(), lambda s: start(s, refused))
    b = _next_iterates(make(), lambda s: start(s, lambda s: None))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # a rank of a job rounds through its exchange
    s = make(rank=0, world_size=2)
    s.set_X(X0)
    assert _status(lambda: s.round()) == UNSUPPORTED
    assert _status(lambda: s.round(anchor=np.eye(r, d + 1), cost=True)) == UNSUPPORTED
    s.close()


# ---- h. the driver -----------------------------------------------------------------------------------------------------------
PARENT_KEYS = {"X", "rank", "certified", "theta", "total_iters", "suboptimality_gap_f", "levels", "cost", "gradnorm",
               "selected", "rank_trace"}


def test_staircase_driver_rounds_on_the_device(env):
    da, orc = env
    from dcora_amd import driver
    fx = bf.load()
    ds = common.product_dataset("smallGrid3D")
    d, n = ds.d, ds.n
    X0 = common.random_point(3, d, n, 4, orc.project_to_manifold)
    kw = dict(num_robots=5, r_min=3, r_max=9, max_iters=400, rgrad_tol=0.05)
    plain = driver.multi_robot_staircase_session(ds, X0, **kw)
    res = driver.multi_robot_staircase_session(ds, X0, round_on_device=True, **kw)
    assert set(plain) == PARENT_KEYS
    assert set(res) == PARENT_KEYS | {"trajectory", "rounded_cost_2f", "rounded_gradnorm"}
    for key in ("X", "cost", "gradnorm", "selected", "rank_trace"):
        assert np.array_equal(plain[key], res[key]), key
    assert (plain["rank"], plain["certified"], plain["total_iters"]) == (res["rank"], res["certified"], res["total_iters"])
    X = res["X"]
    anchor = sri.anchor_of(X, d, 0)
    host = da.align_lifted_trajectory_to_frame(X, anchor, d, n, True)
    tol = sri.oracle_tolerance(X, anchor, d)
    R, t = sri.traj_blocks(res["trajectory"], d)
    Rh, th = sri.traj_blocks(host, d)
    e = float(bf.block_err(R, Rh).max())
    print("driver: trajectory vs host-fed rounding of the returned X %.2f x tol (%.2e); rounded 2f %.9g, relaxation 2f "
          "%.9g, gap f %.3g, |rgrad| at the rounded point %.3g" %
          (e / tol, tol, res["rounded_cost_2f"], res["levels"][-1]["cost_2f"], res["suboptimality_gap_f"],
           res["rounded_gradnorm"]))
    assert e <= 8 * tol
    assert (np.abs(t - th).max(axis=0) <= 2 * sri.translation_bound(X, anchor, d)).all()
    assert float(bf.orth_err(R).max()) <= 8 * float(fx["oracle_orth"])
    assert res["certified"]
    # the relaxation's bound: f_rounded >= f* >= f_relaxed - gap
    assert res["rounded_cost_2f"] >= res["levels"][-1]["cost_2f"] - 2 * res["suboptimality_gap_f"]
    # ... and the rounded cost is the cost of the returned trajectory
    ref, bound = sri.cost_reference(res["trajectory"], da.build_Q_pgo(ds).to_scipy(), res["rank"])
    assert abs(float(ref) - res["rounded_cost_2f"]) <= float(bound)
