"""Projection of a live RBCD session to rank d on the device, in place (dcora_rbcd_project / dcora_ra_rbcd_project:
k_gram_mfma, k_gram_finish, k_project_dets, k_project_states, k_project_points, SessionCore::project; ref
examples/SingleRobotExample_RASLAM.cpp:220-234, projectSolutionRASLAM src/DCORA_utils.cpp:1984-2031).

Inputs and references: tests/session_project_inputs.py, checked on the CPU by tests/test_session_project_cpu.py.
Rules:
  gram      |gram - G_ld|_ab <= (k + 2) eps (|X| |X|^T)_ab, symmetric and repeatable bit for bit;
  sigma^2   against float64 eigvalsh(G_ld): |B|_F (B the matrix of the Gram bounds; Weyl) + 8 max(dist, r eps lambda_1),
            dist the distance between two references on the same matrix, eigvalsh(G_ld) and the squares of numpy's
            float64 SVD of X (the CPU oracle exports no SVD of its own); basis^T basis = I and
            |G basis - basis diag(sigma^2)| under the same rule (relative to lambda_1 for the former);
  point     P^T P against the host-fed dcora_round_project_solution_raslam within 1e-10 (the bound of
            tests/test_block_factors_gpu.py section e); get_X() against Proj(basis^T X) recomputed from the returned
            basis: rotations by the block rule of tests/session_round_inputs.py with [basis | 0] in the anchor's place
            (8 max(oracle error, eps cond)), every other column within 8 r eps |basis|^T |x|;
  sessions  a projected session against a fresh rank-d session handed the same point: bit for bit.
One pose (n / 2 == 0) never reflects: a truncation the eigensolver returned left-handed is projected as it stands, so
the comparison with the host-fed path is left out there (the band tests/test_block_factors_gpu.py leaves out).

Largest ratios observed on an MI355X (each of its bound; rotations: bound 8):
  gram           0.200 at the chunk edges (host arrays), 0.161 through sessions (d=2 r=16), 0.037 range-aided
  sigma^2        0.146 (d=3 r=16); basis orthogonality 0.219 (d=2 r=16); residual 0.299 (d=3 r=16)
  point          rotations 1.54 against longdouble (d=3 r=16), 0.87 range-aided; translations 0.028, unit spheres 0.019;
                 |P^T P - host-fed| 2.9e-15 on the sizes, 2.7e-15 range-aided (bound 1e-10)
  reflect        the expected branch within 8.9e-15, the other one at least 3.6 away
  driver         range_aided_slam_test_3d: sigma 6.155 4.738 3.436 | 0.928, projected 2f 0.0080 refined to 3.8e-07 in 14
                 iterations; smallGrid3D: sigma 19.67 19.42 19.21 | 2.06, 2f 1025.3982 refined to 1025.39809 in 9
"""
import ctypes as C

import numpy as np
import pytest

import block_factors as bf
import common
import ra_loops
import session_project_inputs as spi
import session_round_inputs as sri
from test_raslam import ra_path

pytestmark = pytest.mark.gpu

EPS = bf.EPS
LD = np.longdouble
UNSUPPORTED = 8
ETA = 1e-3
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


def _debug_gram(X):
    from dcora_amd import capi
    r, k = X.shape
    G, chunk = np.zeros(r * r), C.c_int()
    capi.check(capi.lib().dcora_debug_project_gram(r, k, capi.F(X), G, C.byref(chunk)))
    return capi.unF(G, r, r), chunk.value


def _gram_chunk(da):
    return _debug_gram(np.ones((2, 3)))[1]


# ---- a. / b. the Gram matrix, its spectrum --------------------------------------------------------------------------------
def _check_gram(G, X, tag):
    ref, bound = spi.gram_ld(X), spi.gram_bound(X)
    assert np.isfinite(G).all(), tag
    assert np.array_equal(G, G.T), tag
    err = np.abs(G.astype(LD) - ref)
    assert (err <= bound).all(), (tag, float((err - bound).max()))  # (a zero row of X: bound 0, the entry exact)
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _check_spectrum(out, X, d, tag):
    """sigma (all r) and, where the session was projected, the basis -> the ratios observed"""
    r = X.shape[0]
    Gld = spi.gram_ld(X)
    w = np.linalg.eigvalsh(Gld.astype(np.float64))[::-1]
    sv = np.zeros(r)
    s = np.linalg.svd(X, compute_uv=False)
    sv[:len(s)] = s ** 2
    dist = float(np.abs(w - sv).max())
    jac = 8 * max(dist, r * EPS * w[0])
    weyl = float(np.linalg.norm(spi.gram_bound(X).astype(np.float64)))
    sig2 = out["sigma"] ** 2
    assert (np.diff(out["sigma"]) <= 0).all() and (out["sigma"] >= 0).all(), tag
    e_sig = float(np.abs(sig2 - np.maximum(w, 0)).max())
    ratios = [e_sig / (weyl + jac)]
    assert e_sig <= weyl + jac, (tag, e_sig, weyl, jac)
    if out["projected"]:
        B, G = out["basis"], out["gram"]
        e_orth = float(np.abs(B.T @ B - np.eye(d)).max())
        e_res = float(np.linalg.norm(G @ B - B * sig2[:d]))
        ratios += [e_orth / (jac / w[0]), e_res / jac]
        assert e_orth <= jac / w[0], (tag, e_orth, jac / w[0])
        assert e_res <= jac, (tag, e_res, jac)
    return ratios


@pytest.mark.parametrize("d", spi.DIMS)
def test_gram_kernel_at_the_edges_of_its_chunks(env, d):
    """the kernel pair on host arrays: k below 4, no multiple of 4, one below / at / one above a workgroup's chunk, two
    chunks and a remainder, for r in {d, 5, 16}; symmetric, NaN-free (every entry written), twice the same bits"""
    da, _ = env
    chunk = _gram_chunk(da)
    worst = 0.0
    for r in spi.ranks_of(d):
        for k in (1, 2, 3, 5, 7, chunk - 1, chunk, chunk + 1, 2 * chunk + 7):
            X = np.random.default_rng(1000 * r + k).standard_normal((r, k))
            G, _ = _debug_gram(X)
            worst = max(worst, _check_gram(G, X, (d, r, k)))
            assert np.array_equal(G, _debug_gram(X)[0]), (r, k)
    print("RATIO k_gram_mfma edges d=%d chunk %d: %.3f of the (k + 2) eps bound" % (d, chunk, worst))


@pytest.mark.parametrize("d,r", [(d, r) for d in spi.DIMS for r in spi.ranks_of(d)])
def test_sizes_gram_spectrum_and_projected_point(env, d, r):
    """a. - c. on pose-graph sessions with one to three agents: sri.SIZES at nu in {0, 1e-3}, and the pose counts that
    put k at the edges of the Gram kernel's chunks (nu = 1e-3)"""
    da, _ = env
    fx = bf.load()
    chunk = _gram_chunk(da)
    cases = [(n, nu) for n in spi.SIZES for nu in spi.NUS] + [(n, 1e-3) for n in spi.chunk_sizes(d, chunk)
                                                              if n not in spi.SIZES]
    worst = dict(gram=0.0, sigma=0.0, orth=0.0, res=0.0, host=0.0, rot=0.0, euc=0.0)
    for n, nu in cases:
        tag = (d, r, n, nu)
        X = spi.lifted_point(d, r, n, spi.seed_of(d, r, n, nu), nu)
        s = _chain_session(da, d, r, n, X)
        out = s.project()
        assert out["gram_chunk"] == chunk
        worst["gram"] = max(worst["gram"], _check_gram(out["gram"], X, tag))
        rat = _check_spectrum(out, X, d, tag)
        worst["sigma"] = max(worst["sigma"], rat[0])
        assert s.r == d and out["projected"] == (r > d), tag
        P = s.get_X()
        assert P.shape == (d, (d + 1) * n)
        if r == d:
            assert np.array_equal(P, X), tag
            s.close()
            continue
        worst["orth"], worst["res"] = max(worst["orth"], rat[1]), max(worst["res"], rat[2])
        # two sessions, the same X: the same bits
        if n in (17, 257):
            t = _chain_session(da, d, r, n, X)
            again = t.project()
            assert np.array_equal(again["gram"], out["gram"]) and np.array_equal(again["basis"], out["basis"])
            assert np.array_equal(t.get_X(), P)
            t.close()
        s.close()
        R = spi.rotation_blocks(P, d, n, 0, True)
        assert (np.linalg.det(R) > 1 - 64 * EPS).all(), (tag, np.linalg.det(R).min())
        assert float(bf.orth_err(R).max()) <= 8 * float(fx["oracle_orth"]), tag
        B = out["basis"]
        Xd = spi.truncate(X, B)
        npos_now = spi.positive_dets(Xd, d, n, 0, True)
        assert out["positive_dets"] in (0, n) and out["reflected"] == (out["positive_dets"] < n // 2), tag
        # get_X() is Proj(basis^T X)
        anchor = np.concatenate([B, np.zeros((r, 1))], axis=1)
        t_ref = (np.asarray(B, LD).T @ np.asarray(X[:, d::d + 1], LD))
        t_bound = 8 * r * EPS * (np.abs(B).T @ np.abs(X[:, d::d + 1]))
        e_t = float((np.abs(P[:, d::d + 1] - t_ref) / np.maximum(t_bound, 1e-300)).max())
        worst["euc"] = max(worst["euc"], e_t)
        assert e_t <= 1, (tag, e_t)
        if npos_now == n:
            ref, _ = sri.round_reference(X, anchor, d)
            tol = sri.oracle_tolerance(X, anchor, d)
            e_r = float(bf.block_err(R.astype(LD), ref).max()) / tol
            worst["rot"] = max(worst["rot"], e_r)
            assert e_r <= 8, (tag, e_r, tol)
        else:
            assert n // 2 == 0, tag  # (one pose, a left-handed truncation: projected as it stands)
        # gauge-invariant match with the host-fed path (the parent's, pinned to the oracle by tests/test_rounding.py)
        if n // 2 > 0:
            H = da.project_solution_raslam(spi.ra_from_se(X, d, n), r, d, n, 0, 0)
            Pr = spi.ra_from_se(P, d, n)
            e_h = float(np.abs(Pr.T @ Pr - H.T @ H).max())
            worst["host"] = max(worst["host"], e_h)
            assert e_h <= 1e-10, (tag, e_h)
    print("RATIO project sizes d=%d r=%d: gram %.3f, sigma^2 %.3f, basis orthogonality %.3f, residual %.3f of their "
          "bounds; rotations %.2f (bound 8), other columns %.3f; |P^T P - host-fed| %.2e (bound 1e-10)" %
          (d, r, worst["gram"], worst["sigma"], worst["orth"], worst["res"], worst["rot"], worst["euc"], worst["host"]))


# ---- c. range-aided --------------------------------------------------------------------------------------------------------
def _odometry_start(ra, r):
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    return X0


def _ra_session(da, ra, r, X0, iters=3, **kw):
    s = da.RaRbcdSession(ra, r, **kw)
    s.set_X(X0)
    if iters:
        s.run(max_iters=iters, rgrad_tol=0.0)
    return s


@pytest.mark.parametrize("name", RA_NAMES)
def test_range_aided_projected_point(env, name):
    da, _ = env
    fx = bf.load()
    ra = da.RADataset(ra_path(name))
    d, n, l, b, r = ra.d, ra.n, ra.l, ra.b, ra.d + 2
    s = _ra_session(da, ra, r, _odometry_start(ra, r))
    X = s.get_X()
    cost_before = s.evaluate()[0]
    assert spi.eig_gap(X, d) >= spi.GAP and spi.block_sigma_min(X, d, n, l, False) >= spi.BLOCK_SIGMA_MIN
    out = s.project()
    P = s.get_X()
    s.close()
    assert s.r == d and out["projected"] and P.shape == (d, ra.k)
    g = _check_gram(out["gram"], X, name)
    rat = _check_spectrum(out, X, d, name)
    R = spi.rotation_blocks(P, d, n, l, False)
    assert (np.linalg.det(R) > 1 - 64 * EPS).all()
    assert float(bf.orth_err(R).max()) <= 8 * float(fx["oracle_orth"])
    sph = P[:, d * n:d * n + l]
    assert np.abs(np.linalg.norm(sph, axis=0) - 1).max() <= 8 * EPS
    H = da.project_solution_raslam(X, r, d, n, l, b)
    e_h = float(np.abs(P.T @ P - H.T @ H).max())
    assert e_h <= 1e-10, e_h
    # get_X() is Proj(basis^T X)
    B = out["basis"]
    Xse, anchor = sri.se_from_ra(X, d, n, l), np.concatenate([B, np.zeros((r, 1))], axis=1)
    ref, _ = sri.round_reference(Xse, anchor, d)
    tol = sri.oracle_tolerance(Xse, anchor, d)
    e_r = float(bf.block_err(R.astype(LD), ref).max()) / tol
    T_ref = np.asarray(B, LD).T @ np.asarray(X, LD)
    bound = 8 * r * EPS * (np.abs(B).T @ np.abs(X))
    euc = np.r_[d * n + l:ra.k]
    e_t = float((np.abs(P[:, euc] - T_ref[:, euc]) / np.maximum(bound[:, euc], 1e-300)).max())
    sc = np.r_[d * n:d * n + l]
    nrm = np.sqrt((T_ref[:, sc] ** 2).sum(axis=0, keepdims=True))
    e_s = float((np.abs(sph - T_ref[:, sc] / nrm) / (bound[:, sc] / nrm.astype(np.float64) + 8 * EPS)).max())
    print("RATIO project %s: gram %.3f, sigma^2 %.3f, orthogonality %.3f, residual %.3f of their bounds; rotations %.2f "
          "(bound 8), translations / landmarks %.3f, unit spheres %.3f; |P^T P - host-fed| %.2e; 2f %.9g -> %.9g" %
          (name, g, rat[0], rat[1], rat[2], e_r, e_t, e_s, e_h, cost_before, out["cost_2f"]))
    assert e_r <= 8 and e_t <= 1 and e_s <= 1
    # the cost of the adopted point is the cost of the point returned
    ref_c, cb = sri.cost_reference(P, ra.Q.to_scipy(), d)
    assert abs(float(ref_c) - out["cost_2f"]) <= float(cb)


# ---- d. the reflect decision -------------------------------------------------------------------------------------------------
def _synthetic_ra(da, d):
    """a range-aided dataset with the reflect family's dimensions from arrays (dcora_radataset_create): an odometry
    chain of n = 9 poses, b = 3 landmarks seen from poses, l = 4 ranges; the measurements only have to make a session"""
    from dcora_amd import capi
    n, l, b = (spi.REFLECT_DIMS[key] for key in ("n", "l", "b"))
    rng = np.random.default_rng(77 + d)
    pp_ids = np.array([(i, i + 1) for i in range(n - 1)] + [(0, 4), (2, 7)], np.int32)
    m_pp = len(pp_ids)
    pp_vals = np.zeros((m_pp, d * d + d + 3))
    pp_vals[:, :d * d] = sri.random_rotations(rng, d, m_pp).transpose(0, 2, 1).reshape(m_pp, d * d)
    pp_vals[:, d * d:d * d + d] = rng.standard_normal((m_pp, d))
    pp_vals[:, d * d + d:] = [10.0, 5.0, 1.0]
    pl_ids = np.array([(1, 0), (4, 1), (7, 2), (8, 0)], np.int32)
    pl_vals = np.concatenate([rng.standard_normal((len(pl_ids), d)), np.full((len(pl_ids), 1), 4.0),
                              np.ones((len(pl_ids), 1))], axis=1)
    rg_ids = np.array([(0, 0, 1, 0, 0), (0, 3, 1, 1, 1), (0, 5, 1, 2, 2), (0, 2, 0, 6, 3)], np.int32)
    rg_vals = np.concatenate([rng.uniform(1, 3, (l, 1)), np.full((l, 1), 2.0), np.ones((l, 1))], axis=1)
    arrays = [np.ascontiguousarray(a) for a in (pp_ids, pp_vals, pl_ids, pl_vals, rg_ids, rg_vals)]

    class Synthetic(da.RADataset):
        def handle(self):
            h = C.c_void_p()
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            capi.check(capi.lib().dcora_radataset_create(d, n, l, b, m_pp, vp(arrays[0]), vp(arrays[1]), len(pl_ids),
                                                         vp(arrays[2]), vp(arrays[3]), l, vp(arrays[4]), vp(arrays[5]),
                                                         None, C.byref(h)))
            return h
    return Synthetic(None)


@pytest.mark.parametrize("d", spi.DIMS)
def test_reflect_decision(env, d):
    da, _ = env
    n, l, b, r = (spi.REFLECT_DIMS[key] for key in ("n", "l", "b", "r"))
    ra = _synthetic_ra(da, d)
    assert (ra.d, ra.n, ra.l, ra.b) == (d, n, l, b)
    for m in spi.REFLECT_KEEP + spi.REFLECT_FLIP:
        Xd, X = spi.reflect_case(d, m)
        want, kept, flipped = spi.reflect_expected(Xd, d, m)
        s = da.RaRbcdSession(ra, r)
        s.set_X(X)
        out = s.project()
        P = s.get_X()
        s.close()
        assert out["projected"] and s.r == d
        assert out["positive_dets"] in (m, n - m), (m, out)  # either handedness of the truncation
        assert out["reflected"] == (out["positive_dets"] < n // 2), (m, out)
        G = P.T @ P
        dist = {False: np.abs(G - kept.T @ kept).max(), True: np.abs(G - flipped.T @ flipped).max()}
        print("reflect d=%d m=%d: npos %d reflected %d; |G - G_kept| %.2e  |G - G_reflected| %.2e" %
              (d, m, out["positive_dets"], out["reflected"], dist[False], dist[True]))
        assert dist[want] <= 1e-10, (m, dist)
        assert dist[not want] > 1e-3, (m, dist)
        assert (np.linalg.det(spi.rotation_blocks(P, d, n, l, False)) > 1 - 64 * EPS).all()
        assert np.abs(np.linalg.norm(P[:, d * n:d * n + l], axis=0) - 1).max() <= 8 * EPS


# ---- e. r == d ---------------------------------------------------------------------------------------------------------------
def _next_iterates(s, before):
    before(s)
    g = s.run(max_iters=5, rgrad_tol=0.0)
    X = s.get_X()
    s.close()
    return X, g["cost"], g["gradnorm"], g["selected"]


@pytest.mark.parametrize("d", spi.DIMS)
def test_rank_d_session_is_passed_through(env, d):
    """the reference passes X through at r == d: not even a rotation block of determinant -1 is touched"""
    da, _ = env
    n = 17
    X = spi.lifted_point(d, d, n, spi.seed_of(d, d, n, 0.0), 0.0)
    if np.linalg.det(X[:, :d]) > 0:
        X[:, d - 1] = -X[:, d - 1]  # pose 0: det -1
    assert np.linalg.det(X[:, :d]) < 0
    seen = {}

    def call(s):
        s.set_X(X)
        out = s.project()
        assert not out["projected"] and out["basis"] is None and s.r == d
        assert np.array_equal(s.get_X(), X)
        assert out["cost_2f"] == s.evaluate()[0]
        _check_gram(out["gram"], X, d)
        _check_spectrum(out, X, d, d)
        seen.update(out)

    make = lambda: da.RbcdSession(sri.chain_dataset(da.Dataset, d, n, 5), num_robots=2, r=d)
    a = _next_iterates(make(), call)
    b = _next_iterates(make(), lambda s: s.set_X(X))
    assert seen["sigma"].shape == (d,)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- f. the projected session is a fresh session ---------------------------------------------------------------------------
def _solve_facts(s):
    res = s.last_result()
    res.pop("elapsedMs")
    return res


@pytest.mark.parametrize("name,R,r,iters", [("smallGrid3D", 5, 5, 12), ("tinyGrid3D", 3, 4, 35)])
def test_projected_pose_graph_session_runs_as_a_fresh_one(env, name, R, r, iters):
    """35 iterations on tinyGrid3D cross the restart at 30"""
    da, orc = env
    ds = common.product_dataset(name)
    d, n = ds.d, ds.n
    X = common.random_point(r, d, n, 4, orc.project_to_manifold)
    A = da.RbcdSession(ds, num_robots=R, r=r)
    A.set_X(X)
    A.run(max_iters=7, rgrad_tol=0.0)  # (a session in mid-flight: sequences, counters and a last solve to forget)
    out = A.project()
    assert out["projected"] and A.r == d
    Xp = A.get_X()
    assert Xp.shape == (d, (d + 1) * n)
    B = da.RbcdSession(ds, num_robots=R, r=d)
    B.set_X(Xp)
    assert out["cost_2f"] == pytest.approx(B.evaluate()[0], rel=1e-12)
    outs, Xs, facts, runs = [], [], [], []
    for s in (A, B):
        s.profile_tcg_runs(True)
        s.profile_tcg_read()
        outs.append(s.run(max_iters=iters, rgrad_tol=0.0))
        runs.append(s.profile_tcg_read()["launches"])
        s.profile_tcg_runs(False)
        Xs.append(s.get_X())
        facts.append(_solve_facts(s))
    for key in ("selected", "cost", "gradnorm"):
        assert outs[0][key].size == iters and np.array_equal(outs[0][key], outs[1][key]), key
    assert np.array_equal(Xs[0], Xs[1])
    assert facts[0] == facts[1] and runs[0] == runs[1], (facts, runs)  # the same solver form was picked
    A.close()
    B.close()


@pytest.mark.parametrize("name", RA_NAMES)
def test_projected_range_aided_session_runs_as_a_fresh_one(env, name):
    """12 greedy iterations, then 3 coloured sweeps with acceleration off"""
    da, orc = env
    ra = da.RADataset(ra_path(name))
    d, r = ra.d, ra.d + 2
    rng = np.random.default_rng(4)
    X = orc.project_to_manifold(r, d, ra.n, rng.uniform(-1, 1, (r, ra.k)), l=ra.l, b=ra.b)
    A = da.RaRbcdSession(ra, r, restart_interval=5)
    A.set_X(X)
    A.run(max_iters=4, rgrad_tol=0.0)
    out = A.project()
    assert out["projected"] and A.r == d
    Xp = A.get_X()
    B = da.RaRbcdSession(ra, d, restart_interval=5)
    B.set_X(Xp)
    got = []
    for s in (A, B):
        greedy = s.run(max_iters=12, rgrad_tol=0.0)
        Xg = s.get_X()
        facts = _solve_facts(s)
        s.set_acceleration(False)
        sweeps = s.run_coloured(max_sweeps=3, rgrad_tol=0.0)
        got.append((greedy, Xg, facts, sweeps, s.get_X()))
    a, b = got
    for key in ("selected", "cost", "gradnorm"):
        assert a[0][key].size == 12 and np.array_equal(a[0][key], b[0][key]), key
    assert np.array_equal(a[1], b[1]) and a[2] == b[2]
    for key in ("cost", "gradnorm"):
        assert a[3][key].size == 3 and np.array_equal(a[3][key], b[3][key]), key
    assert np.array_equal(a[4], b[4])
    A.close()
    B.close()


# ---- g. robust state survives ---------------------------------------------------------------------------------------------
def _with_outliers(ds_cls, base, n_out, seed):
    # (copied from tests/test_gnc_session_gpu.py)
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


def _robust_state_survives(A, fresh, d, mu_step):
    """tests/test_session_lift_gpu.py's check with the projection in the lift's place.  A: a robust session above rank d
    with its team enabled, after two weight updates; fresh(w, X) -> a robust session at rank d that has made two weight
    updates of its own (mu and the update count advance with them) and was then given the weights w"""
    w, rinfo, tinfo = A.get_weights(), A.robust_info(), A.team_info()
    assert rinfo["updates"] == 2
    out = A.project()
    assert out["projected"] and A.r == d
    assert np.array_equal(A.get_weights(), w)
    assert A.robust_info() == rinfo
    after = A.team_info()
    assert after["weight_updates"] == tinfo["weight_updates"] and after["resets"] == tinfo["resets"]
    assert after["inner_iter"] == 0  # (the round counters are set_X's)
    assert all(A.agent_status(q) is None for q in range(A.R))  # statuses unknown after the projection
    Xp = A.get_X()
    B = fresh(w, Xp)
    B.set_X(Xp)
    assert B.robust_info() == rinfo and np.array_equal(B.get_weights(), w)
    assert B.team_info()["weight_updates"] == after["weight_updates"]
    for q in range(A.R):  # the loop-closure counts the team decides by
        assert A.loop_closure_stats(q) == B.loop_closure_stats(q), q
    outs, Xs = [], []
    for s in (A, B):
        outs.append(s.run(max_iters=12, rgrad_tol=0.0))
        Xs.append(s.get_X())
    assert np.array_equal(outs[0]["selected"], outs[1]["selected"])
    if np.any(w == 0.0):  # explicit zeros on the live session's patterns: tests/test_gnc_session_gpu.py:167-169's bounds
        assert np.allclose(outs[0]["cost"], outs[1]["cost"], rtol=1e-9, atol=0)
        assert common.rel(Xs[0], Xs[1]) < 1e-7
        B.set_X(Xs[0])  # the third update below starts from one point on both
    else:
        assert np.array_equal(outs[0]["cost"], outs[1]["cost"]) and np.array_equal(Xs[0], Xs[1])
    assert any(A.agent_status(q) is not None for q in range(A.R))
    A.update_weights()
    B.update_weights()
    now = A.robust_info()
    assert now["updates"] == 3 and now["mu"] == pytest.approx(rinfo["mu"] * mu_step, rel=1e-12)
    assert np.array_equal(A.get_weights(), B.get_weights())
    out = A.run_team()
    assert out["iters"] > 0
    A.close()
    B.close()


def test_robust_pose_graph_session_keeps_its_state(env):
    da, _ = env
    from dcora_amd import robust as rb
    R, r = 5, 5
    ds = _with_outliers(da.Dataset, common.product_dataset("smallGrid3D"), 12, seed=2)
    params = rb.RobustCostParameters("GNC_TLS", **GNC)
    A = da.RbcdSession(ds, num_robots=R, r=r, robust=params)
    A.enable_team(max_num_iters=20)
    X0 = np.zeros((r, 4 * ds.n))
    X0[:3] = da.chordal_initialization(common.product_dataset("smallGrid3D"))
    A.set_X(X0)
    for _ in range(2):
        A.run(max_iters=5, rgrad_tol=0.0)
        A.update_weights()

    def fresh(w, X):
        B = da.RbcdSession(ds, num_robots=R, r=ds.d, robust=params)
        B.enable_team(max_num_iters=20)
        B.set_X(X)
        B.update_weights()
        B.update_weights()
        B.set_weights(w)
        return B

    _robust_state_survives(A, fresh, ds.d, GNC["GNCMuStep"])


def test_robust_range_aided_session_keeps_its_state(env, tmp_path):
    """the loop-closure variant of tiers the range-aided GNC tests use (ra_loops.GNC_FIXTURE), rank 4 -> 2"""
    da, _ = env
    from dcora_amd import robust as rb
    path = ra_loops.write_loops_variant(tmp_path, **ra_loops.GNC_FIXTURE)[0]
    ra = da.RADataset(path)
    r = ra.d + 2
    params = rb.RobustCostParameters("GNC_TLS", **ra_loops.GNC_PARAMS)
    A = da.RaRbcdSession(ra, r, restart_interval=5, robust=params)
    A.enable_team(max_num_iters=20)
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    A.set_X(X0)
    for _ in range(2):
        A.run(max_iters=5, rgrad_tol=0.0)
        A.update_weights()

    def fresh(w, X):
        B = da.RaRbcdSession(da.RADataset(path), ra.d, restart_interval=5, robust=params)
        B.enable_team(max_num_iters=20)
        B.set_X(X)
        B.update_weights()
        B.update_weights()
        B.set_weights(w)
        return B

    _robust_state_survives(A, fresh, ra.d, ra_loops.GNC_PARAMS["GNCMuStep"])


# ---- h. certificate and lift after a projection ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["smallGrid3D", "range_aided_slam_test_3d"])
def test_certificate_and_lift_after_a_projection(env, name):
    """the session has certified before the projection, so the certificate's r-sized buffer is re-sized, not built anew"""
    da, orc = env
    if name.startswith("range_aided"):
        ra = da.RADataset(ra_path(name))
        d, r = ra.d, ra.d + 2
        rng = np.random.default_rng(4)
        X = orc.project_to_manifold(r, d, ra.n, rng.uniform(-1, 1, (r, ra.k)), l=ra.l, b=ra.b)
        make = lambda rank: da.RaRbcdSession(ra, rank)
        tol = dict(gradient_tolerance=1e-4, preconditioned_gradient_tolerance=1e-4)
    else:
        ds = common.product_dataset(name)
        d, r = ds.d, 5
        X = common.random_point(r, d, ds.n, 4, orc.project_to_manifold)
        make = lambda rank: da.RbcdSession(ds, num_robots=5, r=rank)
        tol = {}
    A = make(r)
    A.set_X(X)
    A.run(max_iters=3, rgrad_tol=0.0)
    A.certify(ETA)
    A.project()
    Xp = A.get_X()
    B = make(d)
    B.set_X(Xp)
    ca, cb = A.certify(ETA), B.certify(ETA)
    B.close()
    print("%s after the projection: psd %s / fresh %s, theta %.12g / fresh %.12g" % (name, ca[0], cb[0], ca[1], cb[1]))
    assert ca[0] == cb[0] and ca[1] == cb[1]
    assert np.array_equal(ca[2], cb[2])
    assert not ca[0], "a random point projected to rank d is no certified solution"
    escaped, _ = A.lift(ca[1], ca[2], **tol)
    assert A.r == d + int(escaped)
    g = A.run(max_iters=5, rgrad_tol=0.0)
    assert g["cost"].size == 5 and np.isfinite(g["cost"]).all()
    if escaped:
        assert A.get_X().shape[0] == d + 1
    A.close()


# ---- i. refusals ---------------------------------------------------------------------------------------------------------------
def _refused_then_run(make, X0, call):
    """(X, cost, gradnorm, selected) of 5 iterations after 3, with the refused call between them or without it"""
    s, ex = make()
    s.set_X(X0)
    s.run(max_iters=3, rgrad_tol=0.0)
    r = s.r
    if call:
        assert _status(s.project) == UNSUPPORTED
        from dcora_amd import capi
        assert b"job" in capi.lib().dcora_last_error()  # the message names the multi-rank follow-up as absent
        assert s.r == r
    g = s.run(max_iters=5, rgrad_tol=0.0)
    X = s.get_X()
    if ex is not None:
        ex.close()
    s.close()
    return X, g["cost"], g["gradnorm"], g["selected"]


@pytest.mark.parametrize("kind", ["exchange attached", "ranked robust", "ranked robust range-aided"])
def test_refusals_leave_the_session_as_it_was(env, kind):
    da, orc = env
    import uuid
    from dcora_amd import robust as rb
    job = lambda: "p%s" % uuid.uuid4().hex[:12]
    if kind == "ranked robust range-aided":
        ra = da.RADataset(ra_path(RA_NAMES[0]))
        X0 = _odometry_start(ra, ra.d + 2)
        make = lambda: da.ra_robust_ranked_session(ra, job(), ra.d + 2, robust=rb.RobustCostParameters("GNC_TLS", **GNC))
    else:
        ds = common.product_dataset("smallGrid3D")
        X0 = common.random_point(5, ds.d, ds.n, 4, orc.project_to_manifold)
        if kind == "exchange attached":
            def make():
                s = da.RbcdSession(ds, num_robots=5, r=5)
                return s, da.Exchange(s, job())
        else:
            make = lambda: da.robust_ranked_session(ds, job(), num_robots=5, r=5,
                                                    robust=rb.RobustCostParameters("GNC_TLS", **GNC))
    a = _refused_then_run(make, X0, True)
    b = _refused_then_run(make, X0, False)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_a_rank_of_a_job_is_refused(env):
    da, orc = env
    ds = common.product_dataset("smallGrid3D")
    X0 = common.random_point(5, ds.d, ds.n, 4, orc.project_to_manifold)
    s = da.RbcdSession(ds, num_robots=4, r=5, rank=0, world_size=2)
    s.set_X(X0)
    assert _status(s.project) == UNSUPPORTED and s.r == 5
    assert np.array_equal(s.get_X(), X0)
    s.close()
    ra = da.RADataset(ra_path(RA_NAMES[0]))
    t = da.RaRbcdSession(ra, ra.d + 2, rank=0, world_size=2)
    t.set_X(_odometry_start(ra, ra.d + 2))
    assert _status(t.project) == UNSUPPORTED and t.r == ra.d + 2
    t.close()


# ---- j. the driver -----------------------------------------------------------------------------------------------------------
PARENT_KEYS = {"X", "rank", "certified", "theta", "total_iters", "suboptimality_gap_f", "levels", "cost", "gradnorm",
               "selected", "rank_trace"}
EXTRA_KEYS = {"sigma", "projected_cost_2f", "refined_cost_2f", "refine_iters"}
ROUND_KEYS = {"trajectory", "unit_spheres", "landmarks", "rounded_cost_2f", "rounded_gradnorm"}


def _driver_checks(plain, res, Q, P_host, d, eta, label):
    for key in ("X", "cost", "gradnorm", "selected", "rank_trace"):
        assert np.array_equal(plain[key], res[key]), key
    for key in ("rank", "certified", "theta", "total_iters", "suboptimality_gap_f"):
        assert plain[key] == res[key], key
    assert [lv["cost_2f"] for lv in plain["levels"]] == [lv["cost_2f"] for lv in res["levels"]]
    assert res["certified"] and res["rank"] > d
    assert res["sigma"].shape == (res["rank"],)
    # the projected cost is the cost of Proj(V_d^T X): a gauge-invariant number, so the host-fed projection of the
    # returned X has it too
    ref, bound = sri.cost_reference(P_host, Q, d)
    relaxed = res["levels"][-1]["cost_2f"]
    # the relaxation's bound.  Where the driver gives no gap (range-aided): S + eta I >= 0 at a stationary X gives
    # <Z Q, Z> >= <X Q, X> - eta |Z|_F^2 for every feasible Z
    gap2 = 2 * res["suboptimality_gap_f"] if res["suboptimality_gap_f"] is not None else eta * float((P_host ** 2).sum())
    print("driver %s: sigma %s, relaxed 2f %.9g, projected 2f %.9g (longdouble %.9g, bound %.2e), refined 2f %.9g in %d "
          "iterations, 2 gap %.3g" % (label, np.array2string(res["sigma"], precision=3), relaxed,
                                      res["projected_cost_2f"], float(ref), float(bound), res["refined_cost_2f"],
                                      res["refine_iters"], gap2))
    assert abs(float(ref) - res["projected_cost_2f"]) <= float(bound)
    assert res["refined_cost_2f"] <= res["projected_cost_2f"]  # (RTR is monotone)
    assert res["refined_cost_2f"] >= relaxed - gap2


def test_raslam_driver_projects_refines_and_rounds_on_the_device(env):
    da, orc = env
    from dcora_amd import driver
    ra = da.RADataset(ra_path("range_aided_slam_test_3d"))
    d = ra.d
    rng = np.random.default_rng(12)
    X0 = orc.project_to_manifold(d, d, ra.n, rng.standard_normal((d, ra.k)), l=ra.l, b=ra.b)
    kw = dict(max_iters=300, rgrad_tol=1e-3, r_max=d + 5)
    plain = driver.raslam_staircase_session(ra, X0, **kw)
    res = driver.raslam_staircase_session(ra, X0, project_on_device=True, round_on_device=True, **kw)
    assert set(plain) == PARENT_KEYS and set(res) == PARENT_KEYS | EXTRA_KEYS | ROUND_KEYS
    X = res["X"]
    H = da.project_solution_raslam(X, X.shape[0], d, ra.n, ra.l, ra.b)
    _driver_checks(plain, res, ra.Q.to_scipy(), H, d, 1e-3, "range_aided_slam_test_3d")
    # the rounding is of the refined rank-d point: its cost is the refined cost (a rotation of the frame keeps it)
    assert res["rounded_cost_2f"] == pytest.approx(res["refined_cost_2f"], rel=1e-9)
    assert res["trajectory"].shape == (d, (d + 1) * ra.n)


def test_pose_graph_driver_projects_and_refines_on_the_device(env):
    da, orc = env
    from dcora_amd import driver
    ds = common.product_dataset("smallGrid3D")
    d, n = ds.d, ds.n
    X0 = common.random_point(3, d, n, 4, orc.project_to_manifold)
    kw = dict(num_robots=5, r_min=3, r_max=9, max_iters=400, rgrad_tol=0.05)
    plain = driver.multi_robot_staircase_session(ds, X0, **kw)
    res = driver.multi_robot_staircase_session(ds, X0, project_on_device=True, **kw)
    assert set(plain) == PARENT_KEYS and set(res) == PARENT_KEYS | EXTRA_KEYS
    X = res["X"]
    H = sri.se_from_ra(da.project_solution_raslam(spi.ra_from_se(X, d, n), X.shape[0], d, n, 0, 0), d, n, 0)
    _driver_checks(plain, res, da.build_Q_pgo(ds).to_scipy(), H, d, 1e-3, "smallGrid3D")
