"""The certificate of a live session, on the device (dcora_rbcd_certify / dcora_ra_rbcd_certify): fastVerification of
S = Q - Lambda(X) with the Q the session holds now and its current iterate.  Every case compares the call with the path
the suite pins to the oracle -- da.dual_certificate followed by da.fast_verification on a host Q -- at the same X, the
same eta and the same block size.

Tolerances (tests/test_gpu_parity.py::test_certification): theta against the host path 2e-3 relative; lambda_min against
numpy's eigvalsh of the host-built S + eta I 2e-3 max(1, |w0|); | |v| - 1 | <= 1e-12; |theta - v^T S_host v| <= d 1e-9
(the device and the host S differ only in the d x d Lambda blocks, whose entries test_certification bounds at 1e-9: the
2-norm of the difference is at most d 1e-9)."""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import common
from test_raslam import ra_path

pytestmark = pytest.mark.gpu

ETA = 1e-3
GNC = dict(GNCBarc=10.0, GNCMuStep=2.0)  # as tests/test_gnc_session_gpu.py


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


@pytest.fixture(scope="module")
def grid(env):
    """smallGrid3D, its host Q and the random point of test_certification (seed 4), shared and left unchanged"""
    da, orc = env
    ds = common.product_dataset("smallGrid3D")
    X = common.random_point(5, ds.d, ds.n, 4, orc.project_to_manifold)
    return ds, da.build_Q_pgo(ds), X


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


def _lifted_start(orc, ra, r, seed, noise):  # as tests/test_ra_session.py
    rng = np.random.default_rng(seed)
    lift = np.linalg.qr(rng.standard_normal((r, ra.d)))[0]
    M = lift @ ra.gt + noise * rng.standard_normal((r, ra.k))
    return orc.project_to_manifold(r, ra.d, ra.n, M, l=ra.l, b=ra.b)


def _host(da, r, d, n, X, Q, block, **kw):
    S = da.dual_certificate(r, d, n, X, Q, **kw)
    return S, da.fast_verification(S, ETA, block=block)


def _refused_alike(tag, got, S, host, d, dense=True):
    """both paths refuse; theta, lambda_min and v of the session call within the module's tolerances"""
    psd, theta, v, lmin, info = got
    hpsd, htheta, hv, hlmin = host
    A = S.to_scipy()
    quad = v @ (A @ v)
    print("%s: psd %s / host %s, theta %.12g / host %.12g, lambda_min %.12g / host %.12g, |v| - 1 %.3g, "
          "theta - v'Sv %.3g, matvecs %d" % (tag, psd, hpsd, theta, htheta, lmin, hlmin, np.linalg.norm(v) - 1,
                                             theta - quad, info["matvecs"]))
    assert not hpsd and not psd
    assert abs(theta - htheta) <= 2e-3 * abs(htheta)
    assert abs(np.linalg.norm(v) - 1) <= 1e-12
    assert abs(theta - quad) <= d * 1e-9
    assert info["matvecs"] > 0
    if dense:
        w0 = np.linalg.eigvalsh((A + ETA * sp.identity(A.shape[0])).toarray())[0]
        print("%s: eigvalsh %.12g" % (tag, w0))
        assert abs(lmin - w0) <= 2e-3 * max(1.0, abs(w0))


def test_indefinite_point_of_a_pose_graph(env, grid):
    da, orc = env
    ds, Q, X = grid
    s = da.RbcdSession(ds, num_robots=5, r=5)
    s.set_X(X)
    got = s.certify(ETA)
    S, host = _host(da, 5, ds.d, ds.n, X, Q, ds.d + 1)
    _refused_alike("smallGrid3D random point", got, S, host, ds.d)
    s.close()


def test_entries_of_lambda_absent_from_the_pattern_of_Q(env):
    """sphere2500: six entries inside rotation blocks are structural zeros of Q, so S has six entries Q's pattern does
    not hold (the host assembly merges them in); k = 10000 is too large for a dense eigvalsh in a quick test"""
    da, orc = env
    ds = common.product_dataset("sphere2500")
    Q = da.build_Q_pgo(ds)
    X = common.random_point(5, ds.d, ds.n, 4, orc.project_to_manifold)
    S, host = _host(da, 5, ds.d, ds.n, X, Q, ds.d + 1)
    assert int(S.rp[-1]) > int(Q.rp[-1])
    s = da.RbcdSession(ds, num_robots=5, r=5)
    s.set_X(X)
    _refused_alike("sphere2500 random point", s.certify(ETA), S, host, ds.d, dense=False)
    s.close()


@pytest.fixture(scope="module")
def grid_optimum(env, grid):
    """the optimum of smallGrid3D at r = 5: a centralised solve from the chordal start to |rgrad| < 1e-6"""
    da, orc = env
    ds, Q, _ = grid
    X0 = np.zeros((5, 4 * ds.n))
    X0[:3] = da.chordal_initialization(ds)
    P = da.QuadraticProblem(5, ds.d, ds.n, Q)
    opt = da.QuadraticOptimizer(P, da.ROptParameters(RTR_iterations=100, RTR_tCG_iterations=200, gradnorm_tol=1e-6))
    X = opt.optimize(X0)
    print("centralised solve: |rgrad| %.3g" % opt.getOptResult()["gradNormOpt"])
    P.close()
    return X


def test_accepted_certificate_of_a_pose_graph(env, grid, grid_optimum):
    da, orc = env
    ds, Q, _ = grid
    X = grid_optimum
    S, host = _host(da, 5, ds.d, ds.n, X, Q, ds.d + 1)
    assert host[0], "the host path must accept this point, or the case shows nothing"
    s = da.RbcdSession(ds, num_robots=5, r=5)
    s.set_X(X)
    psd, theta, v, lmin, info = s.certify(ETA)
    print("optimum: psd %s, numeric %.3f ms, symbolic %.3f ms, logdet %.6g" % (psd, info["numeric_ms"],
                                                                             info["symbolic_ms"], info["logdet"]))
    assert psd
    assert info["numeric_ms"] > 0
    assert info["matvecs"] == 0
    s.close()


def test_analysis_cache_is_shared_with_cert_prepare(env, grid):
    da, orc = env
    ds, Q, X = grid
    s = da.RbcdSession(ds, num_robots=5, r=5)
    s.set_X(X)
    da.chol_cache_clear()
    da.cert_prepare(Q, ds.d, ds.n, block=ds.d + 1)
    info = s.certify(ETA)[4]
    print("after cert_prepare: symbolic %.3f ms, numeric %.3f ms" % (info["symbolic_ms"], info["numeric_ms"]))
    assert info["symbolic_ms"] == 0
    assert info["numeric_ms"] > 0
    s.close()


def test_current_weights_of_a_robust_session(env):
    da, orc = env
    from dcora_amd import driver
    from dcora_amd import robust as rb
    R, r = 5, 5
    ds = _with_outliers(da.Dataset, common.product_dataset("smallGrid3D"), 12, seed=2)
    lc = driver.loop_closure_mask(ds, R)
    s = da.RbcdSession(ds, num_robots=R, r=r, robust=rb.RobustCostParameters("GNC_TLS", **GNC))
    X = common.random_point(r, ds.d, ds.n, 4, orc.project_to_manifold)
    s.set_X(X)
    rng = np.random.default_rng(11)
    w1 = s.get_weights()
    w2 = w1.copy()
    kind = rng.integers(0, 3, int(lc.sum()))
    w2[lc] = np.where(kind == 0, 0.0, np.where(kind == 1, rng.uniform(0.2, 0.9, kind.size), 1.0))
    assert np.any(w2[lc] == 0) and np.any(w2[lc] == 1) and np.any((w2[lc] > 0) & (w2[lc] < 1))
    thetas = []
    for tag, w in (("creation weights", w1), ("set_weights", w2)):
        if w is w2:
            s.set_weights(w)
        assert np.array_equal(s.get_weights(), w)
        got = s.certify(ETA)
        with_w = da.Dataset(ds.d, ds.n, ds.ids.copy(), ds.vals.copy())
        with_w.vals[:, -1] = w
        S, host = _host(da, r, ds.d, ds.n, X, da.build_Q_pgo(with_w), ds.d + 1)
        _refused_alike("robust session, " + tag, got, S, host, ds.d)
        thetas.append(got[1])
    assert thetas[0] != thetas[1]  # (stale values behind the cached slot table would repeat the first)
    s.close()


def test_certify_leaves_the_session_alone(env, grid):
    da, orc = env
    ds, Q, X = grid
    outs, Xs = [], []
    for certifies in (True, False):
        s = da.RbcdSession(ds, num_robots=5, r=5)
        s.set_X(X)
        parts = []
        for iters in (10, 10, 15):  # 35 iterations: the restart at 30 is inside
            parts.append(s.run(max_iters=iters, rgrad_tol=0.0))
            if certifies and len(parts) < 3:
                a = s.certify(ETA)
                b = s.certify(ETA)
                assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and np.array_equal(a[2], b[2])
                assert a[4]["logdet"] == b[4]["logdet"]
        outs.append({k: np.concatenate([p[k] for p in parts]) for k in ("selected", "cost", "gradnorm")})
        Xs.append(s.get_X())
        s.close()
    for k in ("selected", "cost", "gradnorm"):
        assert outs[0][k].size == 35 and np.array_equal(outs[0][k], outs[1][k]), k
    assert np.array_equal(Xs[0], Xs[1])


@pytest.mark.parametrize("name,r", [("range_aided_slam_test_3d", 4), ("range_aided_slam_test_2d", 3)])
def test_range_aided_session(env, name, r):
    da, orc = env
    ra = da.RADataset(ra_path(name))
    s = da.RaRbcdSession(ra, r)
    kw = dict(l=ra.l, b=ra.b)
    X = _lifted_start(orc, ra, r, 5, 0.05)
    s.set_X(X)
    got = s.certify(ETA)
    S, host = _host(da, r, ra.d, ra.n, X, ra.Q, 1, **kw)
    _refused_alike(name + " noisy start", got, S, host, ra.d)
    Xgt = np.linalg.qr(np.random.default_rng(5).standard_normal((r, ra.d)))[0] @ ra.gt
    s.set_X(Xgt)
    S, host = _host(da, r, ra.d, ra.n, Xgt, ra.Q, 1, **kw)
    psd, theta, v, lmin, info = s.certify(ETA)
    print("%s ground truth: psd %s / host %s, numeric %.3f ms" % (name, psd, host[0], info["numeric_ms"]))
    assert host[0] and psd
    assert info["numeric_ms"] > 0
    s.close()


def test_block_csr_central_problem(env):
    """9216 poses: the smallest lattice whose central Q-apply takes the block form"""
    da, orc = env
    from dcora_amd import synth
    ds = synth.lattice_se2()
    assert ds.d == 2 and ds.n == 9216
    r = 3
    X = orc.project_to_manifold(r, 2, ds.n, np.random.default_rng(r).uniform(-1, 1, (r, 3 * ds.n)))
    s = da.RbcdSession(ds, num_robots=1, r=r)
    s.set_X(X)
    psd, theta, v, lmin, info = s.certify(ETA)
    S, (hpsd, htheta, hv, hlmin) = _host(da, r, 2, ds.n, X, da.build_Q_pgo(ds), 3)
    print("lattice: psd %s / host %s, theta %.12g / host %.12g, lambda_min %.12g / host %.12g" %
          (psd, hpsd, theta, htheta, lmin, hlmin))
    assert psd == hpsd
    assert not psd
    assert abs(theta - htheta) <= 2e-3 * abs(htheta)
    s.close()


def test_refusals_and_optional_outputs(env, grid):
    da, orc = env
    from dcora_amd import capi
    ds, Q, X = grid
    ranked = da.RbcdSession(ds, num_robots=4, r=5, rank=0, world_size=2)
    with pytest.raises(capi.DcoraError) as e:
        ranked.certify(ETA)
    assert e.value.status == 8  # DCORA_ERR_UNSUPPORTED
    assert "dcora_exchange_certify" in str(e.value)
    ranked.close()
    s = da.RbcdSession(ds, num_robots=5, r=5)
    s.set_X(X)
    full = s.certify(ETA)
    cert = C.c_int(-1)
    capi.check(capi.lib().dcora_rbcd_certify(s.h, ETA, C.byref(cert), None, None, None, None, None))
    assert cert.value == 0 and not full[0]
    th = C.c_double()
    capi.check(capi.lib().dcora_rbcd_certify(s.h, ETA, C.byref(cert), C.byref(th), None, None, None, None))
    assert th.value == full[1]
    s.close()
    ra = da.RADataset(ra_path("range_aided_slam_test_2d"))
    t = da.RaRbcdSession(ra, 3)
    t.set_X(_lifted_start(orc, ra, 3, 5, 0.05))
    capi.check(capi.lib().dcora_ra_rbcd_certify(t.h, ETA, C.byref(cert), None, None, None, None, None))
    assert cert.value == 0
    t.close()
