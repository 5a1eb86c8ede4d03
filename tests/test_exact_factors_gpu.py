"""The device Cholesky and both preconditioner inverses against exact factors (tests/exact_factors.py: A = L D L^T
formed in integers, so A^-1 V = W, det A = 2^(sum e_i) and the inertia of A are known without a reference solver).

1. dense inverse (k <= 2200):      PreCondition(X, V) == tangent projection of W at X
2. partitioned sparse inverse:     the same through DCORA_PRECOND=sparse, r = 3, 5, 9 (the three k_sp_mtile forms); the
                                   lattice is sparse by size and also runs without the variable
3. verdict and log-determinant of dcora_cert_is_psd_device, block = d + 1 and block = 1
4. ONE non-positive pivot, D_pp = -2^-a, swept over positions of L's order: the verdict is no; with D_pp = +2^-a at the
   same place it is yes and the log-determinant is right
5. dcora_problem_create refuses the negative matrix in both forms, and the creation that follows is sound

Bounds (exact_factors.tol_solve / tol_logdet): a device error may be 8 x max(LAPACK's recorded error on the case,
eps kappa_2(A)); solves relative in the Frobenius norm, the log-determinant absolute with n eps sum |2 ln l_ii| added
for the free order of the device's atomicAdd.  Every figure is printed before it is asserted; the largest
device / reference ratios per kernel family and scale group are in profiles/exact_factors.txt.

Which structure a case reaches is asserted where the library exposes it (precond_info()["kind"], the levels of
is_psd_device).  The panel, super-panel and wide-piece paths taken inside a launch are not exposed: the case table of
exact_factors.py names them from the sizes alone."""
import os

import numpy as np
import pytest

import exact_factors as ef

pytestmark = pytest.mark.gpu

DENSE = ["g16", "g17", "g144", "g145", "p171", "g550"]
SWEPT = ["g16", "g17", "g144", "g145", "l1000", "h144", "ra"]
RATIOS = {}   # (family, a) -> (device error / max(LAPACK, eps kappa), where)


def _note(family, a, ratio, where):
    if ratio > RATIOS.get((family, a), (-1.0, ""))[0]:
        RATIOS[(family, a)] = (ratio, where)


@pytest.fixture(scope="module", autouse=True)
def caches_cleared_at_the_end(built):
    yield
    import dcora_amd as da
    da.precond_cache_clear()
    da.chol_cache_clear()
    for (family, a), (ratio, where) in sorted(RATIOS.items()):
        print("RATIO %-44s a=%-2d %8.3f  (%s)" % (family, a, ratio, where))


@pytest.fixture
def sparse_env(built):
    old = os.environ.get("DCORA_PRECOND")
    os.environ["DCORA_PRECOND"] = "sparse"
    yield
    if old is None:
        del os.environ["DCORA_PRECOND"]
    else:
        os.environ["DCORA_PRECOND"] = old


def _point(c, r):
    import dcora_amd as da
    rng = np.random.default_rng(1000 + r)
    return da.manifold_project(r, c.d, c.n, rng.uniform(-1, 1, (r, c.k)), l=c.l, b=c.b)


def _check_inverse_action(c, a, r, kind, family, p=None):
    """(A^-1 V^T)^T projected at X against the projection of W^T; A is the positive twin at p when p is given"""
    import dcora_amd as da
    from oracle import orc
    W, V = c.WV(a, r, p)
    P = da.QuadraticProblem(r, c.d, c.n, c.csr(a, p), reg=0.0, l=c.l, b=c.b)
    try:
        assert P.precond_info()["kind"] == kind
        X = _point(c, r)
        Z = P.PreCondition(X, np.ascontiguousarray(V.T))
    finally:
        P.close()
    want = orc.tangent_project(r, c.d, c.n, X, np.ascontiguousarray(W.T), l=c.l, b=c.b)
    err = np.linalg.norm(Z - want) / np.linalg.norm(want)
    base = ef.base_solve(c.id, a)
    print("%s a=%d r=%d %s%s: error %.3e = %.3f x max(LAPACK %.2e, eps kappa %.2e)" % (
        c.id, a, r, kind, "" if p is None else " twin p=%d" % p, err, err / base,
        ef.ref()[(c.id, a)]["lapack_solve"], ef.EPS * ef.ref()[(c.id, a)]["kappa"]))
    _note(family, a, err / base, "%s r=%d" % (c.id, r))
    assert err <= 8.0 * base


# ---- 1. dense form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,r", [(c, 5) for c in DENSE] + [("g144", 3), ("g144", 16)])
def test_dense_inverse_action(built, cid, r):
    if os.environ.get("DCORA_PRECOND"):
        pytest.skip("DCORA_PRECOND overrides the choice of preconditioner this test is about")
    c = ef.case(cid)
    for a in ef.SCALES:
        _check_inverse_action(c, a, r, "dense", "dense build (device_dense_spd_inverse)")


# ---- 2. sparse form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,r", [(c, r) for c in ("g144", "h144", "ra") for r in (3, 5, 9)] + [("l1000", 5)])
def test_sparse_inverse_action(sparse_env, cid, r):
    c = ef.case(cid)
    for a in ef.SCALES:
        _check_inverse_action(c, a, r, "sparse", "sparse build + k_sp_mtile replay (k_small_*)")


def test_sparse_inverse_action_by_size(built):
    if os.environ.get("DCORA_PRECOND"):
        pytest.skip("DCORA_PRECOND overrides the choice of preconditioner this test is about")
    c = ef.case("l1000")
    for a in ef.SCALES:
        _check_inverse_action(c, a, 5, "sparse", "sparse build + k_sp_mtile replay (k_small_*)")


# ---- 3. verdict and log-determinant -------------------------------------------------------------------------------------
def _check_logdet(c, a, block, info, p=None):
    want = c.logdet(a, p)
    err = abs(info["logdet"] - want)
    r_ = ef.ref()[(c.id, a)]
    _note("log det, multifrontal k_chol_* (is_psd_device)", a, err / ef.base_logdet(c.id, a),
          "%s block %d%s" % (c.id, block, "" if p is None else " p=%d" % p))
    assert err <= ef.tol_logdet(c.id, a, p), (
        "%s a=%d block %d p=%s: log det %.17g, exact %.17g, error %.3e > %.3e (LAPACK's %.2e)" % (
            c.id, a, block, p, info["logdet"], want, err, ef.tol_logdet(c.id, a, p), r_["lapack_logdet"]))
    return err


@pytest.mark.parametrize("cid", ef.CASES)
def test_verdict_and_logdet(built, cid):
    import dcora_amd as da
    c = ef.case(cid)
    levels = {}
    for block in (c.d + 1, 1):
        for a in ef.SCALES:
            pd, info = da.is_psd_device(c.csr(a), block, info=True)
            assert pd, (cid, a, block)
            err = _check_logdet(c, a, block, info)
            print("%s a=%d block %d: levels %d launches %d, log det error %.3e (bound %.3e, LAPACK's %.2e)" % (
                cid, a, block, info["levels"], info["launches"], err, ef.tol_logdet(cid, a),
                ef.ref()[(cid, a)]["lapack_logdet"]))
            levels[block] = info["levels"]
    if cid in ("g16", "g17"):
        assert levels[4] == 1          # one front: one panel (g17: and one column block past it)
    if cid == "h144":                  # the hubs are eliminated last, as a piece (and a level) of their own
        g = ef.case("g144")
        assert levels[4] == da.is_psd_device(g.csr(0), 4, info=True)[1]["levels"] + 1


# ---- 4. one non-positive pivot --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", ef.SCALES)
@pytest.mark.parametrize("cid", SWEPT)
def test_one_nonpositive_pivot(built, cid, a):
    import dcora_amd as da
    c = ef.case(cid)
    da.is_psd_device(c.csr(a), c.block)     # the analysis of the pattern is cached from here on
    worst = 0.0
    for p in c.sweep_positions():
        p = int(p)
        neg, info = da.is_psd_device(c.csr(a, p, True), c.block, info=True)
        assert info["symbolic_ms"] == 0.0
        assert not neg, "%s a=%d: D_pp = -2^-%d at position %d of %d accepted as positive definite" % (cid, a, a, p, c.k)
        pos, info = da.is_psd_device(c.csr(a, p, False), c.block, info=True)
        assert info["symbolic_ms"] == 0.0
        assert pos, "%s a=%d: D_pp = +2^-%d at position %d of %d refused" % (cid, a, a, p, c.k)
        worst = max(worst, _check_logdet(c, a, c.block, info, p) / ef.tol_logdet(cid, a, p))
    print("%s a=%d: %d positions, largest log det error / bound %.3f" % (cid, a, c.sweep_positions().size, worst))


# ---- 5. the refusal of dcora_problem_create ---------------------------------------------------------------------------------
def _refused_then_sound(c, a, kind, family):
    import dcora_amd as da
    from dcora_amd.capi import DcoraError
    for p in c.create_positions():
        with pytest.raises(DcoraError, match="not positive definite") as ei:
            da.QuadraticProblem(5, c.d, c.n, c.csr(a, p, True), reg=0.0, l=c.l, b=c.b)
        assert ei.value.status == 4     # DCORA_ERR_NOT_PD
        _check_inverse_action(c, a, 5, kind, family, p=p)


@pytest.mark.parametrize("a", ef.SCALES)
def test_create_refuses_one_nonpositive_pivot_dense(built, a):
    if os.environ.get("DCORA_PRECOND"):
        pytest.skip("DCORA_PRECOND overrides the choice of preconditioner this test is about")
    _refused_then_sound(ef.case("g144"), a, "dense", "dense build (device_dense_spd_inverse)")


@pytest.mark.parametrize("a", ef.SCALES)
@pytest.mark.parametrize("cid", ["g144", "h144", "l1000"])
def test_create_refuses_one_nonpositive_pivot_sparse(sparse_env, cid, a):
    _refused_then_sound(ef.case(cid), a, "sparse", "sparse build + k_sp_mtile replay (k_small_*)")
