"""tests/exact_factors.py (matrices A = L D L^T formed in integers: inverse action, determinant and inertia known
exactly) is what it says it is, its sign sweeps meet the conditions that make their verdicts well defined, and the HOST
factorisation code answers it within the bounds the device is held to in test_exact_factors_gpu.py."""
import importlib.util
import os

import numpy as np
import pytest
import scipy.linalg as sl

import exact_factors as ef
from test_sparse_precond import _selftest

EPS = ef.EPS
SWEPT = [c for c in ef.CASES if ef.case(c).sweep_positions() is not None]


def test_case_table():
    want = {"g16": (64, 4), "g17": (68, 4), "g144": (576, 4), "g145": (580, 4), "p171": (513, 3), "g550": (2200, 4),
            "l1000": (4000, 4), "h144": (584, 4), "ra": (414, 1)}
    assert set(ef.CASES) == set(want) == set(ef.CASES_DOC)
    for cid, (k, block) in want.items():
        c = ef.case(cid)
        assert (c.k, c.block) == (k, block)
        assert sorted(c.order.tolist()) == list(range(k))
        assert np.array_equal(c.rp[1:] - c.rp[:-1] > 0, np.ones(k, bool)) and c.rp[-1] == c.ci.size
        # symmetric pattern with the whole diagonal, rows sorted
        key = np.repeat(np.arange(k), np.diff(c.rp)).astype(np.int64) * k + c.ci
        assert np.all(np.diff(key) > 0) and np.array_equal(np.sort((key % k) * k + key // k), key)
        assert np.isin(np.arange(k) * (k + 1), key).all()
    assert SWEPT == ["g16", "g17", "g144", "g145", "l1000", "h144", "ra"]
    assert ef.case("l1000").sweep_positions().size == 16 and {0, 3999} <= set(ef.case("l1000").sweep_positions().tolist())
    h = ef.case("h144")  # the hubs come last in L's order, and the library's own rule takes them for hubs (asserted there)
    assert sorted(h.order[h.hub_positions].tolist()) == list(range(576, 584)) and h.hub_threshold >= 48
    assert set(h.hub_positions.tolist()) <= set(h.sweep_positions().tolist())


def test_recorded_numbers_cover_every_case_and_the_generator_rewrites_the_hashes():
    ref = ef.ref()
    assert set(ref) == {(c, a) for c in ef.CASES for a in ef.SCALES}
    spec = importlib.util.spec_from_file_location(
        "make_exact_factors_ref", os.path.join(os.path.dirname(ef.REF_PATH), "make_exact_factors_ref.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for key, h in gen.hashes().items():
        assert ref[key]["sha256"] == h, key
    for (cid, a), r_ in ref.items():
        assert 1.0 <= r_["kappa"] < 1.0 / (1e3 * ef.case(cid).k * EPS), (cid, a)   # room for the sweeps' condition
        for f in ("lapack_solve", "oracle_solve"):   # both references are within the bound set for the device
            assert 0.0 <= r_[f] <= 8.0 * EPS * r_["kappa"], (cid, a, f)
        assert 0.0 <= r_["lapack_logdet"] <= ef.case(cid).k * EPS * r_["sum_abs_log"] + 8.0 * EPS * r_["kappa"]
    assert os.path.getsize(ef.REF_PATH) < 64 * 1024


def test_g16_entry_by_entry_in_python_integers():
    c = ef.case("g16")
    k = c.k
    L4 = [[int(x) for x in row] for row in c.L4.toarray()]
    for a in ef.SCALES:
        for p, neg in ((None, False), (5, True), (5, False)):
            e = c.exponents(a, p)
            dsc = [(-1 if (neg and i == p) else 2 ** int(e[i] + a)) for i in range(k)]
            v = c.values(a, p, neg)
            seen = 0
            for i in range(k):          # L's order
                for j in range(k):
                    s = sum(L4[i][q] * dsc[q] * L4[j][q] for q in range(min(i, j) + 1))
                    u, w = int(c.order[i]), int(c.order[j])
                    at = np.flatnonzero(c.ci[c.rp[u]:c.rp[u + 1]] == w)
                    if at.size == 0:
                        assert s == 0 and all(L4[i][q] == 0 or L4[j][q] == 0 for q in range(k))
                        continue
                    seen += 1
                    assert v[c.rp[u] + at[0]] * (16 << a) == s
            assert seen == c.ci.size


@pytest.mark.parametrize("cid", ef.CASES)
def test_V_is_exact(cid):
    """WV asserts the integer bound and the long double product; here the det and the exponents' range as well"""
    c = ef.case(cid)
    for a in ef.SCALES:
        W, V = c.WV(a, 5)
        assert np.abs(W).max() <= 3 and np.array_equal(W, np.round(W))
        e = c.exponents(a)
        assert e.min() >= -a and e.max() <= a and c.logdet(a) == ef.LN2 * e.sum()
    if cid in SWEPT:
        p = int(c.sweep_positions()[-1])
        c.WV(12, 5, p, True)
        c.WV(12, 5, p, False)
        assert c.logdet(12, p) == ef.LN2 * (c.exponents(12).sum() - c.exponents(12)[p] - 12)


def _potrf_accepts(A):
    return sl.lapack.dpotrf(A, lower=1, overwrite_a=0, clean=0)[1] == 0


@pytest.mark.parametrize("a", ef.SCALES)
@pytest.mark.parametrize("cid", SWEPT)
def test_conditions_of_the_sign_sweeps(cid, a):
    """every negative case: -lambda_min(A) >= 1e3 n eps |A|_2 and LAPACK's potrf refuses it; every positive twin:
    lambda_min >= the same bound and potrf accepts it.  The eigenvalues are bounded, not computed, per position:
    with x = L^-T e_p (x^T A x = D_pp exactly)   lambda_min(A-) <= -2^-a / |x|^2,
    A+^-1 = A^-1 + (2^a - 1 / D_pp) x x^T        lambda_min(A+) >= 1 / (1 / lambda_min(A) + (2^a - 2^-e_p) |x|^2),
    |A+-|_2 <= |A|_2 + |D_pp -+ 2^-a| |L e_p|^2, with lambda_min(A) and |A|_2 of the unswapped matrix from eigvalsh."""
    c = ef.case(cid)
    k = c.k
    A = c.scipy(a).toarray()
    w = np.linalg.eigvalsh(A)
    lam_min, norm2 = w[0], w[-1]
    assert abs(norm2 / lam_min / ef.ref()[(cid, a)]["kappa"] - 1.0) < 1e-6
    L = c.L().toarray()
    ps = c.sweep_positions()
    X = sl.solve_triangular(L, np.eye(k)[:, ps], lower=True, trans="T", unit_diagonal=True)   # columns x_p
    x2 = (X ** 2).sum(axis=0)
    l2 = (L[:, ps] ** 2).sum(axis=0)
    dp = 2.0 ** c.exponents(a)[ps]
    small = 2.0 ** -a
    bound_neg = 1e3 * k * EPS * (norm2 + (dp + small) * l2)
    bound_pos = 1e3 * k * EPS * (norm2 + (dp - small) * l2)
    assert np.all(small / x2 >= bound_neg), (small / x2 / bound_neg).min()
    lam_pos = 1.0 / (1.0 / lam_min + (1.0 / small - 1.0 / dp) * x2)
    assert np.all(lam_pos >= bound_pos), (lam_pos / bound_pos).min()
    order = c.order
    for i, p in enumerate(ps):          # rank-one changes of the dense matrix: u = column p of L in vertex numbering
        u = np.zeros(k)
        u[order] = L[:, p]
        R = np.outer(u, u)
        assert not _potrf_accepts(A - (dp[i] + small) * R), (cid, a, p)
        assert _potrf_accepts(A - (dp[i] - small) * R), (cid, a, p)
    # the rank-one form above is the matrix the GPU tests use, bit for bit (both are exact)
    p = int(ps[len(ps) // 2])
    u = np.zeros(k)
    u[order] = L[:, p]
    assert np.array_equal(A - (dp[len(ps) // 2] + small) * np.outer(u, u), c.scipy(a, p, True).toarray())


# ---- host code against the exact answer ------------------------------------------------------------------------------------
def _host_cases():
    # the plain host loops of the self-test need 14 s at k = 4000: the lattice runs its hardest scale group only
    return [(c, a) for c in ef.CASES for a in ef.SCALES if c != "l1000" or a == 12]


@pytest.mark.parametrize("cid,a", _host_cases())
def test_host_schedule_factors_the_exact_matrix(built, cid, a):
    """chol_host_selftest: max |P A P^T - L L^T| <= 8 max(LAPACK, eps kappa) |A|_max, verdict yes; one swapped pivot: no"""
    import dcora_amd as da
    c = ef.case(cid)
    ok, resid, info = da.chol_host_selftest(c.csr(a), c.block)
    scale = np.abs(c.values(a)).max()
    print("%s a=%d: residual %.2e |A|max, bound %.2e; %s" % (cid, a, resid / scale, ef.tol_solve(cid, a), info))
    assert ok and resid <= ef.tol_solve(cid, a) * scale
    if cid in ("g16", "g17"):
        assert info["pieces"] == 1 and info["levels"] == 1      # one front, of one panel (g17: and one column block)
    if cid == "h144":                                           # the two hubs make one more piece, on a level of its own
        g = da.chol_host_selftest(ef.case("g144").csr(a), 4)[2]
        assert info["pieces"] == g["pieces"] + 1 and info["levels"] == g["levels"] + 1
    if c.k <= 600:                                              # (1.8 s a call at k = 2200)
        for p in c.create_positions():
            assert not da.chol_host_selftest(c.csr(a, p, True), c.block)[0], p
            assert da.chol_host_selftest(c.csr(a, p, False), c.block)[0], p


@pytest.mark.parametrize("cid", ef.CASES)
def test_partitioned_inverse_replayed_on_the_host(built, cid):
    """dcora_debug_partinv_selftest draws its own right-hand sides, so its figure is the replay against the host's
    sparse Cholesky solve (relative, largest entry), not against W; held to the same 8 max(LAPACK, eps kappa)"""
    c = ef.case(cid)
    for a in ef.SCALES:
        for r in ((3, 5, 9) if cid in ("g144", "h144", "ra") else (5,)):
            rc, err, info = _selftest(c.scipy(a), c.block, r)
            print("%s a=%d r=%d: %.2e, bound %.2e" % (cid, a, r, err, ef.tol_solve(cid, a)))
            assert rc == 0 and err <= ef.tol_solve(cid, a)
    if cid in SWEPT:
        for p in c.create_positions():
            assert _selftest(c.scipy(12, p, True), c.block, 5)[0] != 0
            assert _selftest(c.scipy(12, p, False), c.block, 5)[0] == 0


@pytest.mark.parametrize("cid", ["g16", "g144", "h144"])
def test_host_psd_verdicts_on_the_sign_sweeps(built, cid):
    import dcora_amd as da
    c = ef.case(cid)
    for a in ef.SCALES:
        assert da.is_psd(c.csr(a), c.block)
        for p in c.sweep_positions():
            assert not da.is_psd(c.csr(a, int(p), True), c.block), (a, p)
            assert da.is_psd(c.csr(a, int(p), False), c.block), (a, p)
