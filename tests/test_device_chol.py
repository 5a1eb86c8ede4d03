"""Device sparse Cholesky behind the PSD test of the certificate (dcora_amd/csrc/device_chol.h; ref
src/DCORA_utils.cpp:1737-1747 isSparseSymmetricMatrixPSD = "CHOLMOD's LL^T succeeds").

CPU: the symbolic analysis (ordering, closed piece structures, scatter map, level / slot schedule) executed by plain
host loops reproduces P A P^T = L L^T.  GPU: verdict against the oracle's and the host factorisation's, log det of
the factored matrix against scipy's sparse LU, on the reference's datasets; the positive verdict at BASELINE config 5's
full size (400 000 unknowns), which the host factorisation cannot deliver.  ONE non-positive pivot, late, in a chosen
structure, and the log-determinant against an exact value: test_exact_factors_gpu.py."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import common


def _Q(da, name):
    ds = common.product_dataset(name)
    return ds, da.build_Q_pgo(ds).to_scipy()


def _logdet(A):
    lu = spl.splu(sp.csc_matrix(A), permc_spec="COLAMD", diag_pivot_thresh=0.0)
    d = lu.U.diagonal()
    assert np.all(d > 0)
    return float(np.sum(np.log(d)))


@pytest.mark.parametrize("name,n,block", [("smallGrid3D", 500, 4), ("sphere2500", 3000, 4), ("sphere2500", 1999, 1)])
def test_symbolic_schedule_on_host(built, name, n, block):
    import dcora_amd as da
    ds, Q = _Q(da, name)
    A = (Q[:n, :n] + sp.identity(n)).tocsr()
    ok, resid, info = da.chol_host_selftest(da.Csr.from_scipy(A), block)
    assert ok and resid <= 1e-12 * abs(A).max()
    assert info["levels"] >= 3 and info["pieces"] >= 5
    okn, _, _ = da.chol_host_selftest(da.Csr.from_scipy((Q[:n, :n] - 5.0 * sp.identity(n)).tocsr()), block)
    assert not okn


def test_symbolic_with_hub_and_disconnected_parts(built):
    import dcora_amd as da
    R = sp.random(600, 600, 0.01, random_state=1)
    A = (R + R.T + 30 * sp.identity(600)).tolil()
    A[599, :] = 0.1   # a hub: coupled to every unknown (a landmark ranged from every pose)
    A[:, 599] = 0.1
    A[599, 599] = 100
    B = sp.block_diag([A.tocsr(), sp.identity(7) * 2.0, A.tocsr()[:50, :50]]).tocsr()  # + disconnected components
    ok, resid, info = da.chol_host_selftest(da.Csr.from_scipy(B), 1)
    assert ok and resid <= 1e-12 * abs(B).max()


def _chain(n, diag=4.0):
    A = sp.diags([np.full(n, diag)], [0]).tolil()
    for i in range(n - 1):
        A[i, i + 1] = A[i + 1, i] = -1.0
    return A.tocsr()


@pytest.mark.parametrize("n", [1, 2, 5, 63, 64, 65, 130])
def test_symbolic_tiny_matrices(built, n):
    import dcora_amd as da
    for block in (1, 4):
        ok, resid, info = da.chol_host_selftest(da.Csr.from_scipy(_chain(n)), block)
        assert ok and resid <= 1e-14
    assert not da.chol_host_selftest(da.Csr.from_scipy(_chain(n, diag=-1.0)), 1)[0]


@pytest.mark.gpu
def test_device_tiny_matrices(built):
    """one column, less than / exactly / just over one 64-column panel, two leaves and a separator"""
    import dcora_amd as da
    for n in (1, 2, 5, 63, 64, 65, 130, 200):
        A = _chain(n)
        pd, info = da.is_psd_device(da.Csr.from_scipy(A), 1, info=True)
        ld = np.linalg.slogdet(A.toarray())[1]
        assert pd and abs(info["logdet"] - ld) <= 1e-12 * max(1.0, abs(ld))
        assert not da.is_psd_device(da.Csr.from_scipy(_chain(n, diag=1.0 if n > 2 else -1.0)), 1)


@pytest.mark.gpu
def test_dense_inverse_built_on_the_device(built):
    """the dense preconditioner (k <= 2200) is formed by the device (LL^T, L^-1, L^-T L^-1): against a direct solve"""
    import dcora_amd as da
    if os.environ.get("DCORA_PRECOND"):
        pytest.skip("DCORA_PRECOND overrides the choice of preconditioner this test is about")
    ds, Q = _Q(da, "sphere2500")
    nb = 330                                    # k = 1320: 20 full panels and one of 40 columns
    Qb = Q[:4 * nb, :4 * nb].tocsr()
    da.precond_cache_clear()
    P = da.QuadraticProblem(5, 3, nb, da.Csr.from_scipy(Qb), reg=0.1)
    assert P.precond_info()["kind"] == "dense"
    rng = np.random.default_rng(3)
    X = da.manifold_project(5, 3, nb, rng.uniform(-1, 1, (5, 4 * nb)))
    V = rng.standard_normal((5, 4 * nb))
    Z = P.PreCondition(X, V)
    M = (Qb + 0.1 * sp.identity(4 * nb)).tocsc()
    want = spl.splu(M).solve(V.T).T
    # PreCondition projects the solve onto the tangent space at X: compare through the projection of the reference
    from oracle import orc
    want = orc.tangent_project(5, 3, nb, X, want)
    assert np.linalg.norm(Z - want) <= 1e-10 * np.linalg.norm(want)
    P.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["smallGrid3D", "sphere2500", "CSAIL"])
def test_chordal_initialisation_with_device_solves(built, name):
    """the two SPD systems of the chordal initialisation (ref src/DCORA_solver.cpp:218-268) solved on the device through
    the partitioned inverse: same start point as with the host factorisation and as the oracle's"""
    import dcora_amd as da
    from oracle import orc
    ds = common.product_dataset(name)
    Th = da.chordal_initialization(ds)
    Td = da.chordal_initialization(ds, device=0)
    assert np.linalg.norm(Td - Th) <= 1e-9 * np.linalg.norm(Th)
    To = orc.chordal_initialization(common.oracle_dataset(name))
    assert np.linalg.norm(Td - To) <= 1e-8 * np.linalg.norm(To)


@pytest.mark.gpu
def test_device_verdict_and_logdet_vs_scipy_and_oracle(built):
    import dcora_amd as da
    from oracle import orc
    for name, shifts in (("smallGrid3D", (1.0, 1e-3, -0.5)), ("sphere2500", (1.0, 1e-3, -0.5, -1e-2))):
        ds, Q = _Q(da, name)
        n = Q.shape[0]
        for sh in shifts:
            A = (Q + sh * sp.identity(n)).tocsr()
            S = da.Csr.from_scipy(A)
            pd, info = da.is_psd_device(S, ds.d + 1, info=True)
            assert pd == da.is_psd(S, ds.d + 1) == orc.is_psd(orc.CSR.from_scipy(A), ds.d + 1) == (sh > 0)
            if pd:
                ld = _logdet(A)
                assert abs(info["logdet"] - ld) <= 1e-10 * abs(ld)
    # a second call on the same pattern reuses the analysis
    pd, info = da.is_psd_device(S, ds.d + 1, info=True)
    assert info["symbolic_ms"] == 0.0


@pytest.mark.gpu
def test_certificate_analysis_prepared_ahead(built):
    """dcora_cert_prepare: the PSD test of the dual certificate analysed from Q's pattern alone (on another thread, as
    dcora_amd/driver.py does): the test that follows finds the analysis, and its verdict and log-determinant are those
    of a test that analysed for itself; pose-graph (SE) and range-aided (RA, block 1) layouts"""
    import threading
    import dcora_amd as da
    cases = []
    ds, Q = _Q(da, "sphere2500")
    X = common.random_point(5, ds.d, ds.n, 7, lambda r_, d_, n_, M: da.manifold_project(r_, d_, n_, M))
    cases.append((da.build_Q_pgo(ds), dict(d=ds.d, n=ds.n, l=0, b=0), ds.d + 1, X, 5))
    ra = da.RADataset(os.path.join(common.DATA, "range_aided_slam_test_3d.pyfg.gz"))
    rng = np.random.default_rng(3)
    cases.append((ra.Q, dict(d=ra.d, n=ra.n, l=ra.l, b=ra.b), 1, None, 4))
    for Qc, dm, block, X, r in cases:
        if X is None:
            k = Qc.n
            X = rng.standard_normal((r, k))
        S = da.dual_certificate(r, dm["d"], dm["n"], X, Qc, l=dm["l"], b=dm["b"])
        # S + shift I made positive definite WITHOUT touching the pattern (scipy's sum would drop S's explicit zeros;
        # the library's own fastVerification shifts the diagonal in place as well)
        Ssp = S.to_scipy()
        shift = 10.0 * abs(Ssp).sum(axis=1).max()
        A = da.Csr(S.n, S.rp.copy(), S.ci.copy(), S.v.copy())
        rows = np.repeat(np.arange(S.n), np.diff(S.rp))
        diag = np.flatnonzero(rows == S.ci)
        assert diag.size == S.n
        A.v[diag] += shift
        da.chol_cache_clear()
        pd0, info0 = da.is_psd_device(A, block, info=True)
        assert pd0 and info0["symbolic_ms"] > 0.0
        da.chol_cache_clear()
        t = threading.Thread(target=da.cert_prepare, args=(Qc, dm["d"], dm["n"]),
                             kwargs=dict(l=dm["l"], b=dm["b"], block=block))
        t.start()
        t.join()
        pd1, info1 = da.is_psd_device(A, block, info=True)
        assert pd1 and info1["symbolic_ms"] == 0.0, "the prepared analysis was not found"
        assert abs(info1["logdet"] - info0["logdet"]) <= 1e-12 * abs(info0["logdet"])


@pytest.mark.gpu
def test_device_verdict_tiers_with_hub(built):
    import dcora_amd as da
    ra = da.RADataset(os.path.join(common.DATA, "tiers.pyfg.gz"))
    Q = ra.Q.to_scipy()
    n = Q.shape[0]
    A = (Q + sp.identity(n)).tocsr()
    pd, info = da.is_psd_device(da.Csr.from_scipy(A), 1, info=True)
    ld = _logdet(A)
    assert pd and abs(info["logdet"] - ld) <= 1e-10 * abs(ld)
    assert not da.is_psd_device(da.Csr.from_scipy((Q - 1e-2 * sp.identity(n)).tocsr()), 1)


@pytest.mark.gpu
def test_device_verdict_config5_full_size(built):
    """the whole 100k-pose lattice (k = 400 000): positive and negative verdicts of the complete factorisation"""
    import dcora_amd as da
    from dcora_amd import synth
    ds = synth.lattice_se3()
    Q = da.build_Q_pgo(ds).to_scipy()
    n = Q.shape[0]
    assert n == 400000
    pd, info = da.is_psd_device(da.Csr.from_scipy((Q + 1e-3 * sp.identity(n)).tocsr()), 4, info=True)
    assert pd and info["flops"] > 5e11  # (1.94e12 with whole BFS levels as separators, 0.92e12 with vertex covers)
    # log det against the sum over a 2 x 2 block split?  no closed form: check the factor through the shift instead:
    # Q is PSD with a 1-dimensional kernel per connected component => Q - eps I is indefinite for every eps > 0
    assert not da.is_psd_device(da.Csr.from_scipy((Q - 1e-6 * sp.identity(n)).tocsr()), 4)
