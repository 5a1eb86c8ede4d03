"""The helpers of the block-CSR tests (tests/irregular_graphs.py), without a GPU: the graph builder's block-row
populations, and the extended-precision reference against scipy in double, against exact integer arithmetic and
against the CPU oracle's gradient and Hessian product."""
import numpy as np
import pytest

import common  # noqa: F401
import irregular_graphs as ig


@pytest.mark.parametrize("n", ig.SIZES)
@pytest.mark.parametrize("variant", ["small", "long"])
@pytest.mark.parametrize("d", [2, 3])
def test_block_row_populations(built, d, variant, n):
    """graph() asserts the populations itself; here: every one the kernels' branches need is present, the hubs sit
    where the chunks of 32 poses begin and end, and a tile boundary of k_fused_hess_bsr cuts a row"""
    ds, Q, pops = ig.graph(d, n, 0, variant)
    assert ds.d == d and ds.n == n and len(pops) == n
    bp, bc = ig.block_rows(Q, d)
    assert np.array_equal(np.diff(bp), pops) and len(bc) == bp[-1]
    assert np.all(ds.vals[:, -1] >= 0.5) and np.all(ds.vals[:, -1] <= 1.5)
    have = set(pops.tolist())
    assert {1, 2, 3, 4, 5, 6, 8, 9, 41} <= have
    assert pops[ig.ISOLATED] == 1 and pops[ig.ISOLATED - 1] == 2 and pops[ig.ISOLATED + 1] == 2
    assert any(p % 4 == 1 and p > 4 for p in have)                      # 4 k + 1: one block left for the last step
    hub = ig.hubs(variant, n)
    assert all(pops[p] == c for p, c in hub.items())
    assert 0 in hub and n - 1 in hub
    if variant == "small":
        assert 100 <= pops.max() <= 127
    else:
        assert {160, 161, 330} <= have
    cuts = ig.cut_rows(bp)
    assert cuts.size > 0
    for i in cuts:   # the statement of the issue, in its own arithmetic
        off = bp[i] - bp[32 * (i // 32)]
        assert any(off < 160 * m < off + pops[i] for m in range(1, 4))
    if variant == "long":
        assert pops[cuts].max() > 160                                       # a row longer than one tile
        assert any(pops[i] <= 160 for i in cuts)                            # and a shorter one that a boundary cuts
    if n == 8193:
        assert (n - 1) % 32 == 0                                            # the last workgroup holds one pose: a hub


def test_agent_split_ranges():
    """the pose ranges of the central evaluation's workgroups: 32 or 33 poses at R = 5, hence two passes of 17"""
    for n, R in ((8193, 1), (8193, 3), (8193, 5), (8193, 7), (8193, 64), (8221, 5), (8192, 5)):
        rg = ig.eval_ranges(n, R)
        sizes = {hi - lo for lo, hi in rg}
        assert rg[0][0] == 0 and rg[-1][1] == n and all(a[1] == b[0] for a, b in zip(rg[:-1], rg[1:]))
        assert sizes <= {31, 32, 33}, (n, R, sizes)
        if R == 5:
            assert 33 in sizes, (n, sizes)


def _rand(rng, r, k):
    return rng.standard_normal((r, k)) * np.exp(rng.uniform(-2, 2, (1, k)))


@pytest.mark.parametrize("d,variant", [(3, "long"), (2, "long"), (3, "small")])
def test_reference_against_scipy_in_double(built, d, variant):
    """every entry of scipy's double product lies within gamma_m A of the reference, m = the terms of the entry"""
    ds, Q, pops = ig.graph(d, 8193, 0, variant)
    rng = np.random.default_rng(3)
    r, k = 5, (d + 1) * ds.n
    X, G = _rand(rng, r, k), _rand(rng, r, k)
    ref = ig.reference(Q, X, G, d)
    A = Q.to_scipy()
    Y = (A.T @ X.T).T + G
    m = np.repeat((d + 1) * pops + 1, d + 1)
    err = np.abs(Y.astype(np.longdouble) - ref["E"]).astype(np.float64)
    bound = ig.gamma(m)[None, :] * ref["A"]
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    assert np.all(ref["E"][:, (d + 1) * ig.ISOLATED:(d + 1) * (ig.ISOLATED + 1)] ==
                  G[:, (d + 1) * ig.ISOLATED:(d + 1) * (ig.ISOLATED + 1)])      # the isolated pose's block of zeros: G alone
    assert abs(ref["cost2"] - (np.sum(Y * X) + np.sum(G * X))) <= 1e-12 * 2 * ref["f_abs"]


def test_reference_is_exact_on_integers(built):
    """integer X, Q and G small enough for exact double arithmetic: the reference equals the integer product"""
    import dcora_amd as da
    import scipy.sparse as sp
    ds, Q, _ = ig.graph(3, 8193, 0, "long")
    rng = np.random.default_rng(4)
    Qi = da.Csr(Q.n, Q.rp, Q.ci, rng.integers(-1000, 1001, Q.nnz).astype(np.float64))
    r = 4
    X = rng.integers(-1000, 1001, (r, Q.n)).astype(np.float64)
    G = rng.integers(-10 ** 6, 10 ** 6, (r, Q.n)).astype(np.float64)
    ref = ig.reference(Qi, X, G, 3)
    A = sp.csr_matrix((Qi.v.astype(np.int64), Qi.ci, Qi.rp), shape=(Q.n, Q.n))
    want = (A.T @ X.astype(np.int64).T).T + G.astype(np.int64)
    assert np.array_equal(ref["E"].astype(np.float64), want.astype(np.float64))
    assert np.all(ref["E"] == want.astype(np.longdouble))
    want_abs = (abs(A).T @ np.abs(X).astype(np.int64).T).T + np.abs(G).astype(np.int64)
    assert np.array_equal(ref["A"], want_abs.astype(np.float64))


def test_reference_sums_cancelling_terms_beyond_double(built):
    """1e16 + 1 - 1e16 down a column: lost in double, kept by the double-double accumulation"""
    import dcora_amd as da
    import scipy.sparse as sp
    Q = da.Csr.from_scipy(sp.csr_matrix(np.array([[1e16, 0.0, 0.0], [1.0, 0.0, 0.0], [-1e16, 0.0, 0.0]])))
    E = ig.xq_extended(Q, np.ones((1, 3)))
    assert E[0, 0] == 1 and E[0, 1] == 0 and E[0, 2] == 0


@pytest.mark.parametrize("d", [2, 3])
def test_reference_formulas_against_the_oracle(built, d):
    """S, RG, H[V], 2 f and the norms of the reference are the oracle's (ref src/QuadraticProblem.cpp), to double"""
    from oracle import orc
    ds, Q, _ = ig.graph(d, 8193, 0, "long")
    r, n = 5, ds.n
    k = (d + 1) * n
    rng = np.random.default_rng(5)
    G = rng.standard_normal((r, k))
    X = orc.project_to_manifold(r, d, n, rng.uniform(-1, 1, (r, k)))
    V = orc.tangent_project(r, d, n, X, rng.standard_normal((r, k)))
    ps = ig.agent_ranges(n, 5)
    ref = ig.reference(Q, X, G, d, V=V, pose_start=ps)
    Po = orc.Problem(r, d, n, Q, G=G)
    f64 = lambda M: np.asarray(M, np.float64)
    assert common.rel(f64(ref["E"]), Po.egrad(X)) < 1e-13
    rg = Po.rgrad(X)
    assert common.rel(f64(ref["RG"]), rg) < 1e-13
    assert common.rel(f64(ref["H"]), Po.hess(X, V)) < 1e-13
    assert abs(ref["cost2"] - 2 * Po.f(X)) <= 1e-12 * abs(ref["cost2"])
    assert abs(ref["gradnorm"] - np.linalg.norm(rg)) <= 1e-12 * ref["gradnorm"]
    dh = d + 1
    for a in range(5):
        want = np.linalg.norm(rg[:, dh * ps[a]:dh * ps[a + 1]])
        assert abs(ref["block_norms"][a] - want) <= 1e-12 * want
