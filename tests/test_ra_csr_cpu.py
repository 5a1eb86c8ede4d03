"""The helpers of the generic-CSR tests (tests/ra_layouts.py), without a GPU: the populations, kinds, kind borders and
tile structure the variants promise, the extended reference of the mixed manifold against the CPU oracle, and
xq_extended against an exact rational product."""
from fractions import Fraction

import numpy as np
import pytest

import common
import irregular_graphs as ig
import ra_layouts as ra

HUB_FAMILY = ("edges", "edges_sphere", "edges_rot", "deep")


@pytest.mark.parametrize("variant", ra.VARIANTS)
@pytest.mark.parametrize("d", [2, 3])
def test_rows_kinds_and_borders(built, d, variant):
    """graph() asserts the prescribed populations on the row pointers itself; here: what each variant is for"""
    dims, Q, kinds, pops = ra.graph(d, variant)
    _, n, l, b = dims
    c1, c2, c3, k = ra.cols(dims)
    rp = np.asarray(Q.rp, np.int64)
    assert Q.n == k == len(kinds) == len(pops) and np.array_equal(np.diff(rp), pops)
    assert np.all(Q.v != 0)
    A = Q.to_scipy()
    assert abs(A - A.T).max() == 0 and np.all(A.diagonal() > 0)
    assert np.all(kinds[:c1] == ra.ROT) and np.all(kinds[c1:c2] == ra.SPH) and np.all(kinds[c2:c3] == ra.TRA) \
        and np.all(kinds[c3:] == ra.LMK)
    # Q couples rotation columns with Euclidean ones, and spheres with both
    C = A.tocoo()
    pairs = set(zip(kinds[C.row].tolist(), kinds[C.col].tolist()))
    assert {(ra.ROT, ra.TRA), (ra.ROT, ra.LMK), (ra.SPH, ra.TRA), (ra.SPH, ra.ROT), (ra.TRA, ra.LMK)} <= pairs
    w = np.abs(C.data[C.row != C.col])
    assert w.max() / w.min() > 100   # the weights span orders of magnitude
    have = set(pops.tolist())
    assert set(ra.SHORT_POPS) <= have
    for r in range(d, 17):   # the kind borders lie inside a workgroup of k_spmm_dir_fix
        RB = ra.rb_fix(r, d)
        assert RB >= d and c1 % RB != 0 and c2 % RB != 0, (r, RB)
    long = np.flatnonzero(pops > ra.LONG_ROW)
    euclid = kinds[long] >= ra.TRA
    if variant in HUB_FAMILY:
        assert k <= 2200 or variant == "deep"   # kDensePrecondMaxK
        assert {511, 512, 513, 519, 520, 521, 777} <= have
        assert sorted(pops[long[kinds[long] == ra.TRA]].tolist()) == [513, 777]
        assert {513, 519, 520, 521} <= set(pops[long[kinds[long] == ra.LMK]].tolist())
        for r in (2, 16):
            cut, tiles = ra.tile_facts(rp, r)
            assert tiles >= 3, (r, tiles)
            assert any(pops[j] <= ra.LONG_ROW for j in cut), r   # a row the row-parallel walk itself gathers
            for j in cut:   # the statement in its own arithmetic
                RB = ra.K_BLOCK // r
                off = rp[j] - rp[(j // RB) * RB]
                assert any(off < ra.TILE * m < off + pops[j] for m in range(1, 20))
        # slices: per = ceil(len / 8); lengths that are no multiples of 8, a last slice shorter than the others, a slice
        # shorter than the 256 / r entry groups of r = 2 and r = 3
        per = -(-pops[long] // ra.LONG_SPLIT)
        assert np.any(pops[long] % 8 != 0) and np.any(pops[long] % 8 == 0)
        assert np.all(pops[long] - 7 * per > 0) and np.any(pops[long] - 7 * per < per)
        assert per.min() < ra.K_BLOCK // 3
    if variant in ("edges", "deep", "wide"):
        assert euclid.all()
    if variant == "edges_sphere":
        assert pops[long[~euclid]].tolist() == [600] and kinds[long[~euclid]].tolist() == [ra.SPH]
    if variant == "edges_rot":
        (j,) = long[~euclid]
        assert pops[j] == 600 and kinds[j] == ra.ROT and (d == 2 or 0 < j % d < d - 1)
    if variant == "deep":
        per = -(-pops[long] // ra.LONG_SPLIT)
        assert per.max() > 8 * (ra.K_BLOCK // 2) and pops.max() > 8200   # two trips of slice_sum at r = 2
        assert 4100 in have and 4100 // 8 > 8 * (ra.K_BLOCK // 16)        # and more than one at r = 16
        assert 8300 <= k <= 8500
    if variant == "many":
        assert long.size == ra.MANY + 1 > ra.MAX_PARTIALS // 2           # DevCsr::upload gives up the slices
        assert euclid.sum() == ra.MANY and pops[long[euclid]].min() >= 513 and pops[long[euclid]].max() <= 530
        assert len(set(pops[long[euclid]].tolist())) >= 8
        assert {ra.TRA, ra.LMK} <= set(kinds[long].tolist())
        (j,) = long[~euclid]
        assert kinds[j] == ra.ROT and pops[j] > 512
        for r in (2, 16):
            cut, tiles = ra.tile_facts(rp, r)
            assert tiles >= 3 and cut.size > 0
    if variant == "wide":
        assert k >= 15400 and long.size == 1 and pops[long[0]] == 513 and kinds[long[0]] == ra.LMK
        for r in (15, 16):   # the grid-stride second trip of k_spmm_dir_fix
            assert -(-k // ra.rb_fix(r, d)) > ra.MAX_PARTIALS, (r, k)


def _frac(x):
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - np.longdouble(hi)))


def test_xq_extended_against_an_exact_rational_product(built):
    """6 x 6, every entry a double with a full mantissa: X Q + G in exact rationals against the double-double sum"""
    import dcora_amd as da
    import scipy.sparse as sp
    rng = np.random.default_rng(6)
    M = rng.standard_normal((6, 6)) * np.exp(rng.uniform(-20, 20, (6, 6)))
    M[rng.random((6, 6)) < 0.3] = 0.0
    M[0, 0] = 1e16
    M[1, 0], M[2, 0], M[3:, 0] = 1.0, -1e16, 0.0   # cancellation down column 0
    Q = da.Csr.from_scipy(sp.csr_matrix(M))
    X = rng.standard_normal((3, 6))
    X[:, :3] = 1.0
    G = rng.standard_normal((3, 6)) * 1e-5
    G[:, 0] = 0.5
    E = ig.xq_extended(Q, X, G)
    for t in range(3):
        for j in range(6):
            terms = [Fraction(float(X[t, i])) * Fraction(float(M[i, j])) for i in range(6)] + [Fraction(float(G[t, j]))]
            exact, mag = sum(terms), sum(abs(x) for x in terms)
            assert abs(_frac(E[t, j]) - exact) <= Fraction(1, 2 ** 63) * abs(exact) + Fraction(1, 2 ** 100) * mag, (t, j)
    assert E[0, 0] == 1.5   # 0.5 + 1e16 + 1 - 1e16


@pytest.mark.parametrize("d,r", [(2, 4), (3, 5)])
def test_reference_formulas_against_the_oracle(built, d, r):
    """f, the Riemannian gradient, the Hessian product, the tangent projection and the dual certificate of the
    reference are the oracle's on the mixed manifold, to the oracle's rounding"""
    from oracle import orc
    dims, Q, kinds, pops = ra.graph(d, "edges")
    _, n, l, b = dims
    k = Q.n
    rng = np.random.default_rng(50 + d)
    G = rng.standard_normal((r, k))
    X = ra.random_point(orc, r, dims, 51 + d)
    U = rng.standard_normal((r, k))
    V = orc.tangent_project(r, d, n, X, U, l=l, b=b)
    ref = ra.reference(Q, X, G, dims, V=V)
    Po = orc.Problem(r, d, n, Q, G=G, reg=-1, l=l, b=b)
    f64 = lambda M: np.asarray(M, np.float64)
    assert abs(ref["cost2"] - 2 * Po.f(X)) <= 1e-13 * 2 * ref["f_abs"]
    assert common.rel(f64(ref["E"]), Po.egrad(X)) < 1e-13
    assert common.rel(f64(ref["RG"]), Po.rgrad(X)) < 1e-13
    assert common.rel(f64(ref["H"]), Po.hess(X, V)) < 1e-13
    assert common.rel(f64(ra.tangent(X, U, dims)), V) < 1e-13
    # the kinds one by one: an error in one of them must not hide in the norm of all
    c1, c2, c3, _ = ra.cols(dims)
    for lo, hi in ((0, c1), (c1, c2), (c2, c3), (c3, k)):
        assert common.rel(f64(ref["RG"])[:, lo:hi], Po.rgrad(X)[:, lo:hi]) < 1e-13
        assert common.rel(f64(ref["H"])[:, lo:hi], Po.hess(X, V)[:, lo:hi]) < 1e-13
        assert common.rel(f64(ra.tangent(X, U, dims))[:, lo:hi], V[:, lo:hi]) < 1e-13
    assert abs(ref["VH"] - np.sum(V * Po.hess(X, V))) <= 1e-13 * ref["VH_abs"]
    refc = ra.reference(Q, X, None, dims)
    So = orc.dual_certificate(r, d, n, X, Q, l=l, b=b)
    ratio = ra.check_certificate(So, Q, refc, dims, pops, r, (d, r))
    print("oracle certificate: max ratio %.3f" % ratio)
