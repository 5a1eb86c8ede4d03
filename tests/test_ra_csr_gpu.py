"""The generic CSR kernels -- k_spmm<DOTS>, k_spmm_dir, k_spmm_dir_fix<D> with the row walk of csr_rows.h, and k_rgrad,
k_tangent, k_hessfix over the mixed manifold -- against an extended-precision reference on range-aided layouts built
for the edges of the row walk (tests/ra_layouts.py): rows of 1, 2, 7, 8, 9, 16, 17, 511 and 512 entries, long rows of
513, 519, 520, 521 and 777 entries in landmark and translation columns (edges), a long row in a unit-sphere column
(edges_sphere) or a rotation column (edges_rot), slices of more than 8 x 256 / r entries (deep: 4100 and > 8200), more
than 512 long rows (many: DevCsr::upload gives up the slices, rows of any length take the tiles), and more than 1024
row blocks (wide: the second grid trip of k_spmm_dir_fix).  Every test first asserts the path it means to take.

A. Q-apply per entry: |y - y_ref| <= gamma_m A, A = |X| |Q| + |G|, m = (entries of the row) + 1 -- the forward bound of
   an m-term sum in any order, with or without FMA.  f within 1e-11 f_abs (the project's figure).  Every call is made
   twice on the same handle and must repeat bit for bit (arrival counters, order of the slices).
B. RieGrad, projectToTangentSpace and HessVec (k_spmm + k_hessfix) per item -- rotation block, sphere, translation,
   landmark -- grouped by (kind, population; a rotation block counts with the longest row of its columns): the
   device's largest error in a group is at most 8 x max(the CPU oracle's largest error in that group, u x the group's
   absolute-sum scale), the rule of test_block_factors_gpu.py and test_block_csr_gpu.py.
C. HessVecSolverForm (k_spmm_dir_fix, iteration 0) where it applies (edges, deep, many, wide): H under the rule of B,
   both dots within gamma_M sum |V| |terms of H| of the reference's <V, H>, M = r k + max population + 2 d (r + 1) + 2:
   the r k products of the dot, and per entry of H the row's terms of V Q, the d of V S, the 2 r d products and d means
   of sym(Y^T T), the d of Y S2 (a bound on the count, not the count of every entry).  It must raise DcoraError on
   edges_sphere and edges_rot.
D. RTR with DCORA_SOLVER=generic against the oracle: edges (one-launch form), edges_sphere and edges_rot (k_spmm_dir +
   k_hessfix), deep on the sparse preconditioner; one RTR iteration of 1, 2 and 3 tCG iterations from a warm start and
   3 x 10 from a trust region in which a step is rejected, with and without G.  The project's tolerances: fInit and
   gradNormInit 1e-12, fOpt 1e-9 relative, per-item |X - X_oracle| 1e-7, equal iteration counts.
E. dual_certificate on edges and many at r = d + 1: every entry of Lambda within gamma_m (its absolute sum + |Q
   entry|), m = population + r + 3; the entries of Q carried over bit for bit.

The sparse preconditioner of `deep` keeps its hubs out of the level replay, so the solves of D on it end every tCG
iteration in k_tangent's folded form with hub columns; no entry point tells, and the test does not assert it.

Largest observed on an MI355X (profiles/ra_csr.txt holds every figure; the module's 107 tests take 12 s after the
session's build fixture, test_block_csr_gpu.py about 30 s):
A  max |y - y_ref| / (gamma_m A) (bound 1): edges 0.510 (d = 2) 0.482 (d = 3), deep 0.481 / 0.510, many 0.502 / 0.460,
   wide 0.587 / 0.562, always in a row of 1 to 10 entries, where gamma_m is smallest; |f - f_ref| / f_abs <= 1.5e-16
   (bound 1e-11).
B  device error / max(oracle error, u scale) over the groups (bound 8), edges / edges_sphere / edges_rot / deep / many /
   wide: RieGrad 3.50 / 1.88 / 2.06 / 2.46 / 1.66 / 1.69, projectToTangentSpace 0.89 / 0.97 / 1.00 / 1.00 / 1.20 / 1.00,
   HessVec 3.30 / 2.86 / 2.19 / 1.62 / 1.61 / 1.19.  On Euclidean columns the device's HessVec error equals the oracle's.
C  H of the one-launch form: 3.30 / 1.62 / 1.61 / 1.19 (edges / deep / many / wide), the figures of HessVec; its dots
   within 2.2e-4 of the bound, both forms.
D  per-item |X - X_oracle| <= 6.3e-13; fInit 1.0e-14, gradNormInit 3.9e-13, fOpt 4.0e-14 relative; equal counts throughout.
E  0.125 of the bound.
No group exceeds 8 x.

Value-only changes of the kernels, made locally one at a time, and the tests of this module that fail with them:
  slice_sum stops one entry early (pp < s.pe - 1): 88 -- all of A, B/C and D but the `many` cases (no slices there)
  gather_tile puts its padding weight on the segment's first entry: all 107
  the kind == 1 term of k_spmm_dir_fix dropped: 30 -- B/C (the one-launch H) on edges, deep, many, wide; D on edges, deep
  the `first` prologue values of k_spmm_dir_fix on every trip: the 4 cases of B/C on wide
  slices_total adds 7 slices: the same 88
  the long row's p1 slot written at main_grid: 17 to 20 -- the dots of C on edges and deep (all 10 of deep), D on edges and
    deep; the slots left unwritten keep what the memory held, so on edges the count varies from run to run
"""
import os

import numpy as np
import pytest

import irregular_graphs as ig
import ra_layouts as ra

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ONE_LAUNCH = ("edges", "deep", "many", "wide")


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


def _on_generic_csr(P, precond):
    assert P.qapply_info()["kernel"] == "k_spmm", P.qapply_info()
    assert P.precond_info()["kind"] == precond, P.precond_info()


# ---- A -------------------------------------------------------------------------------------------------------------------
def _cases_a():
    """edges at every r from d to 16; deep at r = 2, 3, 16, many at r = 2, 5, 16, wide at r = 15, 16 (r = 2 at d = 2 alone:
    r >= d)"""
    out = [("edges", d, r) for d in (2, 3) for r in range(d, 17)]
    out += [("deep", 2, 2), ("deep", 2, 3), ("deep", 2, 16), ("deep", 3, 3), ("deep", 3, 16)]
    out += [("many", 2, 2), ("many", 2, 5), ("many", 2, 16), ("many", 3, 5), ("many", 3, 16)]
    out += [("wide", d, r) for d in (2, 3) for r in (15, 16)]
    return out


@pytest.mark.parametrize("variant,d,r", _cases_a())
def test_q_apply_entries_within_the_forward_bound(env, variant, d, r):
    da, orc = env
    dims, Q, kinds, pops = ra.graph(d, variant)
    _, n, l, b = dims
    k = Q.n
    rng = np.random.default_rng(1000 * d + 10 * r + ra.VARIANTS.index(variant))
    X = rng.standard_normal((r, k)) * np.exp(rng.uniform(-1, 1, (1, k)))
    G = rng.standard_normal((r, k)) * np.exp(rng.uniform(-1, 5, (1, k)))
    gam = ig.gamma(pops + 1)[None, :]
    P = da.QuadraticProblem(r, d, n, Q, G=G, reg=-1, l=l, b=b)
    try:
        _on_generic_csr(P, "none")
        XQ = None
        for name, g in (("G", G), ("no G", None)):
            P.set_linear_term(g)
            ref = ra.reference(Q, X, g, dims, XQ=XQ)
            XQ = ref["XQ"]
            y = P.EucGrad(X)
            f = P.f(X)
            assert np.array_equal(P.EucGrad(X), y) and P.f(X) == f, (variant, d, r, name, "the second call differs")
            err = np.abs(y.astype(np.longdouble) - ref["E"]).astype(np.float64)
            bound = gam * ref["A"]
            ratio = err / bound
            j = int(np.argmax(ratio.max(axis=0)))
            print("RATIO A %-5s d=%d r=%2d %-4s max |y - y_ref| / (gamma_m A) = %.3f (column %d, %s, %d entries); "
                  "f: |f - f_ref| / f_abs = %.2e" % (variant, d, r, name, ratio.max(), j, ra.KIND_NAMES[kinds[j]], pops[j],
                                                     abs(f - 0.5 * ref["cost2"]) / ref["f_abs"]))
            assert np.all(err <= bound), (variant, d, r, name, float(ratio.max()), j)
            assert abs(f - 0.5 * ref["cost2"]) <= 1e-11 * ref["f_abs"], (variant, d, r, name)
    finally:
        P.close()


# ---- B and C -------------------------------------------------------------------------------------------------------------
def _cases_b():
    out = []
    for variant in ra.VARIANTS:
        for d in (2, 3):
            rs = (15, 16) if variant == "wide" else sorted({d, d + 2, 7, 9, 16})
            out += [(variant, d, r) for r in rs]
    return out


def _operands(orc, variant, d, r):
    """(dims, Q, kinds, pops, G, X, Uv, V, ref, refT, absT, the oracle's results) of a case of B and C"""
    dims, Q, kinds, pops = ra.graph(d, variant)
    _, n, l, b = dims
    k = Q.n
    rng = np.random.default_rng(2000 * d + 10 * r + ra.VARIANTS.index(variant))
    G = rng.standard_normal((r, k))
    X = ra.random_point(orc, r, dims, 20 + r)
    Uv = rng.standard_normal((r, k))
    V = orc.tangent_project(r, d, n, X, Uv, l=l, b=b)
    Po = orc.Problem(r, d, n, Q, G=G, reg=-1, l=l, b=b)
    return (dims, Q, kinds, pops, G, X, Uv, V, ra.reference(Q, X, G, dims, V=V), ra.tangent(X, Uv, dims),
            ra.tangent_abs(X, Uv, dims), dict(rgrad=Po.rgrad(X), hess=Po.hess(X, V)))


def _check_groups(what, dev_err, orc_err, scale, groups):
    """per (kind, population): device max error <= 8 max(oracle max error, u scale); prints every ratio"""
    kind, pop = groups
    worst, bad = 0.0, []
    for g in np.unique(kind * 100000 + pop):
        sel = (kind * 100000 + pop) == g
        tol = max(orc_err[sel].max(), U * scale[sel].max())
        ratio = dev_err[sel].max() / tol
        line = "%s  %-11s %5d entries (%4d items): device %.3e oracle %.3e u.scale %.3e ratio %.2f" % (
            what, ra.KIND_NAMES[g // 100000], g % 100000, sel.sum(), dev_err[sel].max(), orc_err[sel].max(),
            U * scale[sel].max(), ratio)
        print(line)
        worst = max(worst, ratio)
        if not dev_err[sel].max() <= 8 * tol:
            bad.append(line)
    print("RATIO %s max %.2f" % (what, worst))
    assert not bad, "device error above 8 x max(oracle error, u scale):\n" + "\n".join(bad)


@pytest.mark.parametrize("variant,d,r", _cases_b())
def test_operators_per_item_and_the_one_launch_hessian(env, variant, d, r):
    da, orc = env
    dims, Q, kinds, pops, G, X, Uv, V, ref, refT, absT, oracle = _operands(orc, variant, d, r)
    _, n, l, b = dims
    groups = ra.item_groups(dims, kinds, pops)
    P = da.QuadraticProblem(r, d, n, Q, G=G, reg=-1, l=l, b=b)
    try:
        _on_generic_csr(P, "none")
        tag = "%-12s d=%d r=%2d" % (variant, d, r)
        rg = P.RieGrad(X)
        _check_groups("B RieGrad " + tag, ra.item_err(rg, ref["RG"], dims), ra.item_err(oracle["rgrad"], ref["RG"], dims),
                      ra.item_max(ref["A"], dims), groups)
        _check_groups("B tangent " + tag, ra.item_err(P.projectToTangentSpace(X, Uv), refT, dims),
                      ra.item_err(V, refT, dims), ra.item_max(absT, dims), groups)
        hv = P.HessVec(X, V)
        _check_groups("B HessVec " + tag, ra.item_err(hv, ref["H"], dims), ra.item_err(oracle["hess"], ref["H"], dims),
                      ra.item_max(ref["AV"], dims), groups)
        assert np.array_equal(P.RieGrad(X), rg) and np.array_equal(P.HessVec(X, V), hv), (tag, "the second call differs")
        gn = P.RieGradNorm(X)
        assert abs(gn - ref["gradnorm"]) <= 1e-10 * ref["gradnorm"]
        # ---- C ----
        k = Q.n
        long = np.flatnonzero(pops > ra.LONG_ROW)
        if variant not in ONE_LAUNCH:   # a long row that is no Euclidean column: k_spmm_dir + k_hessfix it must be
            assert np.any(kinds[long] < ra.TRA)
            with pytest.raises(da.DcoraError):
                P.HessVecSolverForm(X, V)
            return
        assert np.all(kinds[long] >= ra.TRA) or long.size > ra.MAX_PARTIALS // 2
        if variant == "wide":
            assert -(-k // ra.rb_fix(r, d)) > ra.MAX_PARTIALS   # the second grid trip
        tag = "%-12s d=%d r=%2d" % (variant, d, r)
        H, dots = P.HessVecSolverForm(X, V)
        _check_groups("C one launch " + tag, ra.item_err(H, ref["H"], dims), ra.item_err(oracle["hess"], ref["H"], dims),
                      ra.item_max(ref["AV"], dims), ra.item_groups(dims, kinds, pops))
        M = r * k + int(pops.max()) + 2 * d * (r + 1) + 2
        bound = ig.gamma(M) * ref["VH_abs"]
        print("RATIO C dots %s: |dot - <V, H>| / (gamma_M sum |V| |H terms|) = %.2e (one launch) %.2e (two launches), M = %d"
              % (tag, abs(dots[0] - ref["VH"]) / bound, abs(dots[1] - ref["VH"]) / bound, M))
        assert abs(dots[0] - ref["VH"]) <= bound and abs(dots[1] - ref["VH"]) <= bound, (tag, dots, ref["VH"], bound)
        H2, dots2 = P.HessVecSolverForm(X, V)   # the arrival counters are back at zero, the long rows' slots where they were
        assert np.array_equal(H2, H) and np.array_equal(dots2, dots), (tag, "the second call differs")
    finally:
        P.close()


# ---- D -------------------------------------------------------------------------------------------------------------------
def _problem(da, r, dims, Q, G, reg=0.1):
    d, n, l, b = dims
    os.environ["DCORA_SOLVER"] = "generic"
    try:
        return da.QuadraticProblem(r, d, n, Q, G=G, reg=reg, l=l, b=b)
    finally:
        os.environ.pop("DCORA_SOLVER", None)


def _item_dist(X, Y, dims):
    d, n, l, b = dims
    D2 = ((X - Y) ** 2).sum(axis=0)
    return float(np.sqrt(np.r_[D2[:n * d].reshape(n, d).sum(axis=1), D2[n * d:]]).max())


# (start, parameters): one RTR iteration of 1, 2 and 3 tCG iterations from a warm start -- the oracle's iterate after
# 30 x 50, from where every run ends on its iteration limit -- and 3 x 10 from the random point with a trust region
# from which the oracle refuses a step and accepts another (asserted below)
REJECT_RADIUS = 300.0
SOLVES = [("warm", dict(RTR_iterations=1, RTR_tCG_iterations=1)), ("warm", dict(RTR_iterations=1, RTR_tCG_iterations=2)),
          ("warm", dict(RTR_iterations=1, RTR_tCG_iterations=3)),
          ("cold", dict(RTR_iterations=3, RTR_tCG_iterations=10, RTR_initial_radius=REJECT_RADIUS))]
KEYS = (("outer_iterations", "outer_iters"), ("inner_iterations", "inner_iters"), ("accepted_steps", "accepted"),
        ("tCGStatus", "tcg_status"))
# (variant, d, r, preconditioner, the warm start's RTR x tCG iterations: at r = 16 the oracle has converged after 30 x 50)
SOLVE_CASES = [("edges", 3, 5, "dense", (30, 50)), ("edges", 2, 4, "dense", (30, 50)),
               ("edges_sphere", 3, 5, "dense", (30, 50)), ("edges_rot", 3, 5, "dense", (30, 50)),
               ("edges_rot", 2, 16, "dense", (10, 20)), ("deep", 3, 5, "sparse", (30, 50))]


@pytest.mark.parametrize("variant,d,r,precond,warm", SOLVE_CASES)
def test_generic_solves_against_the_oracle(env, variant, d, r, precond, warm):
    da, orc = env
    dims, Q, kinds, pops = ra.graph(d, variant)
    _, n, l, b = dims
    k = Q.n
    rng = np.random.default_rng(3000 * d + 10 * r + ra.VARIANTS.index(variant))
    G = rng.standard_normal((r, k))
    X = ra.random_point(orc, r, dims, 30 + r)
    P = _problem(da, r, dims, Q, G)
    try:
        _on_generic_csr(P, precond)
        assert (precond == "dense") == (k <= 2200)
        V = orc.tangent_project(r, d, n, X, rng.standard_normal((r, k)), l=l, b=b)
        if variant in ONE_LAUNCH:   # the solver's Hessian product is k_spmm_dir_fix
            P.HessVecSolverForm(X, V)
        else:                       # k_spmm_dir + k_hessfix
            with pytest.raises(da.DcoraError):
                P.HessVecSolverForm(X, V)
        rejected = 0
        for g in (G, None):
            P.set_linear_term(g)
            Po = orc.Problem(r, d, n, Q, G=g, reg=0.1, l=l, b=b)
            Xw, _ = Po.optimize(X, RTR_iterations=warm[0], RTR_tCG_iterations=warm[1])
            for where, kw in SOLVES:
                X0 = Xw if where == "warm" else X
                opt = da.QuadraticOptimizer(P, da.ROptParameters(**kw))
                Xs = opt.optimize(X0)
                res = opt.getOptResult()
                Xo, reso = Po.optimize(X0, **kw)
                tag = (variant, d, r, g is not None, kw)
                print("D %s: outer %d inner %d accepted %d status %d; per-item |X - X_oracle| %.2e; fInit %.1e "
                      "gradNormInit %.1e fOpt %.1e" % (
                          tag, res["outer_iterations"], res["inner_iterations"], res["accepted_steps"], res["tCGStatus"],
                          _item_dist(Xs, Xo, dims), abs(res["fInit"] / reso["fInit"] - 1),
                          abs(res["gradNormInit"] / reso["gradNormInit"] - 1), abs(res["fOpt"] / reso["fOpt"] - 1)))
                for key, okey in KEYS:
                    assert res[key] == reso[okey], (tag, key, res[key], reso[okey])
                if where == "warm":   # (the gather of every iteration after the first ran)
                    assert res["inner_iterations"] == kw["RTR_tCG_iterations"], tag
                assert abs(res["fInit"] - reso["fInit"]) <= 1e-12 * abs(reso["fInit"]), tag
                assert abs(res["gradNormInit"] - reso["gradNormInit"]) <= 1e-12 * reso["gradNormInit"], tag
                assert abs(res["fOpt"] - reso["fOpt"]) <= 1e-9 * abs(reso["fOpt"]), tag
                assert _item_dist(Xs, Xo, dims) <= 1e-7, tag
                if where == "cold":
                    rejected += 0 < reso["accepted"] < reso["outer_iters"]
        assert rejected == 2, "no step was refused and another accepted in the 3 x 10 runs"
        _on_generic_csr(P, precond)
    finally:
        P.close()


# ---- E -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["edges", "many"])
@pytest.mark.parametrize("d", [2, 3])
def test_dual_certificate_entries(env, variant, d):
    da, orc = env
    r = d + 1
    dims, Q, kinds, pops = ra.graph(d, variant)
    _, n, l, b = dims
    X = ra.random_point(orc, r, dims, 40 + d)
    ref = ra.reference(Q, X, None, dims)
    assert pops.max() > ra.LONG_ROW   # the certificate's Q-apply walks long rows (k_spmm through DevCsr::upload)
    S = da.dual_certificate(r, d, n, X, Q, l=l, b=b)
    ratio = ra.check_certificate(S, Q, ref, dims, pops, r, (variant, d))
    S2 = da.dual_certificate(r, d, n, X, Q, l=l, b=b)
    assert np.array_equal(S.rp, S2.rp) and np.array_equal(S.ci, S2.ci) and np.array_equal(S.v, S2.v)
    print("RATIO E %-5s d=%d r=%d max |Lambda - Lambda_ref| / (gamma_m abs) = %.3f" % (variant, d, r, ratio))
