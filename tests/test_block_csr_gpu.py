"""The block-CSR kernels (pose graphs of 8192 poses or more, SE layout, r <= 8) against an extended-precision reference
on irregular graphs (tests/irregular_graphs.py): k_spmm_bsrq<D, R, DOTS, GRAD> as the Q-apply, as the evaluation of an
RTR iteration and as the central evaluation of a session with its agent split; k_fused_hess_bsr<D> inside the fused
solve; DeviceProblem::set_values restaging the block values.  Every shape reaches the kernels through the production
rule n >= 8192, and every test first asserts the path the device took.

A. Q-apply, all 13 (d, r), `long` graph, n = 8193: per entry |y_dev - y_ref| <= gamma_m A, A = |X| |Q| + |G|,
   m = (d+1) blocks + 1 terms -- the forward bound of an m-term sum in any order, with or without FMA.
B. RieGrad and HessVec per pose, grouped by block-row population: the device's largest error in a group is at most
   8 x max(the CPU oracle's error in that group, u x the group's absolute-sum scale) (the rule of
   test_block_factors_gpu.py).  RieGrad is the block Q-apply followed by the per-pose projection; HessVec of the
   problem handle takes the scalar CSR of Q (k_spmm + k_hessfix) whatever the size: the block Hessian product
   k_fused_hess_bsr is reached through the solves of C alone.
C. RTR solves on the fused form with the block evaluation against the oracle and against DCORA_SOLVER=generic (CSR, no
   block form): 1, 2 and 3 tCG iterations of one RTR iteration (H[-z0], then the beta d_old - z gather), with and
   without G, and 3 x 10 from a trust region where a step is rejected (the `cur` buffer switch).  Both variants keep a
   fused form: n <= 24576 poses (fused_supported), the preconditioner is sparse (k > 2200), hence "three launches",
   and the long rows of the `long` variant matter to the scalar CSR kernels alone (RtrForm::gfb does not ask).
D. RbcdSession.evaluate() with the agent split, R = 1, 3, 5, 7, 64, and RBCD iterations of two agents of 8200 poses.
E. set_weights on the block form, central and agent.

Tolerances of C, D and E are the project's: fInit, gradNormInit 1e-12 and fOpt 1e-9 relative (f, RieGrad and fOpt of
test_planar_lattice_on_the_block_structure), per-pose |X_i - Xref_i| 1e-9 between device paths and 1e-7 against the
oracle (test_fuzz_paths_gpu.py); cost2 1e-11, gradnorm and block norms 1e-10.  The central problem of a session has no
handle of its own: a problem created the way the session creates it states its Q-apply.  The go.posenorm branch of
launch_fused_grad_bsr without agent_start has no caller and is not tested.

Largest observed ratios on an MI355X, per entry point.
A, EucGrad, max |y - y_ref| / (gamma_m A) (bound 1), with G / without; the worst entry always sits in a short row (2 or 3
blocks, m = 9 .. 13), where gamma_m is smallest:
  d=3  r=3 0.306 / 0.307   r=4 0.303 / 0.287   r=5 0.352 / 0.314   r=6 0.359 / 0.381   r=7 0.311 / 0.300   r=8 0.257 / 0.260
  d=2  r=2 0.431 / 0.444   r=3 0.539 / 0.651   r=4 0.367 / 0.454   r=5 0.348 / 0.388   r=6 0.474 / 0.515   r=7 0.490 / 0.510
       r=8 0.389 / 0.378
   f: |f - f_ref| / sum |terms| <= 8.4e-17 (bound 1e-11)
B, device error / max(oracle error, u scale) over the groups (bound 8), small / long variant:
  RieGrad  d=3 r=3 1.30 / 1.80   r=5 1.14 / 2.82   r=7 1.27 / 1.17   r=8 1.00 / 1.59   d=2 r=2 1.17 / 1.13   r=7 1.57 / 1.56
  HessVec  d=3 r=3 1.09 / 1.00   r=5 1.44 / 1.59   r=7 1.25 / 1.31   r=8 2.12 / 1.49   d=2 r=2 1.00 / 2.53   r=7 2.26 / 2.51
C: per-pose |X - X_generic| <= 6.6e-14, |X - X_oracle| <= 1.3e-11; fInit, gradNormInit, fOpt within 3.2e-14 relative.
D, E: cost2, gradnorm and block norms within 1.1e-15 relative; the two-agent trace within 6e-14.

Value-only changes of the kernels, made locally one at a time, and the tests that fail with them:
  k_spmm_bsrq drops the last block of a row of 4 k + 1 blocks: all 48 tests of this module
  k_fused_hess_bsr starts a cut row at lo + 1: the 14 cases of test_fused_solve_on_the_block_form,
    test_two_agents_on_the_block_form and test_reweighting_restages_the_block_values[1]
  set_values skips the block restage: both cases of test_reweighting_restages_the_block_values
"""
import os

import numpy as np
import pytest

import common
import irregular_graphs as ig

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DR = [(3, r) for r in range(3, 9)] + [(2, r) for r in range(2, 9)]


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


def _point(orc, r, d, n, seed):
    return common.random_point(r, d, n, seed, orc.project_to_manifold)


def _on_block_form(P):
    assert P.qapply_info()["kernel"] == "k_spmm_bsrq", P.qapply_info()


# ---- A -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,r", DR)
def test_q_apply_entries_within_the_forward_bound(env, d, r):
    da, orc = env
    n = 8193
    ds, Q, pops = ig.graph(d, n, 0, "long")
    k = (d + 1) * n
    rng = np.random.default_rng(100 * d + r)
    X = rng.standard_normal((r, k)) * np.exp(rng.uniform(-1, 1, (1, k)))
    G = rng.standard_normal((r, k)) * np.exp(rng.uniform(-1, 5, (1, k)))
    gam = ig.gamma(np.repeat((d + 1) * pops + 1, d + 1))[None, :]
    P = da.QuadraticProblem(r, d, n, Q, G=G, reg=-1)
    try:
        _on_block_form(P)
        assert P.precond_info()["kind"] == "none"
        worst = {}
        for name, g in (("G", G), ("no G", None)):
            P.set_linear_term(g)
            ref = ig.reference(Q, X, g, d)
            err = np.abs(P.EucGrad(X).astype(np.longdouble) - ref["E"]).astype(np.float64)
            bound = gam * ref["A"]   # (0 on the isolated pose without G: there the device must return 0)
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
            worst[name] = float(ratio.max())
            j = int(np.argmax(ratio.max(axis=0)))
            print("RATIO A d=%d r=%d %-4s max |y - y_ref| / (gamma_m A) = %.3f (pose %d, %d blocks)" %
                  (d, r, name, worst[name], j // (d + 1), pops[j // (d + 1)]))
            assert np.all(err <= bound), (d, r, name, worst[name])
            f = P.f(X)
            print("        f: |f - f_ref| / sum |terms| = %.2e" % (abs(f - 0.5 * ref["cost2"]) / ref["f_abs"]))
            assert abs(f - 0.5 * ref["cost2"]) <= 1e-11 * ref["f_abs"], (d, r, name)
    finally:
        P.close()


# ---- B -------------------------------------------------------------------------------------------------------------------
def _check_groups(what, dev_err, orc_err, scale, pops):
    """per population: device max error <= 8 max(oracle max error, u scale); prints every ratio, returns the largest"""
    worst, bad = 0.0, []
    for g in np.unique(pops):
        sel = pops == g
        tol = max(orc_err[sel].max(), U * scale[sel].max())
        ratio = dev_err[sel].max() / tol
        line = "%s  %4d blocks (%4d poses): device %.3e oracle %.3e u.scale %.3e ratio %.2f" % (
            what, g, sel.sum(), dev_err[sel].max(), orc_err[sel].max(), U * scale[sel].max(), ratio)
        print(line)
        worst = max(worst, ratio)
        if not dev_err[sel].max() <= 8 * tol:
            bad.append(line)
    print("RATIO B %s max %.2f" % (what, worst))
    assert not bad, "device error above 8 x max(oracle error, u scale):\n" + "\n".join(bad)


@pytest.mark.parametrize("variant", ["small", "long"])
@pytest.mark.parametrize("d,r", [(3, 3), (3, 5), (3, 7), (3, 8), (2, 2), (2, 7)])
def test_riegrad_and_hessvec_per_pose(env, d, r, variant):
    da, orc = env
    n = 8193
    ds, Q, pops = ig.graph(d, n, 0, variant)
    k = (d + 1) * n
    rng = np.random.default_rng(200 * d + r)
    G = rng.standard_normal((r, k))
    X = _point(orc, r, d, n, 20 + r)
    V = orc.tangent_project(r, d, n, X, rng.standard_normal((r, k)))
    ref = ig.reference(Q, X, G, d, V=V)
    Po = orc.Problem(r, d, n, Q, G=G)
    P = da.QuadraticProblem(r, d, n, Q, G=G, reg=-1)
    try:
        _on_block_form(P)
        tag = "d=%d r=%d %-5s" % (d, r, variant)
        _check_groups("RieGrad " + tag, ig.pose_err(P.RieGrad(X), ref["RG"], d), ig.pose_err(Po.rgrad(X), ref["RG"], d),
                      ig.pose_max(ref["A"], d), pops)
        _check_groups("HessVec " + tag, ig.pose_err(P.HessVec(X, V), ref["H"], d), ig.pose_err(Po.hess(X, V), ref["H"], d),
                      ig.pose_max(ref["AV"], d), pops)
        gn = P.RieGradNorm(X)
        assert abs(gn - ref["gradnorm"]) <= 1e-10 * ref["gradnorm"]
    finally:
        P.close()


# ---- C -------------------------------------------------------------------------------------------------------------------
def _problem(da, r, d, n, Q, G, solver=None):
    if solver:
        os.environ["DCORA_SOLVER"] = solver
    try:
        return da.QuadraticProblem(r, d, n, Q, G=G, reg=0.1)
    finally:
        os.environ.pop("DCORA_SOLVER", None)


def _pose_dist(X, Y, d):
    r = X.shape[0]
    D = (X - Y).reshape(r, -1, d + 1).transpose(1, 0, 2)
    return np.sqrt((D * D).sum(axis=(1, 2))).max()


# (start, parameters): one RTR iteration of 1, 2 and 3 tCG iterations from a warm start -- the oracle's iterate after
# 10 x 20, where the runs end on the iteration limit and not on the trust-region boundary after one iteration as they do
# from a random point -- and 3 x 10 from the random point with the trust region from which the oracle refuses one step
# of the three and accepts two (asserted below)
REJECT_RADIUS = 1e3
SOLVES = [("warm", dict(RTR_iterations=1, RTR_tCG_iterations=1)), ("warm", dict(RTR_iterations=1, RTR_tCG_iterations=2)),
          ("warm", dict(RTR_iterations=1, RTR_tCG_iterations=3)),
          ("cold", dict(RTR_iterations=3, RTR_tCG_iterations=10, RTR_initial_radius=REJECT_RADIUS))]
KEYS = (("outer_iterations", "outer_iters"), ("inner_iterations", "inner_iters"), ("accepted_steps", "accepted"),
        ("tCGStatus", "tcg_status"))


@pytest.mark.parametrize("variant", ["small", "long"])
@pytest.mark.parametrize("d,n,r", [(3, 8192, 3), (3, 8192, 5), (3, 8192, 8), (3, 8193, 3), (3, 8193, 5), (3, 8193, 8),
                                   (2, 8221, 3)])
def test_fused_solve_on_the_block_form(env, d, n, r, variant):
    da, orc = env
    ds, Q, pops = ig.graph(d, n, 0, variant)
    k = (d + 1) * n
    rng = np.random.default_rng(300 * d + r + n)
    G = rng.standard_normal((r, k))
    X = _point(orc, r, d, n, 30 + r)
    P = _problem(da, r, d, n, Q, G)
    Pg = _problem(da, r, d, n, Q, G, "generic")
    try:
        # the fused split form with the block evaluation (k_spmm_bsrq<.., GRAD>) and k_fused_hess_bsr: SE layout, r <= 8,
        # 8192 <= n <= 24576 (fused_supported), sparse preconditioner; under DCORA_SOLVER=generic no block form is built
        _on_block_form(P)
        assert (P.precond_info()["kind"], P.solver_info()["tcg"]) == ("sparse", "three launches"), P.solver_info()
        assert 8192 <= n <= 24576 and r <= 8
        assert Pg.qapply_info()["kernel"] == "k_spmm", Pg.qapply_info()
        rejected = 0
        for g in (G, None):
            P.set_linear_term(g)
            Pg.set_linear_term(g)
            Po = orc.Problem(r, d, n, Q, G=g, reg=0.1)
            Xw, _ = Po.optimize(X, RTR_iterations=10, RTR_tCG_iterations=20)
            for where, kw in SOLVES:
                X0 = Xw if where == "warm" else X
                out = []
                for prob in (P, Pg):
                    opt = da.QuadraticOptimizer(prob, da.ROptParameters(**kw))
                    Xs = opt.optimize(X0)
                    out.append((Xs, opt.getOptResult()))
                Xo, reso = Po.optimize(X0, **kw)
                tag = (d, n, r, variant, g is not None, kw)
                (Xf, resf), (Xg, resg) = out
                print("C %s: outer %d inner %d accepted %d status %d; per-pose |X - X_generic| %.2e |X - X_oracle| %.2e; "
                      "fInit %.1e gradNormInit %.1e fOpt %.1e" % (
                          tag, resf["outer_iterations"], resf["inner_iterations"], resf["accepted_steps"], resf["tCGStatus"],
                          _pose_dist(Xf, Xg, d), _pose_dist(Xf, Xo, d), abs(resf["fInit"] / reso["fInit"] - 1),
                          abs(resf["gradNormInit"] / reso["gradNormInit"] - 1), abs(resf["fOpt"] / reso["fOpt"] - 1)))
                for key, okey in KEYS:
                    assert resf[key] == resg[key] == reso[okey], (tag, key, resf[key], resg[key], reso[okey])
                assert resf["inner_iterations"] >= min(2, kw["RTR_tCG_iterations"]), tag   # (the gather of iteration 1 ran)
                for res in (resf, resg):
                    assert abs(res["fInit"] - reso["fInit"]) <= 1e-12 * abs(reso["fInit"]), tag
                    assert abs(res["gradNormInit"] - reso["gradNormInit"]) <= 1e-12 * reso["gradNormInit"], tag
                    assert abs(res["fOpt"] - reso["fOpt"]) <= 1e-9 * abs(reso["fOpt"]), tag
                assert _pose_dist(Xf, Xg, d) <= 1e-9, tag
                assert _pose_dist(Xf, Xo, d) <= 1e-7 and _pose_dist(Xg, Xo, d) <= 1e-7, tag
                if kw["RTR_iterations"] == 3:
                    rejected += 0 < reso["accepted"] < reso["outer_iters"]
        assert rejected == 2, "no step was refused and another accepted: the `cur` buffer switch did not run"
        _on_block_form(P)
    finally:
        P.close()
        Pg.close()


# ---- D -------------------------------------------------------------------------------------------------------------------
def _check_evaluation(out, ref, R, tag):
    c2, gn, bn, nxt = out
    print("D/E %s: cost2 %.1e gradnorm %.1e block norms %.1e next %d" % (
        tag, abs(c2 / ref["cost2"] - 1), abs(gn / ref["gradnorm"] - 1), np.abs(bn / ref["block_norms"] - 1).max(), nxt))
    assert abs(c2 - ref["cost2"]) <= 1e-11 * abs(ref["cost2"]), tag
    assert abs(gn - ref["gradnorm"]) <= 1e-10 * ref["gradnorm"], tag
    assert np.all(np.abs(bn - ref["block_norms"]) <= 1e-10 * ref["block_norms"]), tag
    top = np.sort(ref["block_norms"])[::-1]
    if R > 1:
        assert top[0] - top[1] > 1e-6 * top[0], (tag, top[:2])   # the argmax is decided
    assert nxt == int(np.argmax(ref["block_norms"])), tag


def _central_twin_on_block_form(da, r, d, n, Q):
    """the session's central problem is DeviceProblem::init of (r, d, n, Q) without a preconditioner: a problem handle
    created the same way reports the Q-apply the rules give it"""
    P = da.QuadraticProblem(r, d, n, Q, reg=-1)
    try:
        _on_block_form(P)
    finally:
        P.close()


@pytest.mark.parametrize("d,n,R,r", [(3, 8193, 1, 3), (3, 8193, 3, 4), (3, 8193, 5, 5), (3, 8193, 7, 6), (3, 8193, 64, 8),
                                     (2, 8221, 5, 4)])
def test_central_evaluation_with_the_agent_split(env, d, n, R, r):
    da, orc = env
    ds, Q, pops = ig.graph(d, n, 0, "long")
    _central_twin_on_block_form(da, r, d, n, Q)
    sizes = {hi - lo for lo, hi in ig.eval_ranges(n, R)}
    assert sizes <= {31, 32, 33}
    if R == 5:
        assert 33 in sizes   # more than 32 poses in a workgroup's range: two passes of 17
    X = _point(orc, r, d, n, 40 + R)
    ps = ig.agent_ranges(n, R)
    ref = ig.reference(Q, X, None, d, pose_start=ps)
    s = da.RbcdSession(ds, num_robots=R, r=r)
    try:
        assert [s.agent_info(a)["first_pose"] for a in range(R)] == ps[:-1].tolist()
        s.set_X(X)
        _check_evaluation(s.evaluate(), ref, R, (d, n, R, r))
    finally:
        s.close()


def test_two_agents_on_the_block_form(env):
    """RBCD++ with two agents of 8200 poses: their local problems take the block form (n_a >= 8192, r <= 8) with the
    linear term of the coupling, against the oracle's driver as test_planar_lattice_on_the_block_structure does"""
    da, orc = env
    import bench
    d, n, R, r, iters = 3, 16400, 2, 5, 3
    ds, Q, pops = ig.graph(d, n, 0, "long")
    dso = orc.Dataset(d, n, ds.ids, ds.vals)
    # from the oracle's iterate after 5 iterations, all of agent 0: the next three are of agent 0, 1 and 1
    X0 = orc.run_rbcd(dso, _point(orc, r, d, n, 50), num_robots=R, r_min=r, max_iters=5, staircase=0, rgrad_tol=0.0)["X"]
    for b in range(R):   # an agent's own problem, created as the session creates it
        nb, ids, vals = bench.agent_block(ds, R, b)
        assert nb >= 8192
        Pa = da.QuadraticProblem(r, d, nb, da.build_Q_pgo(ds, n=nb, agent=b, ids=ids, vals=vals))
        try:
            _on_block_form(Pa)
            assert Pa.solver_info()["tcg"] == "three launches" and Pa.precond_info()["kind"] == "sparse"
        finally:
            Pa.close()
    tr = orc.run_rbcd(dso, X0, num_robots=R, r_min=r, max_iters=iters, staircase=0, rgrad_tol=0.0)
    s = da.RbcdSession(ds, num_robots=R, r=r)
    try:
        assert [s.agent_info(a)["num_poses"] for a in range(R)] == [8200, 8200]
        s.set_X(X0)
        out = s.run(max_iters=iters, rgrad_tol=0.0)
        X = s.get_X()
    finally:
        s.close()
    print("two agents: cost %s gradnorm %s |X - X_oracle| %.2e" % (
        np.abs(out["cost"] / tr["cost"] - 1), np.abs(out["gradnorm"] / tr["gradnorm"] - 1), common.rel(X, tr["X"])))
    assert set(tr["selected"].tolist()) == {0, 1}   # both agents solved
    assert out["iters"] == iters and np.array_equal(out["selected"], tr["selected"])
    assert np.allclose(out["cost"], tr["cost"], rtol=1e-10, atol=0)
    assert np.allclose(out["gradnorm"], tr["gradnorm"], rtol=1e-8, atol=0)
    assert common.rel(X, tr["X"]) < 1e-7


# ---- E -------------------------------------------------------------------------------------------------------------------
def _weights(m, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, m)
    pick = rng.permutation(m)
    w[pick[:m // 10]] = 0.0
    w[pick[m // 10:m // 5]] = 1e-8
    return w


@pytest.mark.parametrize("R", [5, 1])
def test_reweighting_restages_the_block_values(env, R):
    da, orc = env
    from dcora_amd import robust as rb
    d, n, r = 3, 8192, 5
    ds, Q, pops = ig.graph(d, n, 0, "small")
    _central_twin_on_block_form(da, r, d, n, Q)
    X = _point(orc, r, d, n, 60)
    ps = ig.agent_ranges(n, R)
    w = _weights(ds.m, 61)
    dw = da.Dataset(d, n, ds.ids.copy(), ds.vals.copy())
    dw.vals[:, -1] = w
    Qw = da.build_Q_pgo(dw)
    s = da.RbcdSession(ds, num_robots=R, r=r, robust=rb.RobustCostParameters("GNC_TLS"))
    try:
        w0 = s.get_weights()   # 1 on every loop closure (initializeRobustOptimization), the data set's on the odometry
        d0 = da.Dataset(d, n, ds.ids.copy(), ds.vals.copy())
        d0.vals[:, -1] = w0
        s.set_X(X)
        first = s.evaluate()
        _check_evaluation(first, ig.reference(da.build_Q_pgo(d0), X, None, d, pose_start=ps), R, ("created", R))
        s.set_weights(w)
        assert np.array_equal(s.get_weights(), w)
        ref_w = ig.reference(Qw, X, None, d, pose_start=ps)
        assert abs(ref_w["cost2"] - first[0]) > 1e-3 * abs(first[0])   # the new weights show
        _check_evaluation(s.evaluate(), ref_w, R, ("reweighted", R))
        s.set_weights(w0)
        again = s.evaluate()
        assert again[0] == first[0] and again[1] == first[1] and np.array_equal(again[2], first[2]) and again[3] == first[3]
        if R == 1:   # the agent's own block form: one iteration on the new weights against a session created with them
            s.set_weights(w)
            s.set_X(X)
            s.evaluate()
            got = s.iterate(0)
            Xa = s.get_X()
            t = da.RbcdSession(dw, num_robots=1, r=r)
            try:
                assert t.agent_info(0)["num_poses"] == n >= 8192
                t.set_X(X)
                t.evaluate()
                exp = t.iterate(0)
                Xt = t.get_X()
            finally:
                t.close()
            print("E agent: cost2 %.1e gradnorm %.1e per-pose |X - X_fresh| %.2e" % (
                abs(got[0] / exp[0] - 1), abs(got[1] / exp[1] - 1), _pose_dist(Xa, Xt, d)))
            assert got[0] < ref_w["cost2"]   # the iteration moved
            assert abs(got[0] - exp[0]) <= 1e-9 * abs(exp[0]) and abs(got[1] - exp[1]) <= 1e-8 * exp[1]
            assert _pose_dist(Xa, Xt, d) <= 1e-9
            _check_evaluation(got, ig.reference(Qw, Xa, None, d, pose_start=ps), R, ("after iterate", R))
    finally:
        s.close()
