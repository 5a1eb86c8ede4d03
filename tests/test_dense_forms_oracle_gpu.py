"""The dense-preconditioner forms of the local solve against the CPU oracle at the sizes where they run.

An agent of the headline (sphere2500 / 5, n = 500, k = 2000) solves with the dense inverse of Q + reg I applied inside
k_fused_pc (form 1, "two launches") or inside the one-launch tCG run k_tcg_run (form 2, "one launch per run"); beyond
fused_pc_preferred() the step, product and projection stay separate launches (form 0, "three launches"), and beyond
kDensePrecondMaxK the preconditioner is the partitioned sparse inverse.  Every shape below states the form the rules of
device_problem.hip / fused_step.hip give it, checks that the device chose it, and only then compares the HIP path with
the oracle: the operations at a random point, then whole RTR solves (iteration counts, exit reasons, optimum, iterate).
Form 2 is checked a second time on the launches (DCORA_SOLVER_TCG=launch): both forms against the oracle, not only
against each other.  Then the trust-region corners on the run form, RBCD++ traces of the headline split, and the
thread-per-variable (generic) solver on a block whose hub pose has long rotation rows: the two-launch Hessian product
k_spmm_dir + k_hessfix, which no dataset of the suite reaches."""
import os

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

NAME = "sphere2500"
TCG = {0: "three launches", 1: "two launches", 2: "one launch per run"}

# (id, block, r, preconditioner, tCG form).  block: ("prefix", n) = the first n poses with their private measurements,
# ("agent", b) = agent b of the contiguous 5-way split (bench.agent_block), ("hub", n, pose, nnz) = a prefix block with
# measurements added from `pose` until the worst two-pose row pair of Q holds exactly `nnz` CSR entries, ("long", n,
# pose, m) = a prefix block with measurements added from `pose` to m poses that were not its neighbours.
# Form 2 (tcg_run_supported): d = 3, 4 <= r <= 6, fused_pc_preferred, grid (n + 1) / 2 <= 256, k <= 4 * 4 * 128 = 2048,
# worst row pair <= kRunQCap = 1024.  Form 1 (fused_pc_preferred): k within one LDS chunk of the residual
# (3200 / 2688 / 2304 columns at r = 5 / 6 / 7), r k <= 2 * 25 * 256 = 12800, r <= 7.  Dense while k <= 2200.
SHAPES = [
    ("n2_r5", ("prefix", 2), 5, "dense", 2),          # a grid of one workgroup
    ("b0_r4", ("agent", 0), 4, "dense", 2),           # the headline blocks, k = 2000
    ("b0_r5", ("agent", 0), 5, "dense", 2),
    ("b0_r6", ("agent", 0), 6, "dense", 2),
    ("b4_r4", ("agent", 4), 4, "dense", 2),
    ("b4_r5", ("agent", 4), 5, "dense", 2),
    ("b4_r6", ("agent", 4), 6, "dense", 2),
    ("n511_r5", ("prefix", 511), 5, "dense", 2),      # grid 256, the last workgroup holds one pose
    ("n512_r4", ("prefix", 512), 4, "dense", 2),      # k = 2048: grid and register caps both exactly met
    ("n512_r5", ("prefix", 512), 5, "dense", 2),
    ("n512_r6", ("prefix", 512), 6, "dense", 2),
    ("n513_r5", ("prefix", 513), 5, "dense", 1),      # one past both caps; k = 2052: a partial last 128-column step
    ("n533_r6", ("prefix", 533), 6, "dense", 1),      # r k = 12792
    ("n534_r6", ("prefix", 534), 6, "dense", 0),      # r k = 12816
    ("n457_r7", ("prefix", 457), 7, "dense", 1),      # r k = 12796; r = 7 is never the run form
    ("n458_r7", ("prefix", 458), 7, "dense", 0),      # r k = 12824
    ("n550_r5", ("prefix", 550), 5, "dense", 1),      # k = 2200 = kDensePrecondMaxK
    ("n551_r5", ("prefix", 551), 5, "sparse", 0),     # k = 2204
    ("hub150_1024", ("hub", 300, 150, 1024), 5, "dense", 2),   # kRunQCap exactly met by an interior pair
    ("hub150_1040", ("hub", 300, 150, 1040), 5, "dense", 1),
    ("hub300_1024", ("hub", 301, 300, 1024), 5, "dense", 2),   # ... by the lone last pose of an odd n
    ("hub300_1040", ("hub", 301, 300, 1040), 5, "dense", 1),
]


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


def worst_pair_nnz(Q, n, d=3):
    """CSR entries of the worst pair of poses (2 i, 2 i + 1) of Q: what tcg_run_max_rows_nnz compares with kRunQCap"""
    dh = d + 1
    return max(int(Q.rp[min(n, p + 2) * dh] - Q.rp[p * dh]) for p in range(0, n, 2))


def _edges_from(rng, hub, cand, count, zeros, kappa, tau):
    """`count` measurements from `hub` to the poses popped off `cand`: random rotations, translations in +-[0.5, 1.5]
    with the first `zeros` components exactly zero, the given precisions, weights in [0.5, 1.5]"""
    from dcora_amd import synth
    R = synth._rand_rot(rng, count)
    t = rng.uniform(0.5, 1.5, (count, 3)) * rng.choice([-1.0, 1.0], (count, 3))
    t[:, :zeros] = 0.0
    j = [cand.pop() for _ in range(count)]
    ids = np.array([[0, hub, 0, q] for q in j], np.int32).reshape(-1, 4)
    vals = np.column_stack([R.transpose(0, 2, 1).reshape(count, 9), t, np.full(count, kappa), np.full(count, tau),
                            rng.uniform(0.5, 1.5, count)])
    return ids, vals


def _long_edges(ids, vals, n, hub, m):
    """measurements from `hub` to m distinct poses of the block that are not yet its neighbours"""
    near = set(ids[ids[:, 1] == hub, 3]) | set(ids[ids[:, 3] == hub, 1]) | {hub}
    rng = np.random.default_rng(hub + m)
    cand = [int(j) for j in rng.permutation(n) if int(j) not in near]
    return _edges_from(rng, hub, cand, m, 0, np.median(vals[:, 12]), np.median(vals[:, 13]))


def _hub_edges(ds, ids, vals, n, hub, target):
    """measurements from `hub` to distinct new neighbours of the block until the row pair holding it has exactly
    `target` CSR entries.  A new neighbour adds 13 entries to the hub's rows (its 4 x 4 block of Q less the structural
    zeros of the translation row), a translation component that is exactly zero one fewer (Q keeps no explicit zeros),
    and the first measurement leaving a pose fills the rotation-translation coupling of its diagonal block: so the
    count is measured on the built Q after every step rather than predicted."""
    import dcora_amd as da
    p0 = hub - hub % 2
    near = set(ids[ids[:, 1] == hub, 3]) | set(ids[ids[:, 3] == hub, 1]) | set(range(p0, min(n, p0 + 2)))
    rng = np.random.default_rng(hub + target)
    cand = [int(j) for j in rng.permutation(n) if int(j) not in near]
    kappa, tau = np.median(vals[:, 12]), np.median(vals[:, 13])
    new_ids, new_vals = np.zeros((0, 4), np.int32), np.zeros((0, vals.shape[1]))

    def held():
        rp = da.build_Q_pgo(ds, n=n, ids=np.r_[ids, new_ids], vals=np.r_[vals, new_vals]).rp
        return int(rp[min(n, p0 + 2) * 4] - rp[p0 * 4])

    def add(count, zeros):
        nonlocal new_ids, new_vals
        hi, hv = _edges_from(rng, hub, cand, count, zeros, kappa, tau)
        new_ids, new_vals = np.r_[new_ids, hi], np.r_[new_vals, hv]

    add(1, 0)
    rem = target - held()
    m = -(-rem // 13)   # m new neighbours of 13 - zeros entries each
    cut = [(13 * m - rem) // m + (i < (13 * m - rem) % m) for i in range(m)]
    assert max(cut) <= 3
    for c in sorted(set(cut)):
        add(cut.count(c), c)
    assert held() == target
    return new_ids, new_vals


_CASES = {}


def case(block, r):
    """one block, built once per module: n, the device's Q, the oracle's problem (Q + reg I, G), G, a random start X, a
    tangent V at X, and a warm start (the oracle's iterate after 15 RTR iterations from X, where tCG runs go deep)"""
    key = (block, r)
    if key in _CASES:
        return _CASES[key]
    import bench
    import dcora_amd as da
    from oracle import orc
    ds, dso = common.product_dataset(NAME), common.oracle_dataset(NAME)
    if block[0] == "agent":
        b = block[1]
        n, ids, vals = bench.agent_block(ds, 5, b)
        _, idso, valso = bench.agent_block(dso, 5, b)
        Q = da.build_Q_pgo(ds, n=n, agent=b, ids=ids, vals=vals)
        Qo = orc.build_Q_pgo(dso, n=n, agent=b, ids=idso, vals=valso)
    else:
        n = block[1]
        keep = (ds.ids[:, 1] < n) & (ds.ids[:, 3] < n)
        ids, vals, idso, valso = ds.ids[keep], ds.vals[keep], dso.ids[keep], dso.vals[keep]
        if block[0] in ("hub", "long"):
            hi, hv = (_hub_edges(ds, ids, vals, n, block[2], block[3]) if block[0] == "hub" else
                      _long_edges(ids, vals, n, block[2], block[3]))
            ids, vals = np.r_[ids, hi], np.r_[vals, hv]
            idso, valso = np.r_[idso, hi], np.r_[valso, hv]
        Q = da.build_Q_pgo(ds, n=n, ids=ids, vals=vals)
        Qo = orc.build_Q_pgo(dso, n=n, ids=idso, vals=valso)
        if block[0] == "hub":
            assert worst_pair_nnz(Q, n) == block[3]   # (the oracle's Q also stores the zeros of those translations)
            assert max(np.diff(Q.rp)) <= 512   # (no long row: the hub stays on the row-parallel Q-apply)
    k = 4 * n
    rng = np.random.default_rng(2)
    G = 0.1 * rng.standard_normal((r, k))
    X = common.random_point(r, 3, n, 9, orc.project_to_manifold)
    V = orc.tangent_project(r, 3, n, X, common.random_tangent(r, 3, n, 6))
    Po = orc.Problem(r, 3, n, Qo, G=G, reg=0.1)
    Xw, _ = Po.optimize(X, RTR_iterations=15, RTR_tCG_iterations=50)
    _CASES[key] = (n, Q, Po, G, X, V, Xw)
    return _CASES[key]


def make_problem(da, r, n, Q, G, form, solver=None):
    """the device problem; form "launch" keeps the run form off and solver "generic" the fused pose-graph kernels (both
    choices are read when the problem is created)"""
    if form:
        os.environ["DCORA_SOLVER_TCG"] = form
    if solver:
        os.environ["DCORA_SOLVER"] = solver
    try:
        return da.QuadraticProblem(r, 3, n, Q, G=G, reg=0.1)
    finally:
        os.environ.pop("DCORA_SOLVER_TCG", None)
        os.environ.pop("DCORA_SOLVER", None)


PARAMS = [dict(), dict(RTR_iterations=4, RTR_tCG_iterations=3),
          dict(RTR_iterations=8, RTR_tCG_iterations=60, gradnorm_tol=1e-9)]


def compare_solve(da, P, Po, X0, kw, exact, tag):
    """one optimize on both sides: counts and exit reason equal (exact), or the optimum and its gradient (long runs)"""
    opt = da.QuadraticOptimizer(P, da.ROptParameters(**kw))
    X = opt.optimize(X0)
    res = opt.getOptResult()
    Xo, reso = Po.optimize(X0, **kw)
    assert abs(res["fOpt"] - reso["fOpt"]) <= 1e-8 * abs(reso["fOpt"]), (tag, kw, res, reso)
    if exact:
        for key, okey in (("outer_iterations", "outer_iters"), ("inner_iterations", "inner_iters"),
                          ("accepted_steps", "accepted"), ("tCGStatus", "tcg_status")):
            assert res[key] == reso[okey], (tag, kw, key, res[key], reso[okey])
        assert abs(res["fInit"] - reso["fInit"]) <= 1e-11 * abs(reso["fInit"]), (tag, kw)
        assert common.rel(X, Xo) < 1e-6, (tag, kw, common.rel(X, Xo))
    else:
        assert abs(Po.f(X) - res["fOpt"]) <= 1e-10 * abs(res["fOpt"]), (tag, kw)
        gn = np.linalg.norm(Po.rgrad(X))
        assert abs(gn - res["gradNormOpt"]) <= 1e-6 * max(1.0, gn), (tag, kw, gn, res["gradNormOpt"])
    return reso


@pytest.mark.parametrize("sid,block,r,precond,form", SHAPES, ids=[s[0] for s in SHAPES])
def test_dense_form_matches_oracle(env, sid, block, r, precond, form):
    """the form the rules give this shape, then f, RieGrad, HessVec, PreCondition and three RTR solves from a random
    and a warm start against the oracle -- in both tCG forms where the run form applies"""
    da, _ = env
    n, Q, Po, G, X, V, Xw = case(block, r)
    for variant in ((None, "launch") if form == 2 else (None,)):
        P = make_problem(da, r, n, Q, G, variant)
        try:
            want = TCG[1] if variant else TCG[form]
            assert P.precond_info()["kind"] == precond, (sid, P.precond_info())
            assert P.solver_info()["tcg"] == want, (sid, variant, P.solver_info())
            fo = Po.f(X)
            assert abs(P.f(X) - fo) <= 1e-12 * abs(fo), sid
            assert common.rel(P.RieGrad(X), Po.rgrad(X)) < 1e-12, sid
            assert common.rel(P.HessVec(X, V), Po.hess(X, V)) < 1e-12, sid
            assert common.rel(P.PreCondition(X, V), Po.precondition(X, V)) < 1e-9, sid
            for i, kw in enumerate(PARAMS):
                compare_solve(da, P, Po, X, kw, i < 2, (sid, variant, "cold"))
            # from the warm start the tCG runs go 20-30 iterations deep: sets 1 and 2 only.  Set 3 there (8 x 60) is
            # ill-conditioned in itself -- the oracle against the oracle from a start moved by 1e-14 relative ends
            # 5e-6 .. 9e-3 apart in f at b0_r5, n511_r5, n513_r5 and n533_r6, with the same iteration counts
            for kw in PARAMS[:2]:
                compare_solve(da, P, Po, Xw, kw, True, (sid, variant, "warm"))
            assert P.solver_info()["tcg"] == want, (sid, variant)   # (the run form did not give up)
        finally:
            P.close()


# (id, new neighbours of pose 150 in the 300-pose prefix, r, DCORA_SOLVER).  The rotation rows 600 .. 602 of the hub
# hold 578 (m = 140) and 1098 (m = 270) entries, more than kLongRow = 512, and are no Euclidean columns: the generic
# solver's Hessian product is k_spmm_dir + k_hessfix (hess_one_launch() is false), every Q-apply takes k_spmm's slices.
# A slice (row / kLongSplit = 8) is 73 entries against a stride of 8 * (256 / 5) = 408 at r = 5, one masked trip, and
# 138 against 8 * 16 = 128 at r = 16, two trips; the hub's row block holds 2735 and 3795 entries, two and three tiles
# of kSpmmTile = 1536.
LONG_ROWS = [
    ("long150_r5", 140, 5, "generic"),   # r <= 8: the fused pose-graph kernels are switched off
    ("long150_r16", 270, 16, None),      # r > 8 is generic by itself
]


@pytest.mark.parametrize("sid,m,r,solver", LONG_ROWS, ids=[s[0] for s in LONG_ROWS])
def test_generic_solver_long_rotation_rows_match_oracle(env, sid, m, r, solver):
    """long rows that are not Euclidean columns: the two-launch Hessian product of the generic tCG is the one in use;
    f, RieGrad, HessVec, PreCondition and RTR solves from a random and a warm start against the oracle (from the warm
    start the tCG runs go 4 to 8 iterations deep, and with 3 tCG iterations every run ends on the iteration limit),
    and the same solve twice bit for bit: the order in which the slices of a row arrive must not show"""
    da, _ = env
    from dcora_amd import capi
    n, Q, Po, G, X, V, Xw = case(("long", 300, 150, m), r)
    nnz = np.diff(Q.rp)
    assert max(nnz) > 512 and any(j % 4 != 3 for j in np.flatnonzero(nnz > 512)), sid
    P = make_problem(da, r, n, Q, G, None, solver)
    try:
        # (solver_info() looks at the preconditioner form alone and says "two launches" under DCORA_SOLVER=generic)
        assert P.qapply_info()["kernel"] == "k_spmm", (sid, P.qapply_info())
        assert solver or P.solver_info()["tcg"] == TCG[0], (sid, P.solver_info())
        with pytest.raises(capi.DcoraError):   # the one-launch product does not apply: k_spmm_dir + k_hessfix it is
            P.HessVecSolverForm(X, V)
        fo = Po.f(X)
        assert abs(P.f(X) - fo) <= 1e-12 * abs(fo), sid
        assert common.rel(P.RieGrad(X), Po.rgrad(X)) < 1e-12, sid
        assert common.rel(P.HessVec(X, V), Po.hess(X, V)) < 1e-12, sid
        assert common.rel(P.PreCondition(X, V), Po.precondition(X, V)) < 1e-9, sid
        for i, kw in enumerate(PARAMS):
            compare_solve(da, P, Po, X, kw, i < 2, (sid, "cold"))
        for kw in PARAMS[:2]:
            compare_solve(da, P, Po, Xw, kw, True, (sid, "warm"))
        runs = []
        for _ in range(2):
            opt = da.QuadraticOptimizer(P, da.ROptParameters(**PARAMS[0]))
            Xr = opt.optimize(Xw)
            res = opt.getOptResult()
            res.pop("elapsedMs")
            runs.append((Xr, res))
        assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1], (sid, runs[0][1], runs[1][1])
    finally:
        P.close()


def test_trust_region_corners_on_the_run_form(env):
    """a headline agent block in form 2 from a tiny and a huge initial radius, two seeds each, against the oracle: the
    cases together reach a rejected step, a tCG run ended on the trust-region boundary and one on negative curvature
    (oracle_problem.cpp tcg(): status 0 = negative curvature, 1 = boundary)"""
    da, orc = env
    n, Q, Po0, G, _, _, _ = case(("agent", 0), 5)
    seen = {"rejected": 0, "boundary": 0, "negative": 0}
    for seed in (1, 2):
        X = common.random_point(5, 3, n, seed, orc.project_to_manifold)
        P = make_problem(da, 5, n, Q, G, None)
        try:
            assert P.solver_info()["tcg"] == TCG[2]
            for radius in (1e-2, 1e4):
                for i in (0, 2):
                    kw = dict(PARAMS[i], RTR_initial_radius=radius)
                    reso = compare_solve(da, P, Po0, X, kw, i == 0, (seed, radius))
                    seen["rejected"] += reso["accepted"] < reso["outer_iters"]
                    seen["boundary"] += reso["tcg_status"] == 1
                    seen["negative"] += reso["tcg_status"] == 0
            assert P.solver_info()["tcg"] == TCG[2]
        finally:
            P.close()
    assert all(seen.values()), seen


def _trace(env, R, r, iters):
    da, orc = env
    import bench
    ds, dso = common.product_dataset(NAME), common.oracle_dataset(NAME)
    X0 = bench.initial_point(da, ds, r)
    tr = orc.run_rbcd(dso, X0, num_robots=R, r_min=r, max_iters=iters, staircase=0, rgrad_tol=1e-12)
    s = da.RbcdSession(ds, num_robots=R, r=r)
    try:
        s.set_X(X0)
        s.profile_tcg_runs(True)
        s.profile_tcg_read()
        out = s.run(max_iters=iters, rgrad_tol=1e-12)
        prof = s.profile_tcg_read()
        s.profile_tcg_runs(False)
        X = s.get_X()
    finally:
        s.close()
    assert out["iters"] == iters
    assert prof["launches"] >= iters, prof   # the agents ran k_tcg_run and it did not give up
    assert np.array_equal(out["selected"], tr["selected"])
    assert np.allclose(out["cost"], tr["cost"], rtol=1e-8)
    assert np.allclose(out["gradnorm"], tr["gradnorm"], rtol=1e-5)
    assert common.rel(X, tr["X"]) < 1e-6


def test_rbcd_sphere2500_five_agents_matches_oracle(env):
    """the headline: RBCD++ on sphere2500 split over 5 agents (n = 500 each) at r = 5, acceleration and greedy
    selection, 40 iterations across the restart at 30, against the oracle's driver"""
    _trace(env, 5, 5, 40)


@pytest.mark.parametrize("R,r", [(5, 4), (5, 6), (8, 5)])
def test_rbcd_sphere2500_run_form_ranks_match_oracle(env, R, r):
    """the other run-form shapes of the staircase, 24 iterations: r = 4 and r = 6 at R = 5 (k_tcg_run<3,6,4> spills
    to scratch), and R = 8 at r = 5 (312 poses per agent, the last one 316)"""
    _trace(env, R, r, 24)
