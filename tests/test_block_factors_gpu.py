"""polar_blk, qf_blk (manifold.hip) and so_project (round.hip) against tests/golden/block_factors.npz, the 50-digit
factors of single blocks, through the entry points that exist: manifold_project (k_polar), QuadraticProblem.Retract
(k_retract), align_lifted_trajectory_to_frame (k_align_poses) and project_solution_raslam (k_project_rotations and the
reflect decision); and the second grid pass of k_polar.

Every comparison is per block -- the maximum over the blocks of a group, never a ratio over a whole matrix.  A group
passes when the device's error is at most 8 x max(oracle_err_g, eps cond_g): oracle_err_g is what the CPU oracle, the
same algorithm in IEEE double, achieves on the same blocks (stored in the fixture); 8 covers FMA contraction, the
device's 40 sweeps against the oracle's 60 and the under-estimate of a group's maximum by 4 samples.  The orthogonality
error is at most 8 x oracle_orth whatever the conditioning.  A flaw of the method sits orders of magnitude above.

Largest device error / max(oracle_err_g, eps cond_g) observed on an MI355X, per entry point (bound: 8):
  k_polar    SE 1.58 (d=2 r=2 kappa=1)   RA 1.21 (d=2 r=5 kappa=1)
  k_retract  SE 1.58 (d=2 r=2 kappa=1)   RA 1.39 (d=3 r=6 kappa=1)
  so_project r=d 1.41 (d=2, det<0, sigma_min=1e-9)   r=5 under R0 1.58 (d=2, det>0, close pair)
  exact rank d-1 blocks: error 0;  orthogonality: 1.03 x oracle_orth at most (bound: 8)
  reflect decision: |G - G_expected|_max <= 8.0e-15 (bound 1e-10), the other branch >= 3.6 away
  second grid pass of k_polar: 8.3e-16 (first pass 1.4e-15; bound 1e-12)
With so_project as it was before the zero column was completed, the two r = d cases of the SO(d) test fail (det = 0 on
the rank d-1 blocks) and nothing else does.
"""
import numpy as np
import pytest

import block_factors as bf

pytestmark = pytest.mark.gpu

EPS = bf.EPS


def _check_groups(entry, rows, orth, fx):
    """rows: (group name, device error, max(oracle error, eps cond)); prints every ratio, asserts each <= 8"""
    lines = ["%-14s %-34s device %.3e  oracle-or-eps-cond %.3e  ratio %.2f" % (entry, n, e, t, e / t) for n, e, t in rows]
    worst = max(rows, key=lambda x: x[1] / x[2])
    print("\n".join(lines))
    print("RATIO %s max %.2f (%s); orthogonality %.2f x oracle_orth" % (entry, worst[1] / worst[2], worst[0],
                                                                         orth / float(fx["oracle_orth"])))
    bad = [ln for ln, (n, e, t) in zip(lines, rows) if not e <= 8 * t]
    assert not bad, "device error above 8 x max(oracle_err_g, eps cond_g):\n" + "\n".join(bad)
    assert orth <= 8 * float(fx["oracle_orth"]), (entry, orth)


def _pq_rows(groups, out, what):
    return [(g.name, err, g.tol(what)) for g, err in bf.pq_group_errors(groups, out, what)]


def _identity(k):
    import scipy.sparse as sp
    import dcora_amd as da
    return da.Csr.from_scipy(sp.identity(k, format="csr"))


# ---- a. k_polar, b. k_retract: SE layout ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d,r", bf.PQ_DR)
def test_polar_blocks_match_the_high_precision_factor(built, d, r):
    import dcora_amd as da
    fx = bf.load()
    groups = bf.pq_groups(fx, d, r)
    A = np.concatenate([g.inp for g in groups])
    nb = len(A)
    T = 10 * np.random.default_rng(r * 10 + d).standard_normal((r, nb))
    out = da.manifold_project(r, d, nb, bf.se_matrix(A, T))
    assert np.array_equal(out[:, d::d + 1], T)  # translations: bitwise
    Y = bf.se_blocks(out, d)
    _check_groups("k_polar", _pq_rows(groups, Y, "polar"), bf.orth_err(Y).max(), fx)


@pytest.mark.parametrize("d,r", bf.PQ_DR)
def test_qf_retraction_blocks_match_the_high_precision_factor(built, d, r):
    """DeviceProblem::retract passes alpha = 1, so the kernel forms X + V; V = A - X makes that sum the fixture's block"""
    import dcora_amd as da
    fx = bf.load()
    groups = bf.pq_groups(fx, d, r)
    A = np.concatenate([g.inp for g in groups])
    nb = len(A)
    rng = np.random.default_rng(r * 10 + d)
    X = bf.se_matrix(bf.qf_point(nb, r, d), 10 * rng.standard_normal((r, nb)))
    V = bf.se_matrix(A - bf.qf_point(nb, r, d), rng.standard_normal((r, nb)))
    W = X + V
    assert np.array_equal(bf.se_blocks(W, d), A)
    P = da.QuadraticProblem(r, d, nb, _identity((d + 1) * nb))
    try:
        out = P.Retract(X, V)
    finally:
        P.close()
    assert np.array_equal(out[:, d::d + 1], W[:, d::d + 1])  # translations: X + V bitwise
    Y = bf.se_blocks(out, d)
    _check_groups("k_retract", _pq_rows(groups, Y, "qf"), bf.orth_err(Y).max(), fx)


# ---- c. the RA layout through both entry points --------------------------------------------------------------------------
def _ra_blocks(M, d, n):
    return np.ascontiguousarray(M[:, :d * n].reshape(M.shape[0], n, d).transpose(1, 0, 2))


def _unit_columns_longdouble(W):
    W = W.astype(np.longdouble)
    return W / np.sqrt((W * W).sum(axis=0, keepdims=True))


@pytest.mark.parametrize("d", [2, 3])
def test_ra_layout_polar_and_qf(built, d):
    import dcora_amd as da
    fx = bf.load()
    r, l, b = d + 3, 5, 3
    groups = bf.pq_groups(fx, d, r)
    A = np.concatenate([g.inp for g in groups])
    n = len(A)
    k = (d + 1) * n + l + b
    sph, euc = slice(d * n, d * n + l), slice(d * n + l, k)
    rng = np.random.default_rng(40 + d)
    # polar: [Y_1 .. Y_n | spheres | translations | landmarks]
    M = rng.standard_normal((r, k)) * np.exp(rng.uniform(-3, 3, k))
    M[:, :d * n] = A.transpose(1, 0, 2).reshape(r, d * n)
    out = da.manifold_project(r, d, n, M, l=l, b=b)
    assert np.array_equal(out[:, euc], M[:, euc])
    assert np.abs(out[:, sph] - _unit_columns_longdouble(M[:, sph])).max() <= 8 * EPS
    Y = _ra_blocks(out, d, n)
    _check_groups("k_polar RA", _pq_rows(groups, Y, "polar"), bf.orth_err(Y).max(), fx)
    # retraction from an on-manifold point: eye(r, d) blocks, unit vectors on the spheres
    X = rng.standard_normal((r, k))
    X[:, :d * n] = bf.qf_point(n, r, d).transpose(1, 0, 2).reshape(r, d * n)
    X[:, sph] = np.eye(r)[:, [j % r for j in range(1, l + 1)]]
    V = rng.standard_normal((r, k))
    V[:, :d * n] = M[:, :d * n] - X[:, :d * n]
    W = X + V
    assert np.array_equal(_ra_blocks(W, d, n), A)
    P = da.QuadraticProblem(r, d, n, _identity(k), l=l, b=b)
    try:
        out = P.Retract(X, V)
    finally:
        P.close()
    assert np.array_equal(out[:, euc], W[:, euc])
    assert np.abs(out[:, sph] - _unit_columns_longdouble(W[:, sph])).max() <= 8 * EPS
    Y = _ra_blocks(out, d, n)
    _check_groups("k_retract RA", _pq_rows(groups, Y, "qf"), bf.orth_err(Y).max(), fx)


# ---- d. so_project through k_align_poses ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d,r", bf.SO_DR)
def test_so_projection_blocks_match_the_high_precision_factor(built, d, r):
    """anchor [I | 0] at r = d: the kernel projects every block as given; [R0 | 0] for the fixture's r = 5 sets.  Both
    determinant signs, sigma_min down to 1e-9, a close pair, and (r = d) the exact rank d - 1 blocks, whose nearest
    rotation is unique: the zero column has to be completed, not left as it is"""
    import dcora_amd as da
    fx = bf.load()
    groups = bf.so_groups(fx, d, r)
    assert {g.sign for g in groups} == ({1, -1, 0} if r == d else {1, -1})
    Yin = np.concatenate([g.inp for g in groups])
    nb = len(Yin)
    T = 10 * np.random.default_rng(60 + r * 10 + d).standard_normal((r, nb))
    anchor = bf.so_anchor(fx, d, r)
    out = da.align_lifted_trajectory_to_frame(bf.se_matrix(Yin, T), anchor, d, nb, True)
    assert out.shape == (d, (d + 1) * nb)
    if r == d:
        assert np.array_equal(out[:, d::d + 1], T)  # R0 = I, t0 = 0: bitwise
    else:
        want = anchor[:, :d].astype(np.longdouble).T @ T.astype(np.longdouble)
        assert (np.abs(out[:, d::d + 1] - want).max(axis=0) <= 8 * EPS * np.linalg.norm(T, axis=0)).all()
    R = bf.se_blocks(out, d)
    assert (np.linalg.det(R) > 1 - 64 * EPS).all(), np.linalg.det(R).min()
    rows = [(g.name, err, g.tol()) for g, err in bf.so_group_errors(groups, R)]
    _check_groups("so_project", rows, bf.orth_err(R).max(), fx)


# ---- e. the reflect decision of project_solution_raslam --------------------------------------------------------------------
def _so_numpy(B):
    U, _, Vt = np.linalg.svd(B)
    D = np.eye(B.shape[0])
    D[-1, -1] = np.sign(np.linalg.det(U @ Vt))
    return U @ D @ Vt


def _project_ra_numpy(Xd, d, n, l, reflect):
    P = Xd.copy()
    if reflect:
        P[d - 1] = -P[d - 1]
    for i in range(n):
        P[:, d * i:d * i + d] = _so_numpy(P[:, d * i:d * i + d])
    P[:, d * n:d * n + l] /= np.linalg.norm(P[:, d * n:d * n + l], axis=0, keepdims=True)
    return P


@pytest.mark.parametrize("d", [2, 3])
def test_reflect_decision_of_project_solution_raslam(built, d):
    """m of the n = 9 rotation blocks of a rank-d solution are improper, R diag(1, .8[, -.5]), the rest proper,
    R diag(1, .8[, .5]).  None is orthogonal: whichever branch is taken, the minority ends up with det < 0, and only
    distinct singular values make its projection unique (a reflected rotation has none).  The rank-d truncation returns
    the solution in either handedness, so the count of positive blocks is n - m or m, and the rule npos < n / 2
    (integer division, ref src/DCORA_utils.cpp:2016) reflects in both cases only for m >= n - n/2 + 1 and in neither
    only for m <= n/2 - 1.  For m in {4, 5} the outcome depends on the handedness the eigensolver happened to return:
    that band is left out.  Expected: reflect iff the majority is improper, then project block by block, from Xd in
    numpy; equal up to a global rotation, so compared through the Gram matrix.  The other branch's Gram matrix is far
    away, so agreement also shows which branch ran."""
    import dcora_amd as da
    n, l, b, r = 9, 4, 3, 5
    k = (d + 1) * n + l + b
    sig = np.array([1.0, 0.8, 0.5][:d])
    sig_improper = sig * np.array([1.0] * (d - 1) + [-1.0])
    keep, flip = [0, 1, n // 2 - 1], [n, n - 1, n - n // 2 + 1]
    for m in keep + flip:
        rng = np.random.default_rng(100 * d + m)
        Xd = rng.standard_normal((d, k))
        improper = set(rng.permutation(n)[:m].tolist())
        for i in range(n):
            R = _so_numpy(rng.standard_normal((d, d)))
            Xd[:, d * i:d * i + d] = R * (sig_improper if i in improper else sig)
        Xd[:, d * n:d * n + l] *= np.exp(rng.uniform(-1, 1, l))
        lift = np.linalg.qr(rng.standard_normal((r, d)))[0]
        P = da.project_solution_raslam(lift @ Xd, r, d, n, l, b)
        assert P.shape == (d, k)
        dets = np.array([np.linalg.det(P[:, d * i:d * i + d]) for i in range(n)])
        assert (dets > 1 - 64 * EPS).all(), (m, dets)
        assert np.abs(np.linalg.norm(P[:, d * n:d * n + l], axis=0) - 1).max() <= 8 * EPS
        G = P.T @ P
        dist = {}
        for reflect in (False, True):
            E = _project_ra_numpy(Xd, d, n, l, reflect)
            dist[reflect] = np.abs(G - E.T @ E).max()
        want = m > n - m
        print("reflect d=%d m=%d: |G - G_kept| %.2e  |G - G_reflected| %.2e" % (d, m, dist[False], dist[True]))
        assert dist[want] <= 1e-10, (m, dist)
        assert dist[not want] > 1e-3, (m, dist)  # the branches are told apart


# ---- f. the second grid pass of k_polar ---------------------------------------------------------------------------------------
def test_polar_second_grid_pass(built):
    import dcora_amd as da
    from oracle import orc
    d, r = 3, 4
    # pose_grid caps the grid at kMaxPartials = 1024 workgroups of kBlock = 256 threads (dcora_amd/csrc/kernels.h), one
    # item per thread and pass: the last 257 blocks, and every translation, are reached by `it += gridDim.x * kBlock`
    first_pass = 1024 * 256
    n = first_pass + 257
    rng = np.random.default_rng(5)
    Q = np.linalg.qr(rng.standard_normal((n, r, d)))[0]
    A = Q + 0.2 * rng.standard_normal((n, r, d))  # kappa <= about 2
    T = rng.standard_normal((r, n))
    M = bf.se_matrix(A, T)
    out = da.manifold_project(r, d, n, M)
    ref = orc.project_to_manifold(r, d, n, M)
    err = bf.block_err(bf.se_blocks(out, d), bf.se_blocks(ref, d))
    print("second pass: max block error %.3e (first pass %.3e)" % (err[first_pass:].max(), err[:first_pass].max()))
    assert err[first_pass:].max() <= 1e-12, "blocks of the second grid pass"
    assert err[:first_pass].max() <= 1e-12
    assert np.array_equal(out[:, d::d + 1], T)
