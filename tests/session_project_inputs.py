"""Inputs and numpy references of the session projection tests (tests/test_session_project_cpu.py checks them without a
GPU; tests/test_session_project_gpu.py uses them).

A point is X = Ylift Xd + nu noise in the style of session_round_inputs.lifted_point: Ylift a random Stiefel matrix
(r x d), Xd random poses of SE(d) -- here with UNIT translations, so that the d leading eigenvalues of G = X X^T stay
within a factor of the largest: with translations of scale 10 and one pose, G = Ylift (I + t t^T) Ylift^T has
sigma_d^2 / sigma_1^2 = 1 / 101 and the rule below could not hold.  nu in {0, 1e-3}.

Two rules make the projection well conditioned, so that the reference alone stays inside every bound of the GPU tests:
  gap       sigma_d^2 - sigma_{d+1}^2 >= 0.25 sigma_1^2 of G (the subspace V_d moves by |dG| / gap);
  blocks    every truncated rotation block V_d^T Y_i has sigma_min >= 0.5 (its polar factor moves by |dB| / sigma_min).

The reference is float64 eigh of the longdouble Gram matrix, then the block projection of
tests/test_block_factors_gpu.py's _project_ra_numpy (SVD with the determinant's sign on the last direction), in either
ordering.  The reflect family is that test's section e: n = 9 blocks of which m are improper, m in
{0, 1, n/2 - 1, n - n/2 + 1, n - 1, n}; for m in {4, 5} the outcome depends on the handedness the eigensolver happened
to return, so that band is left out."""
import numpy as np

import session_round_inputs as sri

EPS = sri.EPS
LD = np.longdouble
SIZES = sri.SIZES
DIMS = sri.DIMS
NUS = [0.0, 1e-3]
GAP, BLOCK_SIGMA_MIN = 0.25, 0.5
REFLECT_DIMS = dict(n=9, l=4, b=3, r=5)
REFLECT_KEEP = [0, 1, REFLECT_DIMS["n"] // 2 - 1]
REFLECT_FLIP = [REFLECT_DIMS["n"], REFLECT_DIMS["n"] - 1, REFLECT_DIMS["n"] - REFLECT_DIMS["n"] // 2 + 1]


def ranks_of(d):
    return [d, 5, 16]


def seed_of(d, r, n, nu):
    return sri.seed_of(d, r, n) + (50000 if nu else 0)


def lifted_point(d, r, n, seed, nu):
    """X (r x (d+1) n, SE ordering) = Ylift [R_i | t_i] + nu noise, |t_i| = 1"""
    rng = np.random.default_rng(seed)
    Ylift = np.linalg.qr(rng.standard_normal((r, d)))[0]
    T = np.zeros((d, (d + 1) * n))
    T.reshape(d, n, d + 1)[:, :, :d] = sri.random_rotations(rng, d, n).transpose(1, 0, 2)
    t = rng.standard_normal((d, n))
    T[:, d::d + 1] = t / np.linalg.norm(t, axis=0, keepdims=True)
    return Ylift @ T + nu * rng.standard_normal((r, (d + 1) * n))


def size_cases():
    return [(d, r, n, nu) for d in DIMS for r in ranks_of(d) for n in SIZES for nu in NUS]


def chunk_sizes(d, chunk):
    """pose counts whose k = (d + 1) n lies below 4 (where d allows), is no multiple of 4, lies next below, at (where
    d + 1 divides the chunk) and next above a workgroup's chunk, and at two chunks plus a remainder"""
    w = d + 1
    ns = {1, 3, (chunk - 1) // w, chunk // w, chunk // w + 1, (2 * chunk) // w + 5}
    return sorted(ns)


# ---- orderings --------------------------------------------------------------------------------------------------------------
def ra_from_se(X, d, n):
    """[rotations | translations] of an SE-ordered matrix: the RA ordering with l = b = 0"""
    rows = X.shape[0]
    out = np.zeros_like(X)
    out[:, :d * n] = X.reshape(rows, n, d + 1)[:, :, :d].reshape(rows, d * n)
    out[:, d * n:] = X[:, d::d + 1]
    return out


def rotation_columns(d, n, l, se):
    """(n, d) column indices of the rotation blocks"""
    i = np.arange(n)[:, None]
    return i * (d + 1) + np.arange(d)[None, :] if se else i * d + np.arange(d)[None, :]


def sphere_columns(d, n, l, se):
    return np.arange(0) if se else d * n + np.arange(l)


def rotation_blocks(P, d, n, l, se):
    """(n, rows, d)"""
    return np.ascontiguousarray(P[:, rotation_columns(d, n, l, se)].transpose(1, 0, 2))


# ---- the reference ---------------------------------------------------------------------------------------------------------
def gram_ld(X):
    Xl = np.asarray(X, LD)
    return Xl @ Xl.T


def gram_bound(X):
    """(k + 2) eps (|X| |X|^T): the standard bound for a length-k inner product in any summation order"""
    A = np.abs(np.asarray(X, LD))
    return (X.shape[1] + 2) * EPS * (A @ A.T)


def eig_descending(G):
    """float64 eigh of G (longdouble or double) -> (values descending, vectors as columns)"""
    w, V = np.linalg.eigh(np.asarray(G, np.float64))
    return w[::-1].copy(), V[:, ::-1].copy()


def eig_gap(X, d):
    """(sigma_d^2 - sigma_{d+1}^2) / sigma_1^2 of G; at r == d the next eigenvalue is none (0)"""
    w, _ = eig_descending(gram_ld(X))
    nxt = w[d] if len(w) > d else 0.0
    return (w[d - 1] - nxt) / w[0]


def so_numpy(B):
    U, _, Vt = np.linalg.svd(B)
    D = np.eye(B.shape[0])
    D[-1, -1] = np.sign(np.linalg.det(U @ Vt))
    return U @ D @ Vt


def project_blocks(Xd, d, n, l, se, reflect):
    """_project_ra_numpy of tests/test_block_factors_gpu.py in either ordering: optional reflection of the last row, the
    rotation blocks projected to SO(d), the unit-sphere columns normalised (a zero column stays zero)"""
    P = np.array(Xd, np.float64)
    if reflect:
        P[d - 1] = -P[d - 1]
    cols = rotation_columns(d, n, l, se)
    for i in range(n):
        P[:, cols[i]] = so_numpy(P[:, cols[i]])
    sc = sphere_columns(d, n, l, se)
    if sc.size:
        nrm = np.linalg.norm(P[:, sc], axis=0, keepdims=True)
        P[:, sc] = np.where(nrm > 0, P[:, sc] / np.where(nrm > 0, nrm, 1.0), P[:, sc])
    return P


def truncate(X, basis):
    return (np.asarray(basis, LD).T @ np.asarray(X, LD)).astype(np.float64)


def positive_dets(Xd, d, n, l, se):
    return int((np.linalg.det(rotation_blocks(Xd, d, n, l, se)) > 0).sum())


def project_reference(X, d, n, l, se):
    """projectSolutionRASLAM in numpy -> dict(P d x k, basis r x d (reflection folded in), npos, reflect, sigma)"""
    w, V = eig_descending(gram_ld(X))
    basis = V[:, :d].copy()
    Xd = truncate(X, basis)
    npos = positive_dets(Xd, d, n, l, se)
    reflect = npos < n // 2
    if reflect:
        basis[:, d - 1] = -basis[:, d - 1]
    return dict(P=project_blocks(truncate(X, basis), d, n, l, se, False), basis=basis, npos=npos, reflect=reflect,
                sigma=np.sqrt(np.maximum(w, 0.0)))


def block_sigma_min(X, d, n, l, se):
    """least singular value over the truncated rotation blocks V_d^T Y_i"""
    _, V = eig_descending(gram_ld(X))
    blocks = rotation_blocks(truncate(X, V[:, :d]), d, n, l, se)
    return float(np.linalg.svd(blocks, compute_uv=False)[:, -1].min())


# ---- the reflect family ------------------------------------------------------------------------------------------------------
def reflect_case(d, m):
    """tests/test_block_factors_gpu.py section e: (Xd d x k in the RA ordering, X = lift Xd at r = 5); m of the n = 9
    rotation blocks are improper, R diag(1, .8[, -.5]), the rest proper, R diag(1, .8[, .5])"""
    n, l, b, r = (REFLECT_DIMS[key] for key in ("n", "l", "b", "r"))
    k = (d + 1) * n + l + b
    sig = np.array([1.0, 0.8, 0.5][:d])
    sig_improper = sig * np.array([1.0] * (d - 1) + [-1.0])
    rng = np.random.default_rng(100 * d + m)
    Xd = rng.standard_normal((d, k))
    improper = set(rng.permutation(n)[:m].tolist())
    for i in range(n):
        R = so_numpy(rng.standard_normal((d, d)))
        Xd[:, d * i:d * i + d] = R * (sig_improper if i in improper else sig)
    Xd[:, d * n:d * n + l] *= np.exp(rng.uniform(-1, 1, l))
    lift = np.linalg.qr(rng.standard_normal((r, d)))[0]
    return Xd, lift @ Xd


def reflect_expected(Xd, d, m):
    """(want, E_kept, E_reflected): reflect iff the majority is improper"""
    n, l = REFLECT_DIMS["n"], REFLECT_DIMS["l"]
    return m > n - m, project_blocks(Xd, d, n, l, False, False), project_blocks(Xd, d, n, l, False, True)

