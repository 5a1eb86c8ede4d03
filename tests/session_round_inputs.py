"""Inputs and numpy references of the session rounding tests (tests/test_session_round_cpu.py checks them without a
GPU; tests/test_session_round_gpu.py and tests/test_round_ranks_gpu.py use them).

The point of a case is X = Ylift T + 1e-3 noise: Ylift a random Stiefel matrix (r x d), T random SE(d) poses with
translations of scale 10.  Every R0^T Y_i is then a rotation up to 1e-3: well conditioned, determinant > 0, so the
projection onto SO(d) is the polar factor, which numpy forms in longdouble by Newton's iteration (numpy has no
longdouble SVD; at cond <= 2 the iteration converges quadratically in a handful of steps).

The rule the device is held to is tests/test_block_factors_gpu.py's: per group, device error <= 8 max(oracle_err_g,
eps cond_g) -- oracle_err_g what the CPU oracle (the same algorithm in IEEE double) achieves on the same blocks -- and
orthogonality error <= 8 oracle_orth; translations, unit spheres and landmarks <= 8 eps (|p| + |p_anchor|) per column,
all against longdouble."""
import numpy as np

import block_factors as bf

EPS = bf.EPS
LD = np.longdouble

# b. the sizes where the lane map (4 lanes per pose, 64 poses per workgroup) can go wrong
SIZES = [1, 15, 16, 17, 63, 64, 65, 257]
DIMS = [2, 3]


def ranks_of(d):
    return [d, 5, 16]


def seed_of(d, r, n):
    return 100000 * d + 1000 * r + n


def robots_of(n):
    """1, 2 or 3 agents, each with at least one pose"""
    return min(n, 1 + n % 3)


def size_cases():
    return [(d, r, n) for d in DIMS for r in ranks_of(d) for n in SIZES]


def random_rotations(rng, d, n):
    Q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    Q[:, :, -1] *= np.sign(np.linalg.det(Q))[:, None]
    return Q


def lifted_point(d, r, n, seed):
    """X (r x (d+1) n, SE ordering) = Ylift T + 1e-3 noise"""
    rng = np.random.default_rng(seed)
    Ylift = np.linalg.qr(rng.standard_normal((r, d)))[0]
    T = np.zeros((d, (d + 1) * n))
    T.reshape(d, n, d + 1)[:, :, :d] = random_rotations(rng, d, n).transpose(1, 0, 2)
    T[:, d::d + 1] = 10 * rng.standard_normal((d, n))
    return Ylift @ T + 1e-3 * rng.standard_normal((r, (d + 1) * n))


def chain_dataset(cls, d, n, seed):
    """odometry i -> i + 1 plus a few closures, from arrays (cls: dcora_amd.Dataset or the oracle's): the measurements
    only have to make a session; what they say plays no part in rounding"""
    rng = np.random.default_rng(seed + 7)
    pairs = [(i, i + 1) for i in range(n - 1)]
    pairs += [(i, i + j) for i, j in ((0, 3), (2, 9), (5, 40), (11, 200)) if i + j < n]
    m = len(pairs)
    ids = np.zeros((m, 4), np.int32)
    vals = np.zeros((m, d * d + d + 3))
    if m:
        ids[:, 1], ids[:, 3] = np.array(pairs).T
        vals[:, :d * d] = random_rotations(rng, d, m).transpose(0, 2, 1).reshape(m, d * d)
        vals[:, d * d:d * d + d] = rng.standard_normal((m, d))
        vals[:, d * d + d:] = [10.0, 5.0, 1.0]
    return cls(d, n, ids, vals)


def anchor_of(X, d, j):
    return np.array(X[:, (d + 1) * j:(d + 1) * (j + 1)])


def se_from_ra(X, d, n, l):
    """the poses of an RA-ordered matrix in the SE ordering"""
    out = np.zeros((X.shape[0], (d + 1) * n), X.dtype)
    out.reshape(X.shape[0], n, d + 1)[:, :, :d] = X[:, :d * n].reshape(X.shape[0], n, d)
    out[:, d::d + 1] = X[:, d * n + l:d * n + l + n]
    return out


# ---- longdouble -----------------------------------------------------------------------------------------------------------
def _inv_ld(M):
    """inverses of (nb, d, d) longdouble blocks by the adjugate, d in {2, 3}"""
    d = M.shape[1]
    if d == 2:
        det = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]
        adj = np.stack([np.stack([M[:, 1, 1], -M[:, 0, 1]], -1), np.stack([-M[:, 1, 0], M[:, 0, 0]], -1)], -2)
        return adj / det[:, None, None]
    c = np.empty_like(M)
    for i in range(3):
        for j in range(3):
            a, b = [(i + 1) % 3, (i + 2) % 3], [(j + 1) % 3, (j + 2) % 3]
            c[:, j, i] = M[:, a[0], b[0]] * M[:, a[1], b[1]] - M[:, a[0], b[1]] * M[:, a[1], b[0]]
    det = (M[:, 0, :] * c[:, :, 0]).sum(-1)
    return c / det[:, None, None]


def polar_ld(M, dtype=LD):
    """the orthogonal polar factor of well-conditioned (nb, d, d) blocks with det > 0, in longdouble (or in dtype):
    Newton's iteration U <- (U + U^-T) / 2, run to a fixed point (quadratic: a dozen steps are ample at cond <= 2)"""
    U = np.asarray(M, dtype)
    for _ in range(40):
        Un = (U + _inv_ld(U).transpose(0, 2, 1)) / 2
        if np.abs(Un - U).max() <= 4 * np.finfo(dtype).eps:
            return Un
        U = Un
    raise AssertionError("polar_ld did not converge: the blocks are not well conditioned")


def frame_blocks_ld(X, anchor, d):
    """(R0^T Y_i as (n, d, d), R0^T p_i - R0^T p_anchor as d x n) in longdouble, X in the SE ordering"""
    R0 = np.asarray(anchor, LD)[:, :d]
    M = R0.T @ np.asarray(X, LD)
    n = X.shape[1] // (d + 1)
    blocks = np.ascontiguousarray(M.reshape(d, n, d + 1)[:, :, :d].transpose(1, 0, 2))
    t = M[:, d::d + 1] - (R0.T @ np.asarray(anchor, LD)[:, d])[:, None]
    return blocks, t


def round_reference(X, anchor, d):
    """the rounded trajectory in longdouble: (rotations (n, d, d), translations d x n)"""
    blocks, t = frame_blocks_ld(X, anchor, d)
    return polar_ld(blocks), t


def points_reference(P, anchor, d, shift):
    """R0^T P (- R0^T p_anchor) in longdouble, P r x count"""
    R0 = np.asarray(anchor, LD)[:, :d]
    out = R0.T @ np.asarray(P, LD)
    return out - (R0.T @ np.asarray(anchor, LD)[:, d])[:, None] if shift else out


def sigma_range(X, anchor, d):
    """(least sigma_min, largest cond) of the blocks R0^T Y_i"""
    blocks, _ = frame_blocks_ld(X, anchor, d)
    s = np.linalg.svd(blocks.astype(np.float64), compute_uv=False)
    return s[:, -1].min(), (s[:, 0] / s[:, -1]).max()


def traj_blocks(T, d):
    """(rotations (n, d, d), translations d x n) of a trajectory d x (d+1) n"""
    return bf.se_blocks(T, d), T[:, d::d + 1]


def oracle_tolerance(X, anchor, d):
    """max(oracle_err_g, eps cond_g) for the group of all poses of X: the CPU oracle's own error against longdouble"""
    n = X.shape[1] // (d + 1)
    ref, _ = round_reference(X, anchor, d)
    Ro = bf.oracle_so(bf.se_blocks(X, d), anchor)
    err = float(bf.block_err(Ro.astype(LD), ref).max())
    assert n == len(ref)
    return max(err, EPS * sigma_range(X, anchor, d)[1])


def translation_bound(X, anchor, d):
    """8 eps (|p_i| + |p_anchor|) per pose"""
    return 8 * EPS * (np.linalg.norm(X[:, d::d + 1], axis=0) + np.linalg.norm(anchor[:, d]))


# ---- the rounded cost -----------------------------------------------------------------------------------------------------
def cost_reference(Z, Q, r):
    """(<Z Q, Z> in longdouble, the bound 8 (max row nnz + r) eps sum |Z| |Q| |Z^T|) for Z d x k and scipy Q"""
    Q = Q.tocsr()
    Zl = np.asarray(Z, LD)
    coo = Q.tocoo()
    val = coo.data.astype(LD)
    terms = (Zl[:, coo.row] * Zl[:, coo.col]).sum(axis=0) * val
    cost = terms.sum()
    absum = (np.abs(Zl[:, coo.row]) * np.abs(Zl[:, coo.col])).sum(axis=0) @ np.abs(val)
    row_nnz = int(np.diff(Q.indptr).max()) if Q.nnz else 0
    return cost, 8 * (row_nnz + r) * EPS * absum


def unit_columns(S):
    S = np.asarray(S, LD)
    return S / np.sqrt((S * S).sum(axis=0, keepdims=True))


def ra_point(T, S, L, d, n, normalise=True):
    """[rotations | spheres (normalised) | translations | landmarks] from the returned states, longdouble d x k"""
    R, t = T.reshape(d, n, d + 1)[:, :, :d].reshape(d, d * n), T[:, d::d + 1]
    Sp = unit_columns(S) if normalise and S.shape[1] else np.asarray(S, LD)
    return np.concatenate([np.asarray(R, LD), Sp, np.asarray(t, LD), np.asarray(L, LD)], axis=1)
