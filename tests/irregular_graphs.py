"""Pose graphs with irregular block rows for the block-CSR kernels (n >= 8192), and an extended-precision reference of
X Q + G and of what the evaluation kernels derive from it.

graph(d, n, seed, variant): an odometry chain 0 - 1 - ... - n-1 plus loop closures, random precisions and weights in
[0.5, 1.5] as in test_run_waits_gpu._graph.  The block-row populations of Q (blocks per block row = 1 + the number of
distinct neighbours of the pose) are fixed by construction and asserted on the row pointers of the built Q:
  1   pose ISOLATED has no measurement at all: build_Q_pgo accepts it, but keeps the diagonal of Q as explicit zeros,
      so its block row holds one block of zeros and no block row of a built Q is ever empty
  2   its chain neighbours ISOLATED - 1 and ISOLATED + 1, the two leaves the cut chain leaves inside the graph
  3   every other pose of the chain that no loop closure touches
  4   the far end of every loop closure (each far end is used once, and is no chain neighbour of a hub)
  5, 6, 8, 9   the poses of MINOR
  41 (= 4 k + 1), 100, 118, 127   the hubs of the `small` variant: no scalar row exceeds kLongRow = 512 entries
  160, 161, 330                   the hubs the `long` variant adds (and it moves 41, 100, 118 to other poses)
Hubs sit at pose 0, at pose n - 1, at the first pose of a 32-pose chunk and at the last pose of one.  At least one
tile boundary of k_fused_hess_bsr (kBsrTile = 160 blocks, counted from the first block of the workgroup's 32 poses)
falls strictly inside a pose's row; the `long` variant has rows longer than one tile.  The graph stays connected apart
from the isolated pose: the hubs' closures bridge the cut.

reference(Q, X, G, ...): E = X Q + G accumulated in double-double (two-sum / two-product) over the entries of Q, error
far below 2^-60 A with A = |X| |Q| + |G|; the pose blocks derived from it in np.longdouble."""
import numpy as np

TILE = 160          # kBsrTile
CHUNK = 32          # kPosesPerBlock
ISOLATED = 3000
MINOR = {96: 5, 200: 6, 304: 8, 400: 9}
SIZES = (8192, 8193, 8221, 16400)


def hubs(variant, n):
    """pose -> blocks of its block row"""
    if variant == "small":
        return {0: 41, 2047: 127, 4096: 100, n - 1: 118}
    assert variant == "long", variant
    return {0: 330, 2047: 127, 4096: 160, n - 1: 161, 1000: 41, 5119: 118, 6144: 100}


def block_rows(Q, d):
    """(bp, bc) of the block form of the CSR matrix Q with (d+1) x (d+1) blocks: a block exists where an entry does"""
    dh = d + 1
    nb = Q.n // dh
    rp, ci = np.asarray(Q.rp, np.int64), np.asarray(Q.ci, np.int64)
    rows = np.repeat(np.arange(Q.n, dtype=np.int64), np.diff(rp))
    keys = np.unique((rows // dh) * nb + ci // dh)
    bp = np.zeros(nb + 1, np.int64)
    np.cumsum(np.bincount(keys // nb, minlength=nb), out=bp[1:])
    return bp, keys % nb


def cut_rows(bp):
    """poses whose block row a tile boundary of k_fused_hess_bsr cuts strictly inside: the workgroup of poses
    32 j .. 32 j + 31 stages blocks bp[32 j] + 160 m .. of its rows per pass"""
    n = len(bp) - 1
    i = np.arange(n)
    off = bp[i] - bp[CHUNK * (i // CHUNK)]
    end = off + (bp[i + 1] - bp[i])
    first = (off // TILE + 1) * TILE   # the first boundary behind the row's first block
    return i[first < end]


def _rot(rng, d, scale):
    q, u = np.linalg.qr(np.eye(d) + scale * rng.standard_normal((d, d)))
    q = q * np.sign(np.diag(u))
    if np.linalg.det(q) < 0:
        q[:, d - 1] = -q[:, d - 1]
    return q


_graphs = {}


def graph(d, n, seed=0, variant="small"):
    """(ds, Q, pops): the da.Dataset, its build_Q_pgo and the blocks per block row; built once per argument set"""
    key = (d, n, seed, variant)
    if key in _graphs:
        return _graphs[key]
    import dcora_amd as da
    rng = np.random.default_rng(90000 + 1000 * seed + 10 * n + d)
    hub = hubs(variant, n)
    want = dict(hub)
    want.update(MINOR)
    leaves = (ISOLATED - 1, ISOLATED + 1)
    chain = [(i, i + 1) for i in range(n - 1) if ISOLATED not in (i, i + 1)]
    deg = np.zeros(n, int)
    for i, j in chain:
        deg[i] += 1
        deg[j] += 1
    special = set(want) | {ISOLATED, 0, n - 1} | set(leaves)
    near = {p + s for p in special for s in (-1, 0, 1)}
    far = [int(j) for j in rng.permutation(n) if int(j) not in near]
    closures = []
    for p in sorted(want):
        for _ in range(want[p] - 1 - deg[p]):
            j = far.pop()
            closures.append((p, j) if rng.random() < 0.5 else (j, p))
    far_ends = sorted({i if j in want else j for i, j in closures})
    Rg = [_rot(rng, d, 0.8) for _ in range(n)]
    tg = 3.0 * rng.standard_normal((n, d))
    ids, vals = [], []
    for i, j in chain + closures:
        Rij = Rg[i].T @ Rg[j] @ _rot(rng, d, 0.05)
        tij = Rg[i].T @ (tg[j] - tg[i]) + 0.05 * rng.standard_normal(d)
        ids.append([0, i, 0, j])
        vals.append(np.r_[Rij.T.reshape(-1), tij, rng.uniform(50, 150), rng.uniform(5, 15), rng.uniform(0.5, 1.5)])
    ds = da.Dataset(d, n, np.array(ids), np.array(vals))
    Q = da.build_Q_pgo(ds)
    bp, _ = block_rows(Q, d)
    pops = np.diff(bp)
    expect = np.full(n, 3)
    expect[ISOLATED] = 1
    expect[list(leaves)] = 2
    expect[far_ends] = 4
    for p, c in want.items():
        expect[p] = c
    bad = np.flatnonzero(pops != expect)
    assert bad.size == 0, (key, bad[:8], pops[bad[:8]], expect[bad[:8]])
    assert {1, 2, 3, 4, 5, 6, 8, 9, 41} <= set(pops.tolist())
    dh = d + 1
    if variant == "small":
        assert 100 <= pops.max() <= 127 and np.diff(np.asarray(Q.rp)).max() <= 512   # kLongRow
    else:
        assert {160, 161, 330} <= set(pops.tolist()) and pops.max() == 330
        assert d == 2 or np.diff(np.asarray(Q.rp)).max() > 512
    for p in (0, n - 1):
        assert pops[p] >= 41
    assert any(p % CHUNK == 0 and p > 0 for p in hub) and any(p % CHUNK == CHUNK - 1 for p in hub)
    cuts = cut_rows(bp)
    assert cuts.size > 0, key
    assert int(Q.n) == dh * n
    _graphs[key] = (ds, Q, pops)
    return _graphs[key]


# ---- the reference ---------------------------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a   # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def xq_extended(Q, X, G=None):
    """X Q + G in np.longdouble from a double-double accumulation: per output column j the exact products
    X[:, i] Q[i, j] (two-product) are added in double-double (two-sum), entry by entry in the order of the rows i.
    Each step errs by at most a few 2^-104 of the running absolute sum: far below 2^-60 A for the 1321 terms of the
    longest row here"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, \
        "np.longdouble is not an extended type here (eps %g): the reference needs 64 mantissa bits" % np.finfo(np.longdouble).eps
    At = Q.to_scipy().tocsc()   # column j of Q: the terms of output column j
    At.sort_indices()
    ptr, idx, val = At.indptr.astype(np.int64), At.indices, At.data
    r, k = X.shape
    X = np.asarray(X, np.float64)
    hi = np.zeros((r, k)) if G is None else np.array(G, np.float64)
    lo = np.zeros((r, k))
    length = np.diff(ptr)
    order = np.argsort(-length, kind="stable")   # columns by falling length: step p works on a prefix
    for p in range(int(length.max()) if k else 0):
        m = int(np.searchsorted(-length[order], -p, side="left"))   # columns with length > p
        cols = order[:m]
        e = ptr[cols] + p
        prod, perr = _two_prod(X[:, idx[e]], val[e][None, :])
        s, serr = _two_sum(hi[:, cols], prod)
        t = lo[:, cols] + (serr + perr)
        h2 = s + t
        lo[:, cols] = t - (h2 - s)
        hi[:, cols] = h2
    return hi.astype(np.longdouble) + lo.astype(np.longdouble)


def _abs_sum(Q, X, G=None):
    A = (abs(Q.to_scipy()).T @ np.abs(X).T).T
    return A if G is None else A + np.abs(G)


def _pose_view(M, d):
    """r x (d+1) n -> n x r x (d+1)"""
    r = M.shape[0]
    return M.reshape(r, -1, d + 1).transpose(1, 0, 2)


def _sym(M):
    return (M + M.transpose(0, 2, 1)) / 2


def reference(Q, X, G, d, V=None, pose_start=None):
    """dict of: E = X Q + G (np.longdouble) and its per-entry absolute sum A = |X| |Q| + |G|; S = sym(Y_i^T E_i) per
    pose (n x d x d), RG = the Riemannian gradient, cost2 = 2 f = <X Q, X> + 2 <G, X> and f_abs = the sum of the
    absolute values of the terms of f, gradnorm = |RG|, block_norms = the |RG| of the pose ranges pose_start[a] ..
    pose_start[a+1]; with V also VQ, its absolute sum AV, and H = Proj_X(V Q - V_rot S)"""
    L = np.longdouble
    r, k = X.shape
    dh = d + 1
    Xl = np.asarray(X, L)
    XQ = xq_extended(Q, X, None)
    E = XQ if G is None else XQ + np.asarray(G, L)   # (one more rounding of 2^-64 relative)
    AQ = _abs_sum(Q, X)
    A = AQ if G is None else AQ + np.abs(G)
    Ep, Xp = _pose_view(E, d), _pose_view(Xl, d)
    Y = Xp[:, :, :d]
    S = _sym(np.matmul(Y.transpose(0, 2, 1), Ep[:, :, :d]))
    RGp = Ep.copy()
    RGp[:, :, :d] -= np.matmul(Y, S)
    RG = RGp.transpose(1, 0, 2).reshape(r, k)
    out = dict(E=E, A=A, S=S, RG=RG)
    out["cost2"] = float((XQ * Xl).sum() + (0 if G is None else 2 * (np.asarray(G, L) * Xl).sum()))
    out["f_abs"] = float(0.5 * (np.abs(X) * AQ).sum() + (0 if G is None else (np.abs(X) * np.abs(G)).sum()))
    pn = (RGp * RGp).sum(axis=(1, 2))
    out["pose_norm2"] = pn
    out["gradnorm"] = float(np.sqrt(pn.sum()))
    if pose_start is not None:
        out["block_norms"] = np.array([float(np.sqrt(pn[a:b].sum())) for a, b in zip(pose_start[:-1], pose_start[1:])])
    if V is not None:
        VQ = xq_extended(Q, V, None)
        Vp = _pose_view(np.asarray(V, L), d)
        Wp = _pose_view(VQ, d).copy()
        Wp[:, :, :d] -= np.matmul(Vp[:, :, :d], S)
        Wp[:, :, :d] -= np.matmul(Y, _sym(np.matmul(Y.transpose(0, 2, 1), Wp[:, :, :d])))
        AV = _abs_sum(Q, V)
        AVp = _pose_view(AV, d).copy()
        AVp[:, :, :d] += np.matmul(np.abs(_pose_view(np.asarray(V, np.float64), d)[:, :, :d]), np.abs(S).astype(np.float64))
        out.update(VQ=VQ, AV=AVp.transpose(1, 0, 2).reshape(r, k), H=Wp.transpose(1, 0, 2).reshape(r, k))
    return out


def pose_err(M, ref, d):
    """largest absolute error per pose (n values) of the r x (d+1) n matrix M against the extended reference"""
    D = np.abs(np.asarray(M, np.longdouble) - ref).astype(np.float64)
    return _pose_view(D, d).max(axis=(1, 2))


def pose_max(M, d):
    return _pose_view(np.abs(np.asarray(M, np.float64)), d).max(axis=(1, 2))


def gamma(m):
    u = 2.0 ** -53
    return m * u / (1 - m * u)


def agent_ranges(n, R):
    """pose_start of the session's contiguous split: n // R poses per agent, the last one takes the rest"""
    per = n // R
    return np.array([a * per for a in range(R)] + [n])


def eval_ranges(n, R):
    """the pose ranges of the workgroups of the central evaluation with the agent split (launch_fused_grad_bsr):
    grid = ceil(n / 32) workgroups, wpa = grid // R per agent, agent a's poses dealt evenly over its wpa workgroups"""
    ps = agent_ranges(n, R)
    wpa = max(1, -(-n // CHUNK) // R)
    out = []
    for a in range(R):
        lo, hi = int(ps[a]), int(ps[a + 1])
        out += [(lo + (hi - lo) * s // wpa, lo + (hi - lo) * (s + 1) // wpa) for s in range(wpa)]
    return out
