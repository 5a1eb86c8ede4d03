"""Range-aided layouts for the generic CSR kernels (k_spmm, k_spmm_dir, k_spmm_dir_fix with the row walk of csr_rows.h;
k_rgrad, k_tangent, k_hessfix), and an extended-precision reference of the operators of the mixed manifold
St(r,d)^n x OB(r,l) x R^(r x n) x R^(r x b) in the RA ordering [Y_1 .. Y_n | s_1 .. s_l | p_1 .. p_n | L_1 .. L_b].

graph(d, variant) -> (dims, Q, kinds, pops): dims = (d, n, l, b); Q a symmetric positive definite CSR assembled from an
edge list over the k scalar columns, Q = sum_e w_e (e_i - e_j)(e_i - e_j)^T + diag(eps), w_e = exp(uniform(-3, 3)),
eps_j = 1e-3 exp(uniform(-1, 1)): row j holds 1 + (distinct neighbours of j) entries and no stored zero; kinds[j] in
ROT, SPH, TRA, LMK; pops[j] the entry count of row j, from the edge list and asserted on the row pointers of Q.

Columns with a prescribed population ("targets") take no part in the base edges; their neighbours are drawn among the
other columns (the "fillers") of every kind, so Q couples rotation columns with Euclidean ones.  The base edges of the
fillers: the rotation columns of a pose with each other and with its translation, pose i with pose i + 1 (column by
column), every sphere with two translations and a landmark, every landmark with a translation and the next landmark.

variant        size                      targets
  edges        k about 2000 (dense       SHORT: populations 1 (diagonal alone), 2, 7, 8, 9, 16, 17 spread over the four
               preconditioner: <= 2200)  kinds; the last four translations 513, 777, 511, 512 and the first four
                                         landmarks 513, 519, 520, 521 (eight neighbouring rows of 4386 entries: a row
                                         block of three tiles); landmarks 10 .. 21 with 300 each, so that rows of
                                         <= 512 entries lie across the tile borders behind the hubs
  edges_sphere as edges                  and sphere 7 with 600
  edges_rot    as edges                  and a rotation column of pose 11 with 600 (the middle one at d = 3)
  deep         k about 8400              as edges, and landmark 5 joined to every filler and every other hub (> 8200),
                                         landmark 9 with 4100
  many         k about 1200              SHORT; 520 Euclidean columns M (translations and landmarks), each joined to
                                         the 256 before and the 256 behind it in M (cyclic) and to i % 10 further
                                         fillers, 513 .. 530 entries; rotation column 1 of pose 11 joined to all of M
  wide         k >= 16500                SHORT and landmark 0 with 513 on the sparse base: more than kMaxPartials = 1024
                                         row blocks in k_spmm_dir_fix at r = 15 and r = 16

In every variant n d and n d + l are no multiples of the rows per workgroup of k_spmm_dir_fix, RB = ((256 / r) / d) d,
for any r from d to 16: the borders rotation | sphere and sphere | translation lie inside a workgroup.

A slice of a long row (len > kLongRow = 512) holds per = ceil(len / 8) entries; 7 per < len for every len > 49, so the
last slice of a long row is shorter than the others and never empty.

reference(...): E = X Q + G from irregular_graphs.xq_extended (double-double), everything derived in np.longdouble."""
import numpy as np

import irregular_graphs as ig

ROT, SPH, TRA, LMK = 0, 1, 2, 3
KIND_NAMES = ("rotation", "sphere", "translation", "landmark")
VARIANTS = ("edges", "edges_sphere", "edges_rot", "deep", "many", "wide")
K_BLOCK, TILE, LONG_ROW, LONG_SPLIT, MAX_PARTIALS = 256, 1536, 512, 8, 1024   # kernels.h
SHORT_POPS = (1, 2, 7, 8, 9, 16, 17)
HUBS_TRA = (513, 777, 511, 512)      # the last four translations
HUBS_LMK = (513, 519, 520, 521)      # the first four landmarks
MID_LMK = (10, 12, 300)              # landmarks 10 .. 21 with 300 entries each
MANY = 520


def rb_fix(r, d):
    """rows per workgroup of k_spmm_dir_fix in the RA ordering"""
    return ((K_BLOCK // r) // d) * d


def _sizes(d, n0, l0, b):
    rs = range(d, 17)
    n = n0
    while any((n * d) % rb_fix(r, d) == 0 for r in rs):
        n += 1
    l = l0
    while any((n * d + l) % rb_fix(r, d) == 0 for r in rs):
        l += 1
    return n, l, b


def cols(dims):
    """first column of the spheres, the translations and the landmarks, and k"""
    d, n, l, b = dims
    return n * d, n * d + l, n * d + l + n, n * d + l + n + b


def column_kinds(dims):
    c1, c2, c3, k = cols(dims)
    kinds = np.full(k, LMK)
    kinds[:c1], kinds[c1:c2], kinds[c2:c3] = ROT, SPH, TRA
    return kinds


def short_targets(dims):
    """column -> population of the short rows: one or two in every kind, among them the last sphere (beside the first
    translation) and the last column of all"""
    d, n, l, b = dims
    c1, c2, c3, k = cols(dims)
    return {5 * d + 1: 1, 9 * d: 9, c1 + 3: 2, c1 + 4: 8, c2 - 1: 17, c2: 7, k - 1: 16}


def hub_targets(dims, variant):
    """column -> population of the hubs with a prescribed population (None: joined to every filler and every hub)"""
    d, n, l, b = dims
    c1, c2, c3, k = cols(dims)
    t = {}
    if variant in ("edges", "edges_sphere", "edges_rot", "deep"):
        t.update({c3 - 4 + i: p for i, p in enumerate(HUBS_TRA)})
        t.update({c3 + i: p for i, p in enumerate(HUBS_LMK)})
        t.update({c3 + MID_LMK[0] + i: MID_LMK[2] for i in range(MID_LMK[1])})
    if variant == "edges_sphere":
        t[c1 + 7] = 600
    if variant == "edges_rot":
        t[11 * d + 1] = 600
    if variant == "deep":
        t[c3 + 5] = None
        t[c3 + 9] = 4100
    if variant == "wide":
        t[c3] = 513
    return t


def tile_facts(rp, r):
    """(rows that a tile border of their row block cuts strictly inside, tiles of the largest row block) for k_spmm's
    row blocks of 256 / r rows, staged kSpmmTile = 1536 entries at a time from the block's first entry"""
    rp = np.asarray(rp, np.int64)
    k = len(rp) - 1
    RB = K_BLOCK // r
    j = np.arange(k)
    j0 = (j // RB) * RB
    off = rp[j] - rp[j0]
    end = off + (rp[j + 1] - rp[j])
    first = (off // TILE + 1) * TILE
    b0 = np.arange(0, k, RB)
    size = rp[np.minimum(b0 + RB, k)] - rp[b0]
    return j[first < end], int(-(-size.max() // TILE))


_graphs = {}


def graph(d, variant):
    key = (d, variant)
    if key in _graphs:
        return _graphs[key]
    import dcora_amd as da
    import scipy.sparse as sp
    assert variant in VARIANTS, variant
    rng = np.random.default_rng(7000 + 100 * VARIANTS.index(variant) + d)
    l0 = 41
    if variant == "deep":
        n0 = 1600 if d == 3 else 2000
        dims = _sizes(d, n0, l0, 8400 - (d + 1) * n0 - l0)
    elif variant == "many":
        n0 = 170 if d == 3 else 220
        dims = _sizes(d, n0, l0, 1200 - (d + 1) * n0 - l0)
    elif variant == "wide":
        n0 = 4000 if d == 3 else 5400
        dims = _sizes(d, n0, l0, 500)
    else:
        n0 = 400 if d == 3 else 520
        dims = _sizes(d, n0, l0, 2000 - (d + 1) * n0 - l0)
    dims = (d,) + dims
    _, n, l, b = dims
    c1, c2, c3, k = cols(dims)
    kinds = column_kinds(dims)
    short = short_targets(dims)
    hubs = hub_targets(dims, variant)
    assert not set(short) & set(hubs)
    target = np.zeros(k, bool)
    target[list(short) + list(hubs)] = True
    many = np.zeros(0, np.int64)
    in_many = np.zeros(k, bool)
    rot_hub = 11 * d + 1
    if variant == "many":
        target[rot_hub] = True
        many = np.flatnonzero(~target & (kinds >= TRA))[:MANY]
        assert many.size == MANY and (kinds[many] == TRA).any() and (kinds[many] == LMK).any()
        in_many[many] = True

    # ---- base edges of the fillers -------------------------------------------------------------------------------
    base = []
    for i in range(n):
        rc = [i * d + a for a in range(d)]
        base += [(rc[a], rc[c]) for a in range(d) for c in range(a + 1, d)]
        base += [(c, c2 + i) for c in rc]
        if i + 1 < n:
            base += [(c, c + d) for c in rc] + [(c2 + i, c2 + i + 1)]
    for i in range(l):
        base += [(c1 + i, c2 + (i * n) // l), (c1 + i, c2 + (7 * i + 3) % n), (c1 + i, c3 + i % b)]
    for i in range(b):
        base += [(c3 + i, c2 + (5 * i) % n)]
        if i + 1 < b:
            base.append((c3 + i, c3 + i + 1))
    adj = [set() for _ in range(k)]

    def join(i, j):
        assert i != j
        adj[i].add(int(j))
        adj[j].add(int(i))

    for i, j in base:
        if target[i] or target[j] or in_many[i] != in_many[j]:
            continue
        join(i, j)
    fillers = np.flatnonzero(~target & ~in_many)

    def draw(j, count):
        free = np.array([c for c in fillers if c not in adj[j]])
        assert 0 <= count <= free.size, (variant, j, count, free.size)
        for c in rng.choice(free, count, replace=False):
            join(j, c)

    # ---- the targets ---------------------------------------------------------------------------------------------
    if variant == "many":
        for q, j in enumerate(many):
            for s in range(1, 257):
                join(j, many[(q + s) % MANY])
        for j in many:
            join(rot_hub, j)
        for q, j in enumerate(many):
            draw(j, q % 10)
    for j in [c for c, p in hubs.items() if p is None]:
        for c in fillers:
            join(j, c)
        for c in hubs:
            if c != j:
                join(j, c)
    for j, p in sorted(hubs.items(), key=lambda e: -(e[1] or 0)):
        if p is not None:
            draw(j, p - 1 - len(adj[j]))
    for j, p in short.items():
        draw(j, p - 1)

    # ---- Q -------------------------------------------------------------------------------------------------------
    ej = np.array([j for i in range(k) for j in sorted(adj[i]) if i < j], np.int64)
    ei = np.repeat(np.arange(k), [sum(1 for j in adj[i] if j > i) for i in range(k)])
    w = np.exp(rng.uniform(-3, 3, ei.size))
    diag = 1e-3 * np.exp(rng.uniform(-1, 1, k))
    np.add.at(diag, ei, w)
    np.add.at(diag, ej, w)
    A = sp.coo_matrix((np.r_[-w, -w, diag], (np.r_[ei, ej, np.arange(k)], np.r_[ej, ei, np.arange(k)])), shape=(k, k)).tocsr()
    A.sort_indices()
    Q = da.Csr.from_scipy(A)
    pops = np.array([1 + len(a) for a in adj])

    # ---- what the variant promises -------------------------------------------------------------------------------
    rp = np.asarray(Q.rp, np.int64)
    assert np.array_equal(np.diff(rp), pops), (key, np.flatnonzero(np.diff(rp) != pops)[:8])
    assert np.all(Q.v != 0) and abs(A - A.T).max() == 0
    for j, p in short.items():
        assert pops[j] == p, (key, j, pops[j], p)
    for j, p in hubs.items():
        assert p is None or pops[j] == p, (key, j, pops[j], p)
    assert set(kinds[list(short)]) == {ROT, SPH, TRA, LMK}
    for r in range(d, 17):
        assert (n * d) % rb_fix(r, d) and (n * d + l) % rb_fix(r, d), (key, r)
    _graphs[key] = (dims, Q, kinds, pops)
    return _graphs[key]


# ---- the reference ---------------------------------------------------------------------------------------------------
def _blocks(M, n, d):
    """r x n d -> n x r x d"""
    return M.reshape(M.shape[0], n, d).transpose(1, 0, 2)


def _unblocks(B):
    n, r, d = B.shape
    return B.transpose(1, 0, 2).reshape(r, n * d)


def _sym(M):
    return (M + M.transpose(0, 2, 1)) / 2


def _project(Xl, W, S_of, dims):
    """Proj_X(W): W_i - Y_i sym(Y_i^T W_i) per rotation, w - x <x, w> per sphere, w per Euclidean column"""
    d, n, l, b = dims
    c1, c2, _, _ = cols(dims)
    out = W.copy()
    Y = _blocks(Xl[:, :c1], n, d)
    out[:, :c1] -= _unblocks(np.matmul(Y, S_of(np.matmul(Y.transpose(0, 2, 1), _blocks(W[:, :c1], n, d)))))
    out[:, c1:c2] -= Xl[:, c1:c2] * (Xl[:, c1:c2] * W[:, c1:c2]).sum(axis=0)
    return out


def tangent(X, U, dims):
    """the tangent projection of U at X in np.longdouble"""
    L = np.longdouble
    return _project(np.asarray(X, L), np.asarray(U, L), _sym, dims)


def tangent_abs(X, U, dims):
    """the absolute sums of the terms of tangent(): |U| + |Y| sym(|Y|^T |U|), |u| + |x| <|x|, |u|>, |u|"""
    aX, aU = np.abs(np.asarray(X, np.float64)), np.abs(np.asarray(U, np.float64))
    return 2 * aU - _project(aX, aU, _sym, dims)   # (_project subtracts what is added here)


def reference(Q, X, G, dims, V=None, XQ=None):
    """dict, everything in np.longdouble unless it is an absolute sum (double): E = X Q + G and A = |X| |Q| + |G|;
    S (n x d x d) = sym(Y_i^T E_i) and s (l) = <x_i, e_i>, with the absolute sums S_abs, s_abs of their terms; RG the
    Riemannian gradient, gradnorm; cost2 = 2 f = <X Q, X> + 2 <G, X> and f_abs, the absolute sum of the terms of f;
    with V: VQ, H = Proj_X(V Q - V S) (V s on the spheres), AV = |V| |Q| + |V| |S| per entry, VH = <V, H> and VH_abs =
    sum |V| (AV + the absolute sums of the projection's terms)"""
    L = np.longdouble
    d, n, l, b = dims
    c1, c2, _, k = cols(dims)
    assert X.shape[1] == k == Q.n
    Xl = np.asarray(X, L)
    aX = np.abs(np.asarray(X, np.float64))
    XQ = ig.xq_extended(Q, X, None) if XQ is None else XQ   # (X Q of an earlier call on the same X)
    out = {}
    E = XQ if G is None else XQ + np.asarray(G, L)
    AQ = ig._abs_sum(Q, X)
    A = AQ if G is None else AQ + np.abs(G)
    Y, aY = _blocks(Xl[:, :c1], n, d), _blocks(aX[:, :c1], n, d)
    S = _sym(np.matmul(Y.transpose(0, 2, 1), _blocks(E[:, :c1], n, d)))
    s = (Xl[:, c1:c2] * E[:, c1:c2]).sum(axis=0)
    out.update(XQ=XQ, E=E, A=A, S=S, s=s)
    out["S_abs"] = _sym(np.matmul(aY.transpose(0, 2, 1), _blocks(A[:, :c1], n, d)))
    out["s_abs"] = (aX[:, c1:c2] * A[:, c1:c2]).sum(axis=0)
    RG = E.copy()
    RG[:, :c1] -= _unblocks(np.matmul(Y, S))
    RG[:, c1:c2] -= Xl[:, c1:c2] * s
    out["RG"] = RG
    out["gradnorm"] = float(np.sqrt((RG * RG).sum()))
    out["cost2"] = float((XQ * Xl).sum() + (0 if G is None else 2 * (np.asarray(G, L) * Xl).sum()))
    out["f_abs"] = float(0.5 * (aX * AQ).sum() + (0 if G is None else (aX * np.abs(G)).sum()))
    if V is not None:
        Vl, aV = np.asarray(V, L), np.abs(np.asarray(V, np.float64))
        VQ = ig.xq_extended(Q, V, None)
        T = VQ.copy()
        T[:, :c1] -= _unblocks(np.matmul(_blocks(Vl[:, :c1], n, d), S))
        T[:, c1:c2] -= Vl[:, c1:c2] * s
        H = _project(Xl, T, _sym, dims)
        AV = ig._abs_sum(Q, V)
        AV[:, :c1] += _unblocks(np.matmul(_blocks(aV[:, :c1], n, d), np.abs(S).astype(np.float64)))
        AV[:, c1:c2] += aV[:, c1:c2] * np.abs(s).astype(np.float64)
        AH = AV.copy()   # and the terms of the projection: |Y| sym(|Y|^T AV), |x| <|x|, AV>
        AH[:, :c1] += _unblocks(np.matmul(aY, _sym(np.matmul(aY.transpose(0, 2, 1), _blocks(AV[:, :c1], n, d)))))
        AH[:, c1:c2] += aX[:, c1:c2] * (aX[:, c1:c2] * AV[:, c1:c2]).sum(axis=0)
        out.update(VQ=VQ, H=H, AV=AV, VH=float((Vl * H).sum()), VH_abs=float((aV * AH).sum()))
    return out


# ---- items: n rotation blocks, l spheres, n translations, b landmarks ------------------------------------------------
def item_max(M, dims):
    """largest absolute value per item of the r x k matrix M"""
    d, n, l, b = dims
    c1 = n * d
    m = np.abs(np.asarray(M)).max(axis=0)
    return np.r_[m[:c1].reshape(n, d).max(axis=1), m[c1:]].astype(np.float64)


def item_err(M, ref, dims):
    return item_max(np.asarray(M, np.longdouble) - ref, dims)


def item_groups(dims, kinds, pops):
    """(kind, population) per item; a rotation block counts with the longest row of its d columns"""
    d, n, l, b = dims
    c1 = n * d
    return np.r_[kinds[:c1:d], kinds[c1:]], np.r_[pops[:c1].reshape(n, d).max(axis=1), pops[c1:]]


def random_point(orc, r, dims, seed):
    d, n, l, b = dims
    rng = np.random.default_rng(seed)
    return orc.project_to_manifold(r, d, n, rng.uniform(-1, 1, (r, cols(dims)[3])), l=l, b=b)


# ---- the dual certificate ------------------------------------------------------------------------------------------------
def _lambda_reference(ref, Qs, dims):
    """Q - Lambda(X) as a dense k x k longdouble image of the rotation blocks' and spheres' entries alone: (rows, cols,
    values, absolute sums)"""
    d, n, l, b = dims
    c1 = n * d
    I, J, Vv, Ab = [], [], [], []
    for i in range(n):
        for a in range(d):
            for c in range(d):
                I.append(i * d + a)
                J.append(i * d + c)
                Vv.append(ref["S"][i, a, c])
                Ab.append(ref["S_abs"][i, a, c])
    for i in range(l):
        I.append(c1 + i)
        J.append(c1 + i)
        Vv.append(ref["s"][i])
        Ab.append(ref["s_abs"][i])
    return np.array(I), np.array(J), np.array(Vv, np.longdouble), np.array(Ab)


def check_certificate(S, Q, ref, dims, pops, r, tag):
    """S = Q - Lambda(X): the pattern is Q's and Lambda's together, every entry outside Lambda's is Q's bit for bit,
    every entry of Lambda lies within gamma_m (its absolute sum + |Q entry|), m = the row's population + r + 3 (the
    entry of X Q, the r products of each of the two Gram entries, their mean, and the subtraction from Q).  Returns
    the largest ratio"""
    import scipy.sparse as sp
    Qs, Ss = Q.to_scipy().tocsr(), S.to_scipy().tocsr()
    k = Q.n
    I, J, lam, lam_abs = _lambda_reference(ref, Qs, dims)
    mask = sp.csr_matrix((np.ones(len(I)), (I, J)), shape=(k, k))
    pat = lambda M: set(zip(*M.nonzero()))
    assert pat(Ss) <= pat(Qs) | pat(mask), tag
    outside = Qs - Qs.multiply(mask)
    diff = (Ss - Ss.multiply(mask)) - outside
    assert diff.nnz == 0 or abs(diff).max() == 0, tag   # the entries of Q are carried over exactly
    q = np.asarray(Qs[I, J]).ravel()
    got = np.asarray(Ss[I, J]).ravel()
    err = np.abs(got.astype(np.longdouble) - (q.astype(np.longdouble) - lam)).astype(np.float64)
    m = np.maximum(pops[I], pops[J]) + r + 3
    bound = ig.gamma(m) * (lam_abs + np.abs(q))
    ratio = float((err / bound).max())
    assert np.all(err <= bound), (tag, ratio)
    return ratio
