"""Sparse symmetric matrices whose factors are known exactly, for the device Cholesky and both preconditioner inverses.

A = L D L^T with L unit lower triangular, its off-diagonal entries in {+-1/4, +-1/2} on the pattern of a pose graph, and
D = diag(2^e_i), e_i integers in [-a, a].  Everything is formed in int64 (L scaled by 4, D by 2^a) and divided by
16 * 2^a at the end, after the bound |L| D |L|^T < 2^53 (scaled) has been asserted, so A is exact in float64 and so are
V = A W for small-integer W, det A = 2^(sum e_i) and, by Sylvester, the inertia of A under ANY elimination order: the
library's nested dissection does not have to agree with the order of L.

  * L's order is a seeded permutation of the unknowns (unrelated to the library's), hub poses last (a hub that came
    early would fill A);
  * for block size b the diagonal blocks of L are full and a pose-pose edge couples slot c of one pose to slot c of
    the other; a scalar unknown (unit sphere, landmark) is coupled to every unknown of its poses.  The block graph of A
    is then the pose graph with the fill of |L| |L|^T, every pose block of A is coupled to its neighbours' through the
    full diagonal blocks, and a row of L stays short.  (Full b x b cross blocks in L, +-1/2 as likely as +-1/4, were
    tried first: kappa_2 reaches 1.5e10 on the lattice and 2.4e11 with hubs at a = 12, and the condition the sign
    sweeps have to meet, |lambda_min| >= 1e3 n eps |A|_2, cannot hold beyond kappa_2 = 1 / (1e3 n eps), 1.1e9 at
    n = 4000.  So +-1/2 is drawn once in eight, the hubs' long rows hold +-1/4 only, and the cross blocks of L are
    diagonal: kappa_2 <= 6.4e8 with hubs, 1.4e8 elsewhere.);
  * A's pattern is that of |L| |L|^T with explicit zeros kept, so every scale group and every sign sweep of a case has
    ONE pattern (one cached analysis) whatever cancels;
  * sign sweeps: D_pp -> -2^-a (exactly: anything smaller in magnitude would vanish under the integer scaling), and the
    positive twin D_pp -> +2^-a, for a position p of L's order.

tests/golden/exact_factors_ref.npz (make_exact_factors_ref.py) records, per case and scale group, kappa_2(A) and what
LAPACK achieves on the same matrix; tol_solve / tol_logdet turn them into the bounds of the tests."""
import hashlib
import os

import numpy as np
import scipy.sparse as sp

EPS = np.finfo(np.float64).eps
LN2 = float(np.log(2.0))
SCALES = (0, 4, 12)
REF_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_factors_ref.npz")
W_COLS = 16  # W is drawn once per case with 16 columns; rank r uses the first r


def _grid(*shape):
    """edges of a lattice of the given shape, vertices numbered in C order"""
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    e = []
    for ax in range(len(shape)):
        a = np.take(idx, range(shape[ax] - 1), axis=ax).ravel()
        b = np.take(idx, range(1, shape[ax]), axis=ax).ravel()
        e += list(zip(a.tolist(), b.tolist()))
    return e


# id -> (d, poses, pose-pose edges, hub poses, l, b); what each reaches is in CASES_DOC
def _spec(cid):
    if cid == "g16":
        return 3, 16, _grid(4, 4), 0, 0, 0
    if cid == "g17":
        return 3, 17, _grid(17), 0, 0, 0
    if cid == "g144":
        return 3, 144, _grid(12, 12), 0, 0, 0
    if cid == "g145":
        return 3, 145, _grid(12, 12) + [(143, 144)], 0, 0, 0
    if cid == "p171":
        return 2, 171, _grid(3, 57), 0, 0, 0
    if cid == "g550":
        return 3, 550, _grid(22, 25), 0, 0, 0
    if cid == "l1000":
        return 3, 1000, _grid(10, 10, 10), 0, 0, 0
    if cid == "h144":
        e = _grid(12, 12)
        for h in (144, 145):
            e += [(i, h) for i in range(144)]
        return 3, 146, e + [(144, 145)], 2, 0, 0
    if cid == "ra":
        return 3, 100, _grid(10, 10), 0, 9, 5
    raise KeyError(cid)


CASES = ("g16", "g17", "g144", "g145", "p171", "g550", "l1000", "h144", "ra")
CASES_DOC = {
    "g16": "4x4 pose grid, SE d=3, k=64: exactly one 64-column panel",
    "g17": "17-pose path, SE d=3, k=68: one column block past a panel",
    "g144": "12x12 grid, SE d=3, k=576: 9 panels, one past the 8-block super-panel",
    "g145": "12x12 grid plus one pose, SE d=3, k=580: a 4-column last panel behind a super-panel",
    "p171": "3x57 planar grid strip, SE d=2, k=513: block 3, odd sizes",
    "g550": "22x25 grid, SE d=3, k=2200: the dense/sparse crossover, ldm = 2304",
    "l1000": "10x10x10 lattice, SE d=3, k=4000: sparse by size, a root separator of 100 poses",
    "h144": "12x12 grid plus 2 hub poses joined to every pose, SE d=3, k=584: hubs",
    "ra": "10x10 grid, l = 9 unit spheres, b = 5 landmarks, RA ordering, k=414: scalar unknowns, block 1",
}
_SEED = {c: 7919 + 104729 * i for i, c in enumerate(CASES)}


class Case:
    def __init__(self, cid):
        self.id = cid
        d, n, edges, nhub, l, b = _spec(cid)
        self.d, self.n, self.l, self.b, self.nhub = d, n, l, b, nhub
        self.k = k = (d + 1) * n + l + b
        self.block = 1 if (l or b) else d + 1   # the block the library gives the layout (RA ordering: scalar)
        rng = np.random.default_rng(_SEED[cid])
        # vertices -> their unknowns
        if l or b:  # RA ordering: rotations | unit spheres | translations | landmarks
            unk = [list(range(d * i, d * i + d)) + [d * n + l + i] for i in range(n)]
            unk += [[d * n + j] for j in range(l)] + [[d * n + l + n + j] for j in range(b)]
            edges = list(edges)
            for j in range(l):  # a range between two poses, or between a pose and a landmark
                p0 = int(rng.integers(n))
                other = n + l + int(rng.integers(b)) if j % 2 else int(rng.integers(n))
                edges += [(p0, n + j), (other, n + j)]
            for j in range(b):  # a landmark seen from three poses
                edges += [(int(p), n + l + j) for p in rng.choice(n, 3, replace=False)]
        else:
            unk = [list(range((d + 1) * i, (d + 1) * (i + 1))) for i in range(n)]
        self.pose_unknowns = unk[:n]
        self.edges = sorted({(min(u, v), max(u, v)) for u, v in edges if u != v})
        # L's order: a seeded permutation of the unknowns, the hubs' unknowns last
        hub = np.array([u for v in unk[n - nhub:n] for u in v], dtype=np.int64) if nhub else np.zeros(0, np.int64)
        rest = np.setdiff1d(np.arange(k), hub)
        self.order = np.concatenate([rng.permutation(rest), rng.permutation(hub)])   # position -> unknown
        self.pos = np.empty(k, np.int64)                                              # unknown -> position
        self.pos[self.order] = np.arange(k)
        self.hub_positions = np.arange(k - hub.size, k)
        # strict lower pattern of L: full inside a vertex, slot to slot across a pose-pose edge
        us, vs = [], []
        for v in unk:
            a = np.array(v)
            uu, vv = np.meshgrid(a, a, indexing="ij")
            m = uu < vv
            us.append(uu[m]); vs.append(vv[m])
        for p, q in self.edges:
            if len(unk[p]) == len(unk[q]):   # two poses: slot c of one to slot c of the other (see the module's text)
                uu, vv = np.array(unk[p]), np.array(unk[q])
            else:                            # a scalar unknown (unit sphere, landmark) to every unknown of a pose
                uu, vv = np.meshgrid(np.array(unk[p]), np.array(unk[q]), indexing="ij")
            us.append(uu.ravel()); vs.append(vv.ravel())
        pu, pv = self.pos[np.concatenate(us)], self.pos[np.concatenate(vs)]
        key = np.unique(np.minimum(pu, pv) * k + np.maximum(pu, pv))     # column-major order of the entries of L
        cols, rows = key // k, key % k
        # 4 L_ij: +-1 seven times in eight, +-2 otherwise; the hubs' rows, 146 entries long, hold +-1 only
        vals = np.where(rng.random(key.size) < 0.125, 2, 1) * np.where(rng.random(key.size) < 0.5, -1, 1)
        vals = np.where(rows >= k - hub.size, np.sign(vals), vals).astype(np.int64)
        self.L4 = sp.csc_matrix((np.concatenate([vals, np.full(k, 4, np.int64)]),
                                 (np.concatenate([rows, np.arange(k)]), np.concatenate([cols, np.arange(k)]))),
                                shape=(k, k), dtype=np.int64)            # 4 L
        self.L4.sort_indices()
        # A (scaled) = sum_p d_p (4 l_p)(4 l_p)^T, entry by entry on the pattern of |L| |L|^T in vertex numbering:
        # C[t, p] = contribution of column p to stored entry t
        ip, ix, dat = self.L4.indptr, self.L4.indices, self.L4.data
        tr, tc, tp, tv = [], [], [], []
        for p in range(k):
            r_ = self.order[ix[ip[p]:ip[p + 1]]]
            x = dat[ip[p]:ip[p + 1]]
            tr.append(np.repeat(r_, r_.size)); tc.append(np.tile(r_, r_.size))
            tv.append(np.outer(x, x).ravel()); tp.append(np.full(r_.size * r_.size, p, np.int64))
        tr, tc, tp, tv = (np.concatenate(z) for z in (tr, tc, tp, tv))
        uniq, inv = np.unique(tr * k + tc, return_inverse=True)
        self.rp = np.concatenate([[0], np.cumsum(np.bincount(uniq // k, minlength=k))]).astype(np.int32)
        self.ci = (uniq % k).astype(np.int32)
        self.C = sp.csc_matrix((tv, (inv.ravel(), tp)), shape=(uniq.size, k), dtype=np.int64)
        self.C.sum_duplicates()
        self.absC = abs(self.C).tocsr()
        self.W = rng.integers(-3, 4, size=(k, W_COLS)).astype(np.int64)
        self._e = {a: np.random.default_rng(_SEED[cid] + 31 * a + 1).integers(-a, a + 1, size=k) for a in SCALES}
        if nhub:  # the library must see the hubs as hubs: amd_like_order's rule on the block graph of A's pattern
            blk = self.d + 1
            rows = np.repeat(np.arange(k), np.diff(self.rp)) // blk
            bk = np.unique(rows * (k // blk) + self.ci // blk)
            bk = bk[bk // (k // blk) != bk % (k // blk)]
            deg = np.bincount(bk // (k // blk), minlength=k // blk)
            self.hub_threshold = max(48, int(8.0 * deg.mean()))
            assert deg[n - nhub:].min() > self.hub_threshold and deg[:n - nhub].max() <= self.hub_threshold

    # ---- D ------------------------------------------------------------------------------------------------------------
    def exponents(self, a, p=None):
        """e_i of D = diag(2^e_i) in L's order; with p, the positive twin of the sign sweep: e_p = -a"""
        e = self._e[a].copy()
        if p is not None:
            e[p] = -a
        return e

    def logdet(self, a, p=None):
        return LN2 * float(self.exponents(a, p).sum())

    def _dscaled(self, a, p, negative):
        ds = np.left_shift(np.int64(1), (self.exponents(a, p) + a).astype(np.int64))   # 2^a D, integers 1 .. 2^(2a)
        if negative:
            assert p is not None
            ds[p] = -1                                                                   # D_pp = -2^-a exactly
        return ds

    # ---- A ------------------------------------------------------------------------------------------------------------
    def values(self, a, p=None, negative=False):
        """A's stored entries (float64, exact) on the case's pattern; p: D_pp -> +2^-a, or -2^-a with negative"""
        ds = self._dscaled(a, p, negative)
        assert (self.absC @ np.abs(ds)).max() < 2 ** 53        # |L| D |L|^T, scaled: every partial sum is an integer
        return (self.C @ ds).astype(np.float64) / float(16 << a)

    def scipy(self, a, p=None, negative=False):
        """explicit zeros stay in .data (csr_matrix from the three arrays drops nothing)"""
        return sp.csr_matrix((self.values(a, p, negative), self.ci, self.rp), shape=(self.k, self.k))

    def csr(self, a, p=None, negative=False):
        import dcora_amd as da
        return da.Csr(self.k, self.rp, self.ci, self.values(a, p, negative))

    def sha256(self, a):
        h = hashlib.sha256()
        for z in (self.rp, self.ci, self.values(a)):
            h.update(np.ascontiguousarray(z).tobytes())
        return h.hexdigest()

    def WV(self, a, r, p=None, negative=False):
        """W (k x r, integers in [-3, 3]) and V = A W, exact; checked against a long double product"""
        W = self.W[:, :r]
        ds = self._dscaled(a, p, negative)
        Ai = sp.csr_matrix(((self.C @ ds), self.ci, self.rp), shape=(self.k, self.k))
        assert (abs(Ai) @ np.abs(W)).max() < 2 ** 53
        V = (Ai @ W).astype(np.float64) / float(16 << a)
        v = self.values(a, p, negative)
        rows = np.repeat(np.arange(self.k), np.diff(self.rp))
        Vl = np.zeros((self.k, r), np.longdouble)
        np.add.at(Vl, rows, v.astype(np.longdouble)[:, None] * W[self.ci].astype(np.longdouble))
        assert np.array_equal(Vl, V.astype(np.longdouble))
        return W.astype(np.float64), V

    # ---- sign sweeps --------------------------------------------------------------------------------------------------
    def sweep_positions(self):
        """positions of L's order whose pivot the sign sweeps replace (None: the case has no sweep)"""
        k = self.k
        if self.id in ("g16", "g17", "ra"):
            return np.arange(k)
        if self.id in ("g144", "g145", "h144"):
            p = [q for q in range(k) if q % 64 in (0, 15, 16, 63)] + list(range(k - 8, k)) + list(self.hub_positions)
            return np.unique(np.array(p))
        if self.id == "l1000":
            # the library does not expose which 100 poses it takes as the root separator; a middle plane of the lattice
            # is one: 3 unknowns from each of the planes x = 4 and x = 5, the first and last position, 8 spread between
            mid = [self.pos[self.pose_unknowns[100 * x + 10 * y + z][c]] for x, y, z, c in
                   ((4, 0, 0, 0), (4, 5, 5, 3), (4, 9, 9, 1), (5, 0, 9, 2), (5, 4, 4, 0), (5, 9, 0, 3))]
            p = np.unique(np.array([0, k - 1] + [int(q) for q in mid]))
            more = [q for q in np.linspace(1, k - 2, 40).astype(int) if q not in p][:16 - p.size]
            return np.unique(np.concatenate([p, np.array(more)]))
        return None

    def create_positions(self):
        """first, middle, last (a hub unknown where the case has hubs) and, with hubs, the first hub unknown"""
        p = [0, self.k // 2 - 1 if self.nhub else self.k // 2, self.k - 1]
        if self.nhub:
            p.insert(2, int(self.hub_positions[0]))
        return p

    def L(self):
        """L (float64, exact) in L's order"""
        return (self.L4.astype(np.float64) / 4.0).tocsc()


_cases = {}


def case(cid):
    if cid not in _cases:
        _cases[cid] = Case(cid)
    return _cases[cid]


# ---- the recorded reference numbers and the bounds made of them -------------------------------------------------------------
_ref = {}


def ref():
    """{(case id, a): dict(kappa, lapack_solve, lapack_logdet, sum_abs_log, oracle_solve, sha256)}"""
    if not _ref:
        with np.load(REF_PATH) as z:
            ids, scales = [str(s) for s in z["case"]], z["a"]
            for i, (c, a) in enumerate(zip(ids, scales)):
                _ref[(c, int(a))] = dict(kappa=float(z["kappa"][i]), lapack_solve=float(z["lapack_solve"][i]),
                                         lapack_logdet=float(z["lapack_logdet"][i]),
                                         sum_abs_log=float(z["sum_abs_log"][i]), oracle_solve=float(z["oracle_solve"][i]),
                                         sha256=str(z["sha256"][i]))
    return _ref


def base_solve(cid, a):
    """max(LAPACK's recorded solve error on the case, eps kappa_2(A)): a device error may be 8 times this"""
    r_ = ref()[(cid, a)]
    return max(r_["lapack_solve"], EPS * r_["kappa"])


def tol_solve(cid, a):
    return 8.0 * base_solve(cid, a)


def base_logdet(cid, a):
    r_ = ref()[(cid, a)]
    return max(r_["lapack_logdet"], EPS * r_["kappa"])


def tol_logdet(cid, a, p=None):
    """absolute: 8 max(LAPACK's log-det error, eps kappa) + n eps sum |2 ln l_ii|, the last term the worst case of a
    sum taken in free order (the device adds the 2 ln l_ii with atomicAdd).  With a swapped pivot the recorded sum is
    corrected by that pivot's exact change, which bounds the change of the sum of |ln| of the pivots of any order only
    loosely; the term stays a small part of the bound."""
    c = case(cid)
    r_ = ref()[(cid, a)]
    s = r_["sum_abs_log"] + (LN2 * (a + abs(int(c._e[a][p]))) if p is not None else 0.0)
    return 8.0 * base_logdet(cid, a) + c.k * EPS * s
