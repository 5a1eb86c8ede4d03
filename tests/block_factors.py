"""reader of tests/golden/block_factors.npz (written by tests/golden/make_block_factors.py) and the helpers its tests and
its generator share: groups of single blocks with their 50-digit polar / QF / SO(d) factors, the SE-ordered matrices
that carry them through the entry points, per-block errors, and the oracle's entry points on the same blocks"""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_factors.npz")
EPS = np.finfo(np.float64).eps

# (d, r) of the polar / QF family: an exact fit and the first rank past it for each register width (4, 8, 16) of the
# thread-per-item kernels, and (3, 6), the rank of the range-aided case
PQ_DR = [(2, 2), (2, 4), (2, 5), (2, 8), (2, 9), (2, 16),
         (3, 3), (3, 4), (3, 5), (3, 6), (3, 8), (3, 9), (3, 16)]
KAPPAS = [1.0, 1e2, 1e4, 1e6, 1e8, 1e10, 1e12]
# kind -> (name, kappa or None for the clustered spectrum, scale of the whole block)
PQ_KINDS = [("kappa=%g" % k, k, 1.0) for k in KAPPAS] + [("clustered", None, 1.0), ("kappa=1e4 x 1e-6", 1e4, 1e-6),
                                                            ("kappa=1e4 x 1e+6", 1e4, 1e6)]
SO_TAILS = [0.5, 1e-3, 1e-6, 1e-9, "close"]
SO_DR = [(2, 2), (3, 3), (2, 5), (3, 5)]

# tests/golden/block_factors_near.npz: the near-orthonormal family of the 8-lanes-per-pose kernels (r <= 8).  A group is
# one (d, r) at one delta = |A^T A - I|_F, on both sides of row_polar's Gram radius 0.25; every entry is a multiple of
# NEAR_QUANTUM.  The nd_* groups carry the cases with non-dyadic coefficients (alpha = ND_ALPHA, gamma = ND_GAMMA).
NEAR_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_factors_near.npz")
NEAR_DR = [(d, r) for d, r in PQ_DR if r <= 8]
NEAR_DELTAS = [1e-6, 1e-3, 0.03, 0.1, 0.2, 0.245, 0.255, 0.4]
NEAR_QUANTUM = 2.0 ** -40
GRAM_RADIUS = 0.25  # kPolarGramRadius of dcora_amd/csrc/pose_group.h
ND_DR = [(2, 4), (3, 5), (3, 8)]
ND_ALPHA, ND_GAMMA = 0.37, 0.61
ND_SPREADS = [0.02, 0.1, 0.3, 0.6, 1.0]  # of v (mode 1) / of the step (mode 2) around x: both branches of row_polar

_cache = {}


def _load(key, path):
    if key not in _cache:
        with np.load(path) as z:
            _cache[key] = {k: z[k] for k in z.files}
    return _cache[key]


def load():
    return _load("fx", PATH)


def load_near():
    return _load("near", NEAR_PATH)


def _blocks(flat, off, cnt, rows, cols):
    """cnt column-major rows x cols blocks starting at off -> (cnt, rows, cols)"""
    return np.ascontiguousarray(flat[off:off + cnt * rows * cols].reshape(cnt, cols, rows).transpose(0, 2, 1))


class PQGroup:
    def __init__(self, fx, i):
        self.d, self.r, self.kind = int(fx["pq_d"][i]), int(fx["pq_r"][i]), int(fx["pq_kind"][i])
        self.name = "d=%d r=%d %s" % (self.d, self.r, PQ_KINDS[self.kind][0])
        self.cond = float(fx["pq_cond"][i])
        off, cnt = int(fx["pq_off"][i]), int(fx["pq_cnt"][i])
        self.inp, self.polar, self.qf = (_blocks(fx["pq_" + k], off, cnt, self.r, self.d) for k in ("in", "polar", "qf"))
        self.oracle_err = {"polar": float(fx["pq_polar_oracle_err"][i]), "qf": float(fx["pq_qf_oracle_err"][i])}

    def ref(self, what):
        return self.polar if what == "polar" else self.qf

    def tol(self, what):
        return max(self.oracle_err[what], EPS * self.cond)


class NearGroup(PQGroup):
    """a group of block_factors_near.npz: PQGroup's fields, with delta instead of kind"""
    def __init__(self, fx, i):
        self.d, self.r, self.delta = int(fx["nr_d"][i]), int(fx["nr_r"][i]), float(fx["nr_delta"][i])
        self.name = "d=%d r=%d delta=%g" % (self.d, self.r, self.delta)
        self.cond = float(fx["nr_cond"][i])
        off, cnt = int(fx["nr_off"][i]), int(fx["nr_cnt"][i])
        self.inp, self.polar, self.qf = (_blocks(fx["nr_" + k], off, cnt, self.r, self.d) for k in ("in", "polar", "qf"))
        self.oracle_err = {"polar": float(fx["nr_polar_oracle_err"][i]), "qf": float(fx["nr_qf_oracle_err"][i])}


class NDGroup:
    """mode 1: the polar factor of c0 a + alpha b (a = x, b = v, c0 = fl(1 - alpha)); mode 2: of a + gamma (b - c) (a = v,
    b = Xloc, c = y) -- the combination formed exactly from the float64 inputs.  smin: its smallest singular value and
    fwd: the norm sum of the forward-error term, per block"""
    def __init__(self, fx, i):
        self.d, self.r, self.mode = int(fx["nd_d"][i]), int(fx["nd_r"][i]), int(fx["nd_mode"][i])
        self.name = "d=%d r=%d mode %d non-dyadic" % (self.d, self.r, self.mode)
        self.cond, self.oracle_err = float(fx["nd_cond"][i]), float(fx["nd_oracle_err"][i])
        off, cnt = int(fx["nd_off"][i]), int(fx["nd_cnt"][i])
        self.a, self.b, self.c, self.ref = (_blocks(fx["nd_" + k], off, cnt, self.r, self.d) for k in ("a", "b", "c", "ref"))
        o = int(fx["nd_cnt"][:i].sum())  # smin, dist: one entry per block
        self.smin, self.dist = fx["nd_smin"][o:o + cnt], fx["nd_dist"][o:o + cnt]

    def tol(self):
        return max(self.oracle_err, EPS * self.cond)

    def forward(self):
        """per block: the error of forming the combination in float64 (u = 2^-53 per rounding, with or without FMA)
        times the polar factor's Lipschitz constant 1 / sigma_min.
        mode 1, fl(fl(c0 x) + fl(alpha v)): at most 2 u (|c0 x|_F + |alpha v|_F);
        mode 2, fl(v + fl(gamma fl(x - y))): at most u |v|_F + 3 u |gamma (x - y)|_F <= 3 u (|v|_F + |gamma (x - y)|_F)"""
        nrm = lambda M: np.sqrt((M ** 2).sum(axis=(1, 2)))
        u = EPS / 2
        if self.mode == 1:
            return 2 * u * (nrm((1.0 - ND_ALPHA) * self.a) + nrm(ND_ALPHA * self.b)) / self.smin
        return 3 * u * (nrm(self.a) + nrm(ND_GAMMA * (self.b - self.c))) / self.smin


def near_groups(fx, d=None, r=None):
    return [NearGroup(fx, i) for i in range(len(fx["nr_d"]))
            if (d is None or fx["nr_d"][i] == d) and (r is None or fx["nr_r"][i] == r)]


def nd_groups(fx, d, r, mode):
    return [NDGroup(fx, i) for i in range(len(fx["nd_d"]))
            if fx["nd_d"][i] == d and fx["nd_r"][i] == r and fx["nd_mode"][i] == mode]


class SOGroup:
    def __init__(self, fx, i):
        self.d, self.r = int(fx["so_d"][i]), int(fx["so_r"][i])
        self.sign, self.tail = int(fx["so_sign"][i]), int(fx["so_tail"][i])
        what = "rank d-1" if self.sign == 0 else "det%s0 tail=%s" % ("<>"[self.sign > 0], SO_TAILS[self.tail])
        self.name = "d=%d r=%d %s" % (self.d, self.r, what)
        self.cond, self.oracle_err = float(fx["so_cond"][i]), float(fx["so_oracle_err"][i])
        cnt = int(fx["so_cnt"][i])
        self.inp = _blocks(fx["so_in"], int(fx["so_off_in"][i]), cnt, self.r, self.d)
        self.ref = _blocks(fx["so_ref"], int(fx["so_off_ref"][i]), cnt, self.d, self.d)

    def tol(self):
        return max(self.oracle_err, EPS * self.cond)


def pq_groups(fx, d=None, r=None):
    return [PQGroup(fx, i) for i in range(len(fx["pq_d"]))
            if (d is None or fx["pq_d"][i] == d) and (r is None or fx["pq_r"][i] == r)]


def so_groups(fx, d=None, r=None):
    return [SOGroup(fx, i) for i in range(len(fx["so_d"]))
            if (d is None or fx["so_d"][i] == d) and (r is None or fx["so_r"][i] == r)]


def so_anchor(fx, d, r):
    """[I | 0] at r = d: the alignment then projects every block as given; [R0 | 0] for the r = 5 sets"""
    a = np.zeros((r, d + 1))
    a[:, :d] = np.eye(d) if r == d else fx["so_R0_%d" % d]
    return a


def so_blocks(fx, g):
    """the d x d blocks that get projected (for r = 5: R0^T Y_i in float64)"""
    return g.inp if g.r == g.d else np.einsum("ia,bic->bac", fx["so_R0_%d" % g.d], g.inp)


# ---- blocks <-> matrices in the SE ordering ----------------------------------------------------------------------------
def se_matrix(blocks, trans=None):
    """(nb, r, d) blocks in the rotation slots of an r x (d+1) nb matrix; trans (r, nb) in the translation columns"""
    nb, r, d = blocks.shape
    M = np.zeros((r, (d + 1) * nb))
    M.reshape(r, nb, d + 1)[:, :, :d] = blocks.transpose(1, 0, 2)
    if trans is not None:
        M[:, d::d + 1] = trans
    return M


def se_blocks(M, d):
    r, k = M.shape
    return np.ascontiguousarray(M.reshape(r, k // (d + 1), d + 1)[:, :, :d].transpose(1, 0, 2))


def block_err(a, b):
    """Frobenius norm of a - b block by block"""
    return np.sqrt(((np.asarray(a) - np.asarray(b)) ** 2).sum(axis=(1, 2)))


def orth_err(Y):
    return block_err(np.einsum("bia,bic->bac", Y, Y), np.eye(Y.shape[2])[None])


def pq_group_errors(groups, out, what):
    """(group, max block error of its slice of out) for out = the factors of the groups' blocks, concatenated"""
    o = 0
    for g in groups:
        n = len(g.inp)
        yield g, block_err(out[o:o + n], g.ref(what)).max()
        o += n


def so_group_errors(groups, out):
    o = 0
    for g in groups:
        n = len(g.inp)
        yield g, block_err(out[o:o + n], g.ref).max()
        o += n


# ---- the oracle's entry points on (nb, r, d) blocks -----------------------------------------------------------------------
def oracle_polar(A):
    from oracle import orc
    nb, r, d = A.shape
    return se_blocks(orc.project_to_manifold(r, d, nb, se_matrix(A)), d)


def qf_point(nb, r, d):
    """the on-manifold point of the retraction tests: every block eye(r, d); V = A - X then gives X + V == A bitwise"""
    return np.ascontiguousarray(np.broadcast_to(np.eye(r, d), (nb, r, d)))


def oracle_qf(A):
    from oracle import orc
    nb, r, d = A.shape
    X = se_matrix(qf_point(nb, r, d))
    return se_blocks(orc.retract(r, d, nb, X, se_matrix(A) - X), d)


def oracle_so(Y, anchor):
    from oracle import orc
    nb, r, d = Y.shape
    return se_blocks(orc.align_lifted_trajectory_to_frame(se_matrix(Y), anchor, d, nb, True), d)
