"""Regenerates tests/golden/block_factors.npz: per-block polar, QF and SO(d) factors at 50 digits (mpmath), rounded to
float64, with what the CPU oracle achieves on the same inputs.  Run on the CPU:  python tests/golden/make_block_factors.py
It also writes tests/golden/block_factors_near.npz (the last section below); with --near it writes only that file.

The three references share nothing with oracle/ or dcora_amd/csrc (those are Hestenes-Jacobi / two-pass MGS in IEEE
double; these are mpmath's Golub-Kahan SVD and a Gram-Schmidt at mp.dps = 50):
  polar : U V^T of the thin SVD of the r x d block
  QF    : the Q factor of the thin QR with positive diag(R)
  SO(d) : U diag(1, ..., 1, sign(det U det V)) V^T of the SVD of the d x d block

Families (4 blocks per group unless stated):
  pq_*  polar and QF share their inputs, A = U diag(sigma) V^T with random orthonormal U (r x d), V (d x d), for
        d in {2, 3}, r in {d, 4, 5, 8, 9, 16} -- an exact fit and the first rank past it for each register width of the
        kernels -- and (d, r) = (3, 6), the rank of the range-aided case.  sigma = geomspace(1, 1/kappa, d) for kappa in
        {1, 1e2, ..., 1e12}; one clustered group (1, 1 - 1e-9[, 1e-6]); kappa = 1e4 scaled by 1e-6 and by 1e+6.
        The retraction forms X + V itself, so every block A satisfies fl(X + fl(A - X)) == A for X = eye(r, d): a test
        passes V = A - X and the kernel's float64 sum X + V is A bit for bit.
  so_*  d x d blocks with sigma_max = 1: (sigma_min) for d = 2, (0.7, sigma_min) for d = 3, sigma_min in {0.5, 1e-3,
        1e-6, 1e-9}; a close pair ending in (1, 0.9); each with det > 0 and with det < 0 (sigma_min negated); as plain
        d x d blocks (r = d) and as r = 5 blocks Y_i under a random d-frame R0 (so_R0_<d>) with R0^T Y_i as above, the
        reference then being computed from R0^T Y_i formed in mpmath.  Exact rank d - 1 blocks (r = d, groups of 24):
        diag(1,0), diag(0,1), [[0,1],[0,0]] and diag(1,.5,0) with three column permutations of it, each multiplied from
        the left by signed permutation matrices of both determinants.

block_factors_near.npz, for the 8-lanes-per-pose kernels (row_polar, row_qf of dcora_amd/csrc/pose_group.h):
  nr_*  near-orthonormal blocks at the (d, r) above with r <= 8: A = U diag(sqrt(1 + x_i)) V^T, x of mixed signs with
        |x|_2 = delta, so |A^T A - I|_F = delta, for delta in {1e-6, 1e-3, 0.03, 0.1, 0.2, 0.245, 0.255, 0.4}: inside
        row_polar's Gram radius 0.25 (two to five Newton-Schulz steps), 2 % clear of it on both sides, and well past it.
        Every entry is rounded to a multiple of 2^-40 BEFORE the references are computed: A - E, 2 A - E and
        E + (2 A - 2 E) / 2 with E = eye(r, d) are then exact in float64, with or without FMA contraction, so a test can
        hand a kernel inputs whose combination is the stored block bit for bit.  Polar and QF references, cond and the
        oracle's errors per group as for pq_*.
  nd_*  inputs that are NOT quantised, for alpha = 0.37 and gamma = 0.61: (a, b) = (x, v) of a mode-1 Nesterov step and
        (a, b, c) = (v, Xloc, y) of a mode-2 step, 15 blocks per (d, r) in {(2, 4), (3, 5), (3, 8)}, with the polar factor
        of fl(1 - alpha) a + alpha b resp. a + gamma (b - c), the combination being formed exactly (mpmath) from the
        float64 inputs; sigma_min and |G - I|_F of the combination per block.  The oracle's error of these groups is
        measured on the combination rounded to float64 against that block's own factor.

Left out, because the factor is not unique there: rank-deficient blocks for polar and QF; SO(d) blocks with det < 0 and
sigma_{d-1} = sigma_d; SO(d) blocks of rank <= d - 2.

Per group: *_cond (polar / QF: sigma_max / sigma_min of the stored block; SO(d): 1 / (sigma_{d-1} + sigma_d) for det > 0,
1 / (sigma_{d-1} - sigma_d) for det < 0, nominal), *_oracle_err (max over the group of |oracle - reference|_F, from
orc.project_to_manifold, orc.retract and orc.align_lifted_trajectory_to_frame), and oracle_orth, the largest
|Y^T Y - I|_F of any oracle output in the file.  The inputs and references are bit-reproducible (fixed seeds, mpmath);
the oracle columns depend on the compiler that built the oracle.
"""
import itertools
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):  # the repository (oracle/) and tests/
    if _p not in sys.path:
        sys.path.insert(0, _p)

import block_factors as bf  # noqa: E402
from block_factors import PQ_DR, PQ_KINDS, SO_DR, SO_TAILS  # noqa: E402

SEED = 20261019
NB = 4  # blocks per group
mp.mp.dps = 50


# ---- mpmath helpers ---------------------------------------------------------------------------------------------------
def _mp(a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in a])


def _np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)], dtype=np.float64)


def gram_schmidt(M):
    """Q of the thin QR of M with positive diag(R), at the working precision"""
    Q = mp.matrix(M.rows, M.cols)
    for j in range(M.cols):
        v = M[:, j].copy()
        for _ in range(2):
            for c in range(j):
                s = mp.fsum(Q[i, c] * v[i] for i in range(M.rows))
                for i in range(M.rows):
                    v[i] -= s * Q[i, c]
        nn = mp.sqrt(mp.fsum(v[i] * v[i] for i in range(M.rows)))
        for i in range(M.rows):
            Q[i, j] = v[i] / nn
    return Q


def ref_polar(A):
    U, _, Vh = mp.svd_r(_mp(A), full_matrices=False, compute_uv=True)
    return _np(U * Vh)


def ref_qf(A):
    return _np(gram_schmidt(_mp(A)))


def ref_so_mp(M):
    U, _, Vh = mp.svd_r(M, full_matrices=True, compute_uv=True)  # singular values in descending order
    d = M.rows
    D = mp.eye(d)
    D[d - 1, d - 1] = mp.sign(mp.det(U) * mp.det(Vh))
    return _np(U * D * Vh)


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def _frame(rng, r, d, proper=False):
    """random orthonormal r x d frame at the working precision (det +1 when square and proper)"""
    Q = gram_schmidt(_mp(rng.standard_normal((r, d))))
    if proper and mp.det(Q) < 0:
        Q[:, d - 1] = -Q[:, d - 1]
    return Q


# ---- polar / QF family --------------------------------------------------------------------------------------------------
def pq_sigma(d, kappa):
    if kappa is None:
        return [1.0, 1.0 - 1e-9] if d == 2 else [1.0, 1.0 - 1e-9, 1e-6]
    return [float(s) for s in np.geomspace(1.0, 1.0 / kappa, d)]


def make_pq_group(d, r, gi):
    """inputs (NB, r, d), polar and QF references (NB, r, d), cond of the stored blocks"""
    _, kappa, scale = PQ_KINDS[gi]
    rng = _rng(1, d, r, gi)
    sig = pq_sigma(d, kappa)
    X = bf.qf_point(1, r, d)[0]
    A_in, P_ref, Q_ref, cond = [], [], [], 0.0
    for _ in range(NB):
        U, V = _frame(rng, r, d), _frame(rng, d, d)
        A = _np(U * mp.diag([mp.mpf(s) for s in sig]) * V.T * mp.mpf(scale))
        for _ in range(8):  # the float64 sum X + (A - X) reproduces A
            A1 = X + (A - X)
            if np.array_equal(A1, A):
                break
            A = A1
        assert np.array_equal(X + (A - X), A)
        s = mp.svd_r(_mp(A), compute_uv=False)
        cond = max(cond, float(s[0] / s[d - 1]))
        A_in.append(A)
        P_ref.append(ref_polar(A))
        Q_ref.append(ref_qf(A))
    return np.array(A_in), np.array(P_ref), np.array(Q_ref), cond


# ---- SO(d) family ---------------------------------------------------------------------------------------------------------
def so_sigma(d, tail):
    if tail == "close":
        return [1.0, 0.9] if d == 2 else [1.0, 1.0, 0.9]
    return [1.0, tail] if d == 2 else [1.0, 0.7, tail]


def so_frame(d):
    """the d-frame R0 (5 x d, float64) of the r = 5 sets"""
    return _np(_frame(_rng(3, d), 5, d))


def make_so_group(d, r, sign, ti):
    """inputs (NB, r, d) -- the d x d block itself for r = d, Y_i with R0^T Y_i = block for r = 5 --, references
    (NB, d, d), nominal cond"""
    sig = so_sigma(d, SO_TAILS[ti])
    rng = _rng(2, d, r, 0 if sign > 0 else 1, ti)
    cond = 1.0 / (sig[d - 2] + sign * sig[d - 1])
    S = mp.diag([mp.mpf(s) for s in sig[:-1]] + [mp.mpf(sign * sig[-1])])
    R0 = so_frame(d) if r != d else None
    ins, refs = [], []
    for _ in range(NB):
        U, V = _frame(rng, d, d, proper=True), _frame(rng, d, d, proper=True)
        M = U * S * V.T
        if r == d:
            Y = _np(M)
            Mq = _mp(Y)
        else:
            # Y = R0 M + (I - R0 R0^T) W: the part outside the frame does not reach R0^T Y
            R0m = _mp(R0)
            W = _mp(rng.standard_normal((r, d)))
            Y = _np(R0m * M + W - R0m * (R0m.T * W))
            Mq = R0m.T * _mp(Y)
        assert mp.sign(mp.det(Mq)) == sign
        ins.append(Y)
        refs.append(ref_so_mp(Mq))
    return np.array(ins), np.array(refs), cond


def signed_permutations(d):
    out = []
    for perm in itertools.permutations(range(d)):
        for sg in itertools.product((1.0, -1.0), repeat=d):
            S = np.zeros((d, d))
            for i, p in enumerate(perm):
                S[i, p] = sg[i]
            out.append(S)
    return out


def make_so_rankdef(d):
    """exact rank d - 1 blocks, 24 per d, and their unique nearest rotations; cond = 1 / sigma_{d-1}"""
    if d == 2:
        bases = [np.diag([1.0, 0.0]), np.diag([0.0, 1.0]), np.array([[0.0, 1.0], [0.0, 0.0]])]
        perms = signed_permutations(2)  # all 8
        cond = 1.0
    else:
        B = np.diag([1.0, 0.5, 0.0])
        bases = [B, B[:, [2, 0, 1]], B[:, [1, 2, 0]], B[:, [1, 0, 2]]]
        allp = signed_permutations(3)
        pos = [S for S in allp if np.linalg.det(S) > 0]
        neg = [S for S in allp if np.linalg.det(S) < 0]
        perms = [pos[0], pos[7], pos[13], neg[2], neg[11], neg[20]]
        cond = 2.0
    ins = [S @ B for B in bases for S in perms]
    refs = [ref_so_mp(_mp(M)) for M in ins]
    return np.array(ins), np.array(refs), cond


# ---- the near-orthonormal family (block_factors_near.npz) -------------------------------------------------------------------
def make_near_group(d, r, di):
    """A = U diag(sqrt(1 + x_i)) V^T with |x|_2 = delta and mixed signs, so |A^T A - I|_F = delta; every entry rounded to
    a multiple of 2^-40; references and cond of the rounded blocks"""
    delta = bf.NEAR_DELTAS[di]
    rng = _rng(4, d, r, di)
    A_in, P_ref, Q_ref, cond = [], [], [], 0.0
    for _ in range(NB):
        U, V = _frame(rng, r, d), _frame(rng, d, d)
        x = rng.uniform(0.3, 1.0, d) * (-1.0) ** (np.arange(d) + rng.integers(2))
        x *= delta / np.linalg.norm(x)
        A = _np(U * mp.diag([mp.sqrt(1 + mp.mpf(float(t))) for t in x]) * V.T)
        A = np.round(A / bf.NEAR_QUANTUM) * bf.NEAR_QUANTUM
        s = mp.svd_r(_mp(A), compute_uv=False)
        cond = max(cond, float(s[0] / s[d - 1]))
        A_in.append(A)
        P_ref.append(ref_polar(A))
        Q_ref.append(ref_qf(A))
    return np.array(A_in), np.array(P_ref), np.array(Q_ref), cond


ND_NB = 15  # blocks per non-dyadic group


def make_nd_group(d, r, mode):
    """unquantised inputs of a mode-1 (y = P(c0 x + alpha v), c0 = fl(1 - alpha)) or a mode-2 (v = P(v + gamma (Xloc - y)))
    launch with alpha = 0.37, gamma = 0.61, the 50-digit polar factor of the combination formed exactly from them, its
    sigma_min and |G - I|_F per block, its cond over the group, and the combination rounded to float64 (for the oracle)"""
    rng = _rng(5, d, r, mode)
    al, ga = mp.mpf(bf.ND_ALPHA), mp.mpf(bf.ND_GAMMA)
    c0 = mp.mpf(1.0 - bf.ND_ALPHA)
    a_, b_, c_, ref, smin, dist, comb, cond = [], [], [], [], [], [], [], 0.0
    for i in range(ND_NB):
        spread = bf.ND_SPREADS[i % len(bf.ND_SPREADS)]
        x = np.linalg.qr(rng.standard_normal((r, d)))[0]
        w = x + spread * rng.standard_normal((r, d)) / np.sqrt(r)
        if mode == 1:  # a = x, b = v
            a, b, c = x, w, np.zeros((r, d))
            M = c0 * _mp(a) + al * _mp(b)
        else:  # a = v, b = Xloc, c = y
            a, b, c = x, w, np.linalg.qr(x + 0.1 * rng.standard_normal((r, d)))[0]
            M = _mp(a) + ga * (_mp(b) - _mp(c))
        U, s, Vh = mp.svd_r(M, full_matrices=False, compute_uv=True)
        cond = max(cond, float(s[0] / s[d - 1]))
        G = M.T * M - mp.eye(d)
        for k, v in zip((a_, b_, c_, ref, smin, dist, comb),
                        (a, b, c, _np(U * Vh), float(s[d - 1]), float(mp.sqrt(mp.fsum(g * g for g in G))), _np(M))):
            k.append(v)
    return tuple(np.array(v) for v in (a_, b_, c_, ref, smin, dist, comb)) + (cond,)


def main_near():
    out = {}
    orth = 0.0
    fl = lambda v: v.transpose(0, 2, 1).reshape(-1)  # column-major blocks, one after another
    meta = {k: [] for k in ("d", "r", "delta", "off", "cnt", "cond", "polar_oracle_err", "qf_oracle_err")}
    data = {k: [] for k in ("in", "polar", "qf")}
    off = 0
    for d, r in bf.NEAR_DR:
        for di, delta in enumerate(bf.NEAR_DELTAS):
            A, P, Q, cond = make_near_group(d, r, di)
            Po, Qo = bf.oracle_polar(A), bf.oracle_qf(A)
            orth = max(orth, bf.orth_err(Po).max(), bf.orth_err(Qo).max())
            for k, v in zip(meta, (d, r, delta, off, NB, cond, bf.block_err(Po, P).max(), bf.block_err(Qo, Q).max())):
                meta[k].append(v)
            for k, v in zip(data, (A, P, Q)):
                data[k].append(fl(v))
            off += NB * r * d
            print("near d=%d r=%d delta=%-6g cond %.3f  oracle polar %.2e  qf %.2e" % (d, r, delta, cond, meta[
                "polar_oracle_err"][-1], meta["qf_oracle_err"][-1]), flush=True)
    for k, v in meta.items():
        out["nr_" + k] = np.array(v, dtype=np.int32 if k in ("d", "r", "off", "cnt") else np.float64)
    for k, v in data.items():
        out["nr_" + k] = np.concatenate(v)
    meta = {k: [] for k in ("d", "r", "mode", "off", "cnt", "cond", "oracle_err")}
    data = {k: [] for k in ("a", "b", "c", "ref", "smin", "dist")}
    off, nd_orth = 0, 0.0
    for d, r in bf.ND_DR:
        for mode in (1, 2):
            a, b, c, ref, smin, dist, comb, cond = make_nd_group(d, r, mode)
            # the oracle cannot take the exact combination: its error is measured on the combination rounded to float64
            Po = bf.oracle_polar(comb)
            nd_orth = max(nd_orth, bf.orth_err(Po).max())
            oerr = bf.block_err(Po, np.array([ref_polar(M) for M in comb])).max()
            for k, v in zip(meta, (d, r, mode, off, ND_NB, cond, oerr)):
                meta[k].append(v)
            for k, v in zip(data, (fl(a), fl(b), fl(c), fl(ref), smin, dist)):
                data[k].append(v)
            off += ND_NB * r * d
            print("nd d=%d r=%d mode %d cond %.3f  oracle %.2e  |G - I| %.3f .. %.3f" % (d, r, mode, cond, oerr,
                                                                                        dist.min(), dist.max()), flush=True)
    for k, v in meta.items():
        out["nd_" + k] = np.array(v, dtype=np.float64 if k in ("cond", "oracle_err") else np.int32)
    for k, v in data.items():
        out["nd_" + k] = np.concatenate(v)
    out["oracle_orth"], out["nd_oracle_orth"] = np.array(orth), np.array(nd_orth)
    np.savez_compressed(bf.NEAR_PATH, **out)
    print("wrote %s: %d bytes, oracle_orth %.2e (nr_*) %.2e (nd_*)" % (bf.NEAR_PATH, os.path.getsize(bf.NEAR_PATH), orth,
                                                                       nd_orth))


# ---- assembly --------------------------------------------------------------------------------------------------------------
def main():
    out = {}
    orth = 0.0
    # polar / QF
    meta = {k: [] for k in ("d", "r", "kind", "off", "cnt", "cond", "polar_oracle_err", "qf_oracle_err")}
    data = {k: [] for k in ("in", "polar", "qf")}
    off = 0
    for d, r in PQ_DR:
        for gi, (name, _, _) in enumerate(PQ_KINDS):
            A, P, Q, cond = make_pq_group(d, r, gi)
            Po, Qo = bf.oracle_polar(A), bf.oracle_qf(A)
            orth = max(orth, bf.orth_err(Po).max(), bf.orth_err(Qo).max())
            for k, v in zip(meta, (d, r, gi, off, NB, cond, bf.block_err(Po, P).max(), bf.block_err(Qo, Q).max())):
                meta[k].append(v)
            # column-major blocks, one after another
            for k, v in zip(data, (A, P, Q)):
                data[k].append(v.transpose(0, 2, 1).reshape(-1))
            off += NB * r * d
            print("pq d=%d r=%2d %-16s cond %.2e  oracle polar %.2e  qf %.2e" % (d, r, name, cond, meta[
                "polar_oracle_err"][-1], meta["qf_oracle_err"][-1]), flush=True)
    for k, v in meta.items():
        out["pq_" + k] = np.array(v, dtype=np.float64 if k in ("cond", "polar_oracle_err", "qf_oracle_err") else np.int32)
    for k, v in data.items():
        out["pq_" + k] = np.concatenate(v)
    # SO(d)
    meta = {k: [] for k in ("d", "r", "sign", "tail", "off_in", "off_ref", "cnt", "cond", "oracle_err")}
    data = {k: [] for k in ("in", "ref")}
    off_in = off_ref = 0

    def add(d, r, sign, tail, Y, R, cond):
        nonlocal off_in, off_ref, orth
        anchor = np.zeros((r, d + 1))
        anchor[:, :d] = np.eye(d) if r == d else so_frame(d)
        Ro = bf.oracle_so(Y, anchor)
        orth = max(orth, bf.orth_err(Ro).max())
        for k, v in zip(meta, (d, r, sign, tail, off_in, off_ref, len(Y), cond, bf.block_err(Ro, R).max())):
            meta[k].append(v)
        data["in"].append(Y.transpose(0, 2, 1).reshape(-1))
        data["ref"].append(R.transpose(0, 2, 1).reshape(-1))
        off_in += Y.size
        off_ref += R.size
        print("so d=%d r=%d sign %+d tail %2d cond %.2e  oracle %.2e" % (d, r, sign, tail, cond,
                                                                         meta["oracle_err"][-1]), flush=True)

    for d, r in SO_DR:
        for sign in (1, -1):
            for ti in range(len(SO_TAILS)):
                add(d, r, sign, ti, *make_so_group(d, r, sign, ti))
    for d in (2, 3):
        add(d, d, 0, -1, *make_so_rankdef(d))  # sign 0, tail -1: the exact rank d - 1 groups
    for k, v in meta.items():
        out["so_" + k] = np.array(v, dtype=np.float64 if k in ("cond", "oracle_err") else np.int32)
    for k, v in data.items():
        out["so_" + k] = np.concatenate(v)
    for d in (2, 3):
        out["so_R0_%d" % d] = so_frame(d)
    out["oracle_orth"] = np.array(orth)
    np.savez_compressed(bf.PATH, **out)
    print("wrote %s: %d bytes, oracle_orth %.2e" % (bf.PATH, os.path.getsize(bf.PATH), orth))


if __name__ == "__main__":
    if sys.argv[1:] not in ([], ["--near"]):
        sys.exit("usage: make_block_factors.py [--near]")
    if not sys.argv[1:]:
        main()
    main_near()
