"""row_qf and row_polar (dcora_amd/csrc/pose_group.h), the 8-lanes-per-pose twins of qf_blk and polar_blk that the SE layout
runs at r <= 8, and the Nesterov bookkeeping of both kernel forms, block by block against 50-digit factors: through
k_g_retract (dcora_debug_group_retract) and k_g_nesterov / k_nesterov (dcora_debug_nesterov, form 1 / form 0).

Blocks: the groups of tests/golden/block_factors.npz with r <= 8 (at |A^T A - I|_F <= 2e-9 or >= 0.99) and the
near-orthonormal family of block_factors_near.npz (1e-6 .. 0.4, both sides of row_polar's Gram radius 0.25), whose
entries are multiples of 2^-40 so that the kernels' own combinations -- X + V, X + V / 2, x / 2 + v / 2,
v + (Xloc - y) / 2 -- are the stored block bit for bit.

The acceptance rule is that of test_block_factors_gpu.py: per group, the largest block error is at most
8 x max(oracle_err_g, eps cond_g), and |Y^T Y - I|_F at most 8 x the file's oracle_orth.  The cases with alpha = 0.37,
gamma = 0.61 add, per block, the forward error of forming the combination in float64 times 1 / sigma_min
(block_factors.NDGroup.forward).  Everything a kernel only copies or combines exactly is compared bitwise.

Largest device error / max(oracle_err_g, eps cond_g) observed on an MI355X, per entry point (bound: 8):
  k_g_retract (row_qf)        block_factors.npz 1.58 (d=2 r=2 kappa=1)   near 1.37 (d=3 r=6 delta=0.001), alpha = 1 and 1/2
  k_g_nesterov mode 1         block_factors.npz 1.00 (d=2 r=2 kappa=1)   near 1.99 (d=2 r=5 delta=0.1), alpha = 0 and 1/2
  k_g_nesterov modes 0, 2, inner_Yloc, cur = 0 / 1 / -1    1.35 (d=2 r=4 delta=0.1)
  k_nesterov (form 0) modes 0, 1, 2    1.01 (d=3 r=9 kappa=1), 1.03 (d=2 r=16 kappa=1);  at (3, 5) 1.36 (delta=0.03)
  form 0 - form 1 at (3, 5): at most 0.11 x the sum of the two bounds
  alpha = 0.37 / gamma = 0.61: device error at most 0.13 x (8 x rule + forward term)
  orthogonality: at most 0.47 (row_qf), 0.91 (row_polar), 1.03 (polar_blk) x oracle_orth (bound: 8)
  partial sums of k_g_retract: |sum - dot| at most 2e-3 x gamma_N sum |terms|

What fails when a value in the kernels is changed (one change at a time, the library rebuilt, this module run on an
MI355X; nothing else in it fails):
  the Newton-Schulz stop at e2 < 1e-8       test_group_polar_blocks_* (all 9; near groups at 27 .. 1.4e5 x the rule,
                                            errors of 1e-14 .. 8e-11), form 1 of test_nesterov_mode_0 and
                                            test_nesterov_modes_1_2_3, test_group_nesterov_inner_yloc, *_cur_names,
                                            *_non_dyadic_coefficients, test_both_forms_agree_block_by_block
  kPolarGramRadius = 1.0                    test_group_polar_blocks_* (all 9: kappa >= 1e2 at d = 2 and the clustered
                                            group at d = 3 sit at |G - I|_F <= 1 and come out with errors of 0.1 .. 1),
                                            test_both_forms_agree_block_by_block
  settled = __all(...) over the wave        test_a_pose_does_not_depend_on_its_neighbours[k_g_nesterov],
                                            test_second_grid_trip[k_g_nesterov]
  row_qf without its second pass            test_group_retraction_blocks_* (all 9)
  the `restart & 2` test inverted           form 1 of test_nesterov_mode_0, test_group_nesterov_inner_yloc
"""
import ctypes as C

import numpy as np
import pytest

import block_factors as bf

pytestmark = pytest.mark.gpu

EPS = bf.EPS
SENT = -7.25           # fill of what a launch must leave alone (finite: 0 * SENT is 0)
MAX_PARTIALS = 1024    # kMaxPartials (dcora_amd/csrc/kernels.h): cap of the group kernels' grid
POSES_PER_BLOCK = 32   # kPosesPerBlock: 256 threads, 8 lanes per pose
STATE = ("X", "V", "Y", "XPrev", "Yloc")


# ---- the two entry points ------------------------------------------------------------------------------------------------
def _opt(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def group_retract(r, d, n, X, V, alpha, grad=None, HV=None):
    """(out as r x (d+1) n, the partial buffer as handed back, the number of slot pairs written)"""
    from dcora_amd import capi
    out, partials, npart = np.full(r * (d + 1) * n, SENT), np.full(2 * MAX_PARTIALS, SENT), C.c_int(-1)
    g, h = (None if a is None else capi.F(a) for a in (grad, HV))
    capi.check(capi.lib().dcora_debug_group_retract(r, d, n, capi.F(X), capi.F(V), alpha, _opt(g), _opt(h), out, partials,
                                                    C.byref(npart)))
    return capi.unF(out, r, (d + 1) * n), partials, npart.value


def nesterov(form, r, d, n, mode, st, restart=0, skip=(0, 0), alpha=0.0, gamma=0.0, Xloc0=None, Xloc1=None, cur=-1,
             inner=None):
    """one launch on copies of st's five matrices; the five after it (and "inner" when given)"""
    from dcora_amd import capi
    k = (d + 1) * n
    flat = [capi.F(st[key]) for key in STATE]
    nan = np.full((r, k), np.nan)
    loc = [capi.F(nan if a is None else a) for a in (Xloc0, Xloc1)]
    fi = None if inner is None else capi.F(inner)
    capi.check(capi.lib().dcora_debug_nesterov(form, r, d, n, mode, restart, skip[0], skip[1], alpha, gamma, *flat, *loc,
                                               cur, _opt(fi)))
    out = {key: capi.unF(f, r, k) for key, f in zip(STATE, flat)}
    if inner is not None:
        out["inner"] = capi.unF(fi, r, inner.shape[1])
    return out


# ---- blocks, states, the rule ----------------------------------------------------------------------------------------------
class Blocks:
    """the blocks of some groups, concatenated, optionally tiled (idx: fixture block of every pose)"""
    def __init__(self, groups, orth_bound, n=None, shift=0):
        self.groups, self.orth_bound = groups, orth_bound
        self.A = np.concatenate([g.inp for g in groups])
        self.gid = np.concatenate([[i] * len(g.inp) for i, g in enumerate(groups)])
        self.idx = (np.arange(len(self.A) if n is None else n) + shift) % len(self.A)

    def inp(self):
        return self.A[self.idx]

    def rows(self, out, what):
        ref = np.concatenate([g.ref(what) for g in self.groups])[self.idx]
        err = bf.block_err(out, ref)
        return [(g.name, err[self.gid[self.idx] == i].max(), g.tol(what)) for i, g in enumerate(self.groups)]


def _families(d, r):
    fx, nfx = bf.load(), bf.load_near()
    return (Blocks(bf.pq_groups(fx, d, r), float(fx["oracle_orth"])),
            Blocks(bf.near_groups(nfx, d, r), float(nfx["oracle_orth"])))


def _near(d, r, n, shift=0):
    nfx = bf.load_near()
    return Blocks(bf.near_groups(nfx, d, r), float(nfx["oracle_orth"]), n, shift)


def _check_groups(entry, rows, orth, orth_bound):
    """rows: (group name, device error, max(oracle error, eps cond)); prints every ratio, asserts each <= 8"""
    lines = ["%-22s %-34s device %.3e  oracle-or-eps-cond %.3e  ratio %.2f" % (entry, n, e, t, e / t) for n, e, t in rows]
    worst = max(rows, key=lambda x: x[1] / x[2])
    print("\n".join(lines))
    print("RATIO %s max %.2f (%s); orthogonality %.2f x oracle_orth" % (entry, worst[1] / worst[2], worst[0],
                                                                         orth / orth_bound))
    bad = [ln for ln, (n, e, t) in zip(lines, rows) if not e <= 8 * t]
    assert not bad, "device error above 8 x max(oracle_err_g, eps cond_g):\n" + "\n".join(bad)
    assert orth <= 8 * orth_bound, (entry, orth)


def _check(entry, B, M, what="polar"):
    """the rotation blocks of the SE matrix M against B's references"""
    Y = bf.se_blocks(M, B.groups[0].d)
    _check_groups(entry, B.rows(Y, what), bf.orth_err(Y).max(), B.orth_bound)


def _check_both(entry, fams, M, what):
    """one launch over the old groups followed by the near groups: each family against its own file"""
    d, o = fams[0].groups[0].d, 0
    for fam, tag in zip(fams, ("", " near")):
        nb = len(fam.idx)
        _check(entry + tag, fam, M[:, o * (d + 1):(o + nb) * (d + 1)], what)
        o += nb


def _trans(M, d):
    return M[:, d::d + 1]


def _E(n, r, d):
    return bf.qf_point(n, r, d)


def _T(seed, r, n, scale=10.0):
    return scale * np.random.default_rng(seed).standard_normal((r, n))


def _fill(r, d, n):
    return np.full((r, (d + 1) * n), SENT)


def _state(r, d, n, **given):
    return {key: given.get(key, _fill(r, d, n)) for key in STATE}


def _same(a, b):
    """bitwise (array_equal would let -0.0 pass for 0.0)"""
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _pose_cols(d, lo, hi):
    return slice(lo * (d + 1), hi * (d + 1))


# ---- a. row_qf through k_g_retract -----------------------------------------------------------------------------------------
def _gamma(N):
    u = EPS / 2
    return N * u / (1 - N * u)


@pytest.mark.parametrize("d,r", bf.NEAR_DR)
def test_group_retraction_blocks_match_the_high_precision_factor(built, d, r):
    fams = _families(d, r)
    A = np.concatenate([f.inp() for f in fams])
    n = len(A)
    rng = np.random.default_rng(300 + 10 * r + d)
    X = bf.se_matrix(_E(n, r, d), _T(1, r, n))
    V = bf.se_matrix(A - _E(n, r, d), _T(2, r, n, 1.0))
    assert _same(bf.se_blocks(X + V, d), A)
    grad, HV = rng.standard_normal(X.shape), rng.standard_normal(X.shape)
    out, partials, npart = group_retract(r, d, n, X, V, 1.0, grad, HV)
    assert _same(_trans(out, d), _trans(X + V, d))
    _check_both("k_g_retract", fams, out, "qf")
    # the two partial sums, slot by slot
    assert npart == -(-n // POSES_PER_BLOCK) and (partials[2 * npart:] == SENT).all()
    N = r * (d + 1) * n + 2
    for j, W in enumerate((grad, HV)):
        s = 0.0
        for p in partials[j:2 * npart:2]:
            s += p
        terms = V.astype(np.longdouble) * W.astype(np.longdouble)
        gap, room = abs(float(s - terms.sum())), _gamma(N) * float(np.abs(terms).sum())
        print("k_g_retract partial %d: |sum - dot| %.2e  gamma_N sum|terms| %.2e" % (j, gap, room))
        assert gap <= room
    # alpha = 1 / 2 on the near groups, and no partial buffer: nothing comes back
    near = fams[1]
    A, n = near.inp(), len(near.idx)
    X = bf.se_matrix(_E(n, r, d), _T(3, r, n))
    V = bf.se_matrix(2 * A - 2 * _E(n, r, d), _T(4, r, n, 1.0))
    out, partials, npart = group_retract(r, d, n, X, V, 0.5)
    assert npart == 0 and (partials == SENT).all()
    assert _same(_trans(out, d), _trans(X + 0.5 * V, d))
    _check("k_g_retract alpha=.5", near, out, "qf")


# ---- b. row_polar through k_g_nesterov, mode 1 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d,r", bf.NEAR_DR)
def test_group_polar_blocks_match_the_high_precision_factor(built, d, r):
    fams = _families(d, r)
    A = np.concatenate([f.inp() for f in fams])
    n = len(A)
    # alpha = 0: y = P(x)
    x = bf.se_matrix(A, _T(5, r, n))
    v = np.random.default_rng(310 + 10 * r + d).standard_normal(x.shape)
    o = nesterov(1, r, d, n, 1, _state(r, d, n, X=x, V=v), alpha=0.0)
    assert _same(o["Y"], o["Yloc"]) and _same(o["XPrev"], x) and _same(o["X"], x) and _same(o["V"], v)
    assert _same(_trans(o["Y"], d), _trans(x, d))
    _check_both("k_g_nesterov mode 1", fams, o["Y"], "polar")
    # alpha = 1 / 2, x = E, v = 2 A - E: the combination is A
    near = fams[1]
    A, n = near.inp(), len(near.idx)
    x = bf.se_matrix(_E(n, r, d), _T(6, r, n))
    v = bf.se_matrix(2 * A - _E(n, r, d), _T(7, r, n))
    o = nesterov(1, r, d, n, 1, _state(r, d, n, X=x, V=v), alpha=0.5)
    assert _same(o["Y"], o["Yloc"]) and _same(o["XPrev"], x) and _same(o["X"], x) and _same(o["V"], v)
    assert _same(_trans(o["Y"], d), 0.5 * _trans(x, d) + 0.5 * _trans(v, d))
    _check("k_g_nesterov mode 1 a=.5", near, o["Y"], "polar")


# ---- c. / d. the bookkeeping of every mode, in both forms ----------------------------------------------------------------------
N_BOOK = 45  # not a multiple of 8: the last wave of the group form has dead groups
SKIP = (13, 29)


def _book_blocks(form, d, r):
    """form 1: the near family, tiled; form 0 (r > 8): the groups of block_factors.npz.  (blocks of x, blocks of v)"""
    if form == 1:
        return _near(d, r, N_BOOK), _near(d, r, N_BOOK, shift=1)
    fx = bf.load()
    return tuple(Blocks(bf.pq_groups(fx, d, r), float(fx["oracle_orth"]), N_BOOK, s) for s in (0, 1))


def _mode2_inputs(form, B, r, d):
    """(gamma, v, y, Xloc) with v + gamma (Xloc - y) == A bit for bit: through halves of the quantised blocks in form
    1, through fl(E + fl(A - E)) == A of block_factors.npz in form 0"""
    n, E = len(B.idx), _E(len(B.idx), r, d)
    v, y = bf.se_matrix(E, _T(11, r, n)), bf.se_matrix(E, _T(12, r, n))
    if form == 1:
        return 0.5, v, y, bf.se_matrix(2 * B.inp() - E, _T(13, r, n))
    return 1.0, v, y, bf.se_matrix(B.inp(), _T(13, r, n))


BOOK = [(1, 2, 4), (1, 3, 5), (1, 3, 8), (0, 3, 9), (0, 2, 16)]


@pytest.mark.parametrize("form,d,r", BOOK)
def test_nesterov_mode_0(built, form, d, r):
    Bx, Bv = _book_blocks(form, d, r)
    n, tag = N_BOOK, "form %d mode 0" % form
    x, v = bf.se_matrix(Bx.inp(), _T(8, r, n)), bf.se_matrix(Bv.inp(), _T(9, r, n))
    st = _state(r, d, n, X=x, V=v)
    # plain: X = Y = P(x), V = P(v), XPrev = x
    o = nesterov(form, r, d, n, 0, st, alpha=0.0)
    assert _same(o["X"], o["Y"]) and _same(o["XPrev"], x) and _same(o["Yloc"], st["Yloc"])
    assert _same(_trans(o["X"], d), _trans(x, d)) and _same(_trans(o["V"], d), _trans(v, d))
    _check(tag + " Y", Bx, o["Y"])
    _check(tag + " V", Bv, o["V"])
    if form == 1:  # bit 2 (form 0 is handed restart & 1): V is known to be feasible and stays as it is
        o2 = nesterov(form, r, d, n, 0, st, restart=2, alpha=0.0)
        assert _same(o2["V"], v)
        for key in ("X", "Y", "XPrev", "Yloc"):
            assert _same(o2[key], o[key]), key
    # bit 1, the restart: V = Y = x, X and XPrev = x
    for restart in (1, 3) if form == 1 else (1,):
        o3 = nesterov(form, r, d, n, 0, st, restart=restart, alpha=0.0)
        for key in ("X", "V", "Y", "XPrev"):
            assert _same(o3[key], x), (restart, key)
        assert _same(o3["Yloc"], st["Yloc"])


@pytest.mark.parametrize("form,d,r", BOOK)
def test_nesterov_modes_1_2_3(built, form, d, r):
    B, _ = _book_blocks(form, d, r)
    n, tag = N_BOOK, "form %d" % form
    # mode 1
    x = bf.se_matrix(B.inp(), _T(8, r, n))
    v = np.random.default_rng(320).standard_normal(x.shape)
    st = _state(r, d, n, X=x, V=v)
    o = nesterov(form, r, d, n, 1, st, alpha=0.0)
    assert _same(o["Y"], o["Yloc"]) and _same(o["XPrev"], x) and _same(o["X"], x) and _same(o["V"], v)
    assert _same(_trans(o["Y"], d), _trans(x, d))
    _check(tag + " mode 1", B, o["Y"])
    # mode 2: X = Xloc, V = P(v + gamma (Xloc - y)) = P(A)
    gamma, v, y, xloc = _mode2_inputs(form, B, r, d)
    st = _state(r, d, n, V=v, Y=y)
    o = nesterov(form, r, d, n, 2, st, gamma=gamma, Xloc0=xloc)
    assert _same(o["X"], xloc) and _same(o["Y"], y) and _same(o["XPrev"], st["XPrev"]) and _same(o["Yloc"], st["Yloc"])
    assert _same(_trans(o["V"], d), _trans(v, d) + gamma * (_trans(xloc, d) - _trans(y, d)))
    _check(tag + " mode 2", B, o["V"])
    # mode 3: X = V = Y = Xloc
    st = _state(r, d, n)
    o = nesterov(form, r, d, n, 3, st, Xloc0=xloc)
    for key in ("X", "V", "Y"):
        assert _same(o[key], xloc), key
    assert _same(o["XPrev"], st["XPrev"]) and _same(o["Yloc"], st["Yloc"])


@pytest.mark.parametrize("form,d,r", BOOK)
def test_nesterov_skip_range(built, form, d, r):
    """the poses of [13, 29) keep their fill in all five arrays, in every mode; the others end as without the range"""
    B, Bv = _book_blocks(form, d, r)
    n = N_BOOK
    sk = _pose_cols(d, *SKIP)
    gamma, v2, y2, xloc = _mode2_inputs(form, B, r, d)
    x, v = bf.se_matrix(B.inp(), _T(8, r, n)), bf.se_matrix(Bv.inp(), _T(9, r, n))
    cases = [(0, dict(X=x, V=v), dict(alpha=0.0)), (0, dict(X=x, V=v), dict(alpha=0.0, restart=1)),
             (1, dict(X=x, V=v), dict(alpha=0.0)), (2, dict(V=v2, Y=y2), dict(gamma=gamma, Xloc0=xloc)),
             (3, dict(), dict(Xloc0=xloc))]
    for mode, given, kw in cases:
        full = nesterov(form, r, d, n, mode, _state(r, d, n, **given), **kw)
        st = _state(r, d, n, **{k: a.copy() for k, a in given.items()})
        for a in st.values():
            a[:, sk] = SENT
        o = nesterov(form, r, d, n, mode, st, skip=SKIP, **kw)
        for key in STATE:
            assert (o[key][:, sk] == SENT).all(), (mode, kw.get("restart", 0), key)
            keep = np.ones(o[key].shape[1], bool)
            keep[sk] = False
            assert _same(o[key][:, keep], full[key][:, keep]), (mode, key)


@pytest.mark.parametrize("d,r", [(2, 4), (3, 5), (3, 8)])
def test_group_nesterov_inner_yloc(built, d, r):
    """mode 0 with inner_Yloc: the skipped poses run mode 1 into Y and inner_Yloc[pose - skip_lo], with
    y = P(x / 2 + v / 2) = P(A); their X, V and Yloc stay.  The others run mode 0."""
    B = _near(d, r, N_BOOK)
    n, (lo, hi) = N_BOOK, SKIP
    sk = _pose_cols(d, lo, hi)
    E = _E(n, r, d)
    x, v = bf.se_matrix(E, _T(14, r, n)), bf.se_matrix(2 * B.inp() - E, _T(15, r, n))
    st = _state(r, d, n, X=x, V=v)
    inner = np.full((r, (d + 1) * (hi - lo)), SENT)
    o = nesterov(1, r, d, n, 0, st, restart=2, skip=SKIP, alpha=0.5, inner=inner)
    assert _same(o["XPrev"], x) and _same(o["V"], v) and _same(o["Yloc"], st["Yloc"])
    assert _same(o["inner"], o["Y"][:, sk]) and _same(o["X"][:, sk], x[:, sk])
    keep = np.ones(x.shape[1], bool)
    keep[sk] = False
    assert _same(o["X"][:, keep], o["Y"][:, keep])
    assert _same(_trans(o["Y"], d), 0.5 * _trans(x, d) + 0.5 * _trans(v, d))
    _check("k_g_nesterov inner_Yloc", B, o["Y"])
    # without the buffer the same launch leaves the range alone
    o2 = nesterov(1, r, d, n, 0, st, restart=2, skip=SKIP, alpha=0.5)
    for key in STATE:
        assert _same(o2[key][:, sk], st[key][:, sk]) and _same(o2[key][:, keep], o[key][:, keep]), key


@pytest.mark.parametrize("d,r", [(2, 4), (3, 5), (3, 8)])
def test_group_nesterov_reads_the_buffer_cur_names(built, d, r):
    B = _near(d, r, N_BOOK)
    n = N_BOOK
    gamma, v, y, xloc = _mode2_inputs(1, B, r, d)
    for cur in (0, 1, -1):
        loc = {"Xloc1" if cur == 1 else "Xloc0": xloc}  # the other buffer is NaN
        o = nesterov(1, r, d, n, 3, _state(r, d, n), cur=cur, **loc)
        for key in ("X", "V", "Y"):
            assert _same(o[key], xloc), (cur, key)
        o = nesterov(1, r, d, n, 2, _state(r, d, n, V=v, Y=y), gamma=gamma, cur=cur, **loc)
        assert _same(o["X"], xloc), cur
        _check("k_g_nesterov mode 2 cur=%d" % cur, B, o["V"])


@pytest.mark.parametrize("d,r", bf.ND_DR)
@pytest.mark.parametrize("mode", [1, 2])
def test_group_nesterov_non_dyadic_coefficients(built, mode, d, r):
    """alpha = 0.37, gamma = 0.61, inputs that are not quantised: against the factor of the exact combination, with the
    forward error of forming it in float64 added per block"""
    nfx = bf.load_near()
    (g,) = bf.nd_groups(nfx, d, r, mode)
    n = N_BOOK
    idx = np.arange(n) % len(g.ref)
    a, b, c = (bf.se_matrix(M[idx], _T(16 + i, r, n)) for i, M in enumerate((g.a, g.b, g.c)))
    if mode == 1:
        o = nesterov(1, r, d, n, 1, _state(r, d, n, X=a, V=b), alpha=bf.ND_ALPHA)
        out = o["Y"]
        assert _same(o["Y"], o["Yloc"]) and _same(o["XPrev"], a)
        # (not bitwise: the products round, and the compiler may contract one of them into the sum)
        p, q = (1.0 - bf.ND_ALPHA) * _trans(a, d), bf.ND_ALPHA * _trans(b, d)
        assert (np.abs(_trans(out, d) - (p + q)) <= EPS * (np.abs(p) + np.abs(q))).all()
    else:
        o = nesterov(1, r, d, n, 2, _state(r, d, n, V=a, Y=c), gamma=bf.ND_GAMMA, Xloc0=b)
        out = o["V"]
        assert _same(o["X"], b)
    Y = bf.se_blocks(out, d)
    err, bound = bf.block_err(Y, g.ref[idx]), 8 * g.tol() + g.forward()[idx]
    orth = bf.orth_err(Y).max()
    worst = int(np.argmax(err / bound))
    for i in range(len(g.ref)):
        print("%-32s block %2d |G - I| %.3f  device %.3e  8 x rule + forward %.3e (forward %.3e)" % (
            g.name, i, g.dist[i], err[i], bound[i], g.forward()[i]))
    print("RATIO k_g_nesterov non-dyadic %s: max device / bound %.2f (block %d); orthogonality %.2f x oracle_orth" % (
        g.name, err[worst] / bound[worst], worst, orth / float(nfx["nd_oracle_orth"])))
    assert (err <= bound).all() and orth <= 8 * float(nfx["nd_oracle_orth"])


def test_both_forms_agree_block_by_block(built):
    """k_nesterov (polar_blk) and k_g_nesterov (row_polar) on the same (3, 5) blocks: within the sum of their bounds"""
    d, r = 3, 5
    for fam in _families(d, r):
        n = len(fam.idx)
        x = bf.se_matrix(fam.inp(), _T(5, r, n))
        v = np.random.default_rng(330).standard_normal(x.shape)
        Y = [bf.se_blocks(nesterov(form, r, d, n, 1, _state(r, d, n, X=x, V=v), alpha=0.0)["Y"], d) for form in (0, 1)]
        for f in (0, 1):
            _check_groups("form %d mode 1 (3,5)" % f, fam.rows(Y[f], "polar"), bf.orth_err(Y[f]).max(), fam.orth_bound)
        gap = bf.block_err(Y[0], Y[1])
        for i, g in enumerate(fam.groups):
            m = gap[fam.gid == i].max()
            print("form 0 - form 1  %-34s %.3e  (2 x 8 x tol %.3e)" % (g.name, m, 16 * g.tol("polar")))
            assert m <= 16 * g.tol("polar"), g.name


# ---- e. a pose's bits do not depend on its neighbours -----------------------------------------------------------------------
def _mixed_set():
    """(3, 5): the 32 near blocks (Gram branch, and Jacobi from 0.255 on), kappa=1e2 tiled to 16 and kappa=1e12 tiled to
    19 (Jacobi, few and many sweeps): 67 = 8 * 8 + 3 blocks, and the kind of each"""
    d, r = 3, 5
    near = np.concatenate([g.inp for g in bf.near_groups(bf.load_near(), d, r)])
    few, many = (g.inp for g in bf.pq_groups(bf.load(), d, r) if g.name.endswith(("kappa=100", "kappa=1e+12")))
    A = np.concatenate([near, few[np.arange(16) % 4], many[np.arange(19) % 4]])
    kind = np.array([0] * 32 + [1] * 16 + [2] * 19)
    assert len(A) == 67 and len(near) == 32 and len(few) == len(many) == 4
    return d, r, A, kind


def _arrangements(kind):
    n = len(kind)
    pools = [list(np.flatnonzero(kind == k)) for k in range(3)]
    inter = []
    for _ in range(n // 8):  # 4 near, 2 few-sweep, 2 many-sweep blocks in every full wave
        inter += [pools[0].pop(0) for _ in range(4)] + [pools[1].pop(0) for _ in range(2)] + [pools[2].pop(0) for _ in
                                                                                              range(2)]
    inter += pools[0] + pools[1] + pools[2]
    inter = np.array(inter)
    assert sorted(inter) == list(range(n))
    for w in range(n // 8):
        assert set(kind[inter[8 * w:8 * w + 8]]) == {0, 1, 2}
    return {"stored": np.arange(n), "reversed": np.arange(n)[::-1].copy(), "interleaved": inter}


def _run_polar(r, d, A, T):
    n = len(A)
    x = bf.se_matrix(A, T)
    return nesterov(1, r, d, n, 1, _state(r, d, n, X=x, V=np.ones(x.shape)), alpha=0.0)["Y"]


def _run_qf(r, d, A, T):
    n = len(A)
    return group_retract(r, d, n, bf.se_matrix(_E(n, r, d), T), bf.se_matrix(A - _E(n, r, d)), 1.0)[0]


@pytest.mark.parametrize("run", [_run_polar, _run_qf], ids=["k_g_nesterov", "k_g_retract"])
def test_a_pose_does_not_depend_on_its_neighbours(built, run):
    d, r, A, kind = _mixed_set()
    n = len(A)
    assert n % 8 == 3  # the last wave has dead groups
    T = _T(17, r, n)
    outs = {}
    for name, perm in _arrangements(kind).items():
        M = run(r, d, A[perm], T[:, perm])
        blocks = M.reshape(r, n, d + 1).transpose(1, 0, 2)  # pose by pose, translation included
        assert not (blocks == SENT).any()
        outs[name] = np.empty_like(blocks)
        outs[name][perm] = blocks
    for name in ("reversed", "interleaved"):
        diff = [i for i in range(n) if not _same(outs[name][i], outs["stored"][i])]
        assert not diff, "%s: blocks %s (kinds %s) differ from the stored order" % (name, diff, kind[diff])


# ---- f. the second trip of the capped grid -----------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [_run_polar, _run_qf], ids=["k_g_nesterov", "k_g_retract"])
def test_second_grid_trip(built, run):
    d, r, A, _ = _mixed_set()
    n = POSES_PER_BLOCK * MAX_PARTIALS + 40
    assert n > POSES_PER_BLOCK * MAX_PARTIALS  # group_grid caps the grid: the last 40 poses are a second trip
    idx = np.arange(n) % len(A)
    T = np.zeros((r, n)) + np.arange(1.0, r + 1)[:, None]
    M = run(r, d, A[idx], T)
    blocks = M.reshape(r, n, d + 1).transpose(1, 0, 2)
    assert not (blocks == SENT).any()
    assert _same(blocks, blocks[idx]), "a copy of a block differs from its first copy"
