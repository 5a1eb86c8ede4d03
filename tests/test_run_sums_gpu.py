"""The sums over the workgroup of the one-launch tCG run (k_tcg_run) and its phase A on rows of every length.

The run form takes its 16-lane row sums as a reduce-scatter over lane-swap instructions (wg_row_sums) where the launches
keep the four-step DPP butterfly; the tree -- logical lanes L ^ 1, L ^ 2, L ^ 4, L ^ 8, then the 16 row sums one after the
other -- is the same, so every partial and every total must agree BIT FOR BIT with the butterfly and with a numpy
emulation of the tree.  Phase A gathers up to 24 entries of a matrix row in one round trip and the rest in chunks: a
hand-made graph with a hub pose has rows on both sides of that threshold."""
import os

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

WG, ROWS = 256, 16  # threads of the workgroup; 16-lane rows in it


def _tree(x):
    """x: nv x 256 (wave-major logical lanes) -> the nv x 16 row sums and the nv totals of the kernels' tree"""
    t = x.reshape(x.shape[0], ROWS, 16)
    for _ in range(4):                       # logical lanes L ^ 1, then L ^ 2, L ^ 4, L ^ 8
        t = t[:, :, 0::2] + t[:, :, 1::2]
    part = t[:, :, 0]
    tot = np.zeros(x.shape[0])
    for w in range(ROWS):                    # the serial add over the 16 row sums, from +0
        tot = tot + part[:, w]
    return part, tot


def _left_to_right(x):
    t = x.reshape(x.shape[0], ROWS, 16)
    s = t[:, :, 0].copy()
    for i in range(1, 16):
        s = s + t[:, :, i]
    return s


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _sums_input(nv, zeros):
    rng = np.random.default_rng(1000 + nv + (7 if zeros else 0))
    x = rng.standard_normal((nv, WG)) * 10.0 ** rng.uniform(-8, 8, (nv, WG))
    if zeros:  # zeros of both signs mixed in; the first value is nothing but zeros, the second nothing but -0
        z = rng.uniform(size=x.shape)
        x[z < 0.15] = 0.0
        x[z > 0.85] = -0.0
        x[0] = np.where(rng.uniform(size=WG) < 0.5, 0.0, -0.0)
        x[1] = -0.0
    return x


@pytest.mark.parametrize("nv,zeros", [(33, False), (41, False), (49, False), (41, True)])
def test_workgroup_sums_are_bitwise_the_butterfly_and_the_tree(built, nv, zeros):
    """one workgroup, nv = 8 r + 1 values per lane (r = 4, 5, 6: an odd count, so the zero padding of both
    reduce-scatter levels is live): the reduce-scatter's nv x 16 row sums and nv totals equal the butterfly's and the
    emulated tree's bit for bit.  The input tells trees apart: a plain left-to-right sum of a row differs from the
    tree's in at least 40 % of the rows (50 such draws gave 52-60 %), so a wrong pairing order cannot pass."""
    from dcora_amd import capi
    x = _sums_input(nv, zeros)
    out = np.zeros(2 * nv * (ROWS + 1))
    assert capi.lib().dcora_debug_wg_sums(nv, np.ascontiguousarray(x.reshape(-1)), out) == 0
    out = out.reshape(2, nv * (ROWS + 1))
    got = {}
    for i, form in enumerate(("reduce-scatter", "butterfly")):
        got[form] = (out[i, :nv * ROWS].reshape(nv, ROWS), out[i, nv * ROWS:])
    part, tot = _tree(x)
    if not zeros:
        differ = np.mean(_bits(_left_to_right(x)) != _bits(part))
        print("left-to-right row sums that differ from the tree's: %.1f %%" % (100 * differ))
        assert differ >= 0.40, differ
    for form, (p, t) in got.items():
        bad = np.argwhere(_bits(p) != _bits(part))
        print(form, "row sums that differ from the emulated tree:", len(bad), "of", p.size)
        assert len(bad) == 0, (form, bad[:8].tolist())
        assert np.array_equal(_bits(t), _bits(tot)), (form, np.flatnonzero(_bits(t) != _bits(tot))[:8].tolist())
    assert np.array_equal(_bits(got["reduce-scatter"][0]), _bits(got["butterfly"][0]))
    assert np.array_equal(_bits(got["reduce-scatter"][1]), _bits(got["butterfly"][1]))


def _chain_graph(n, hub, seed):
    """SE(3) chain 0 - 1 - ... - n-1 (odometry) with noisy relative poses; hub >= 0: that pose also sees every other one"""
    import dcora_amd as da
    rng = np.random.default_rng(seed)

    def rot(scale):
        q, u = np.linalg.qr(np.eye(3) + scale * rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(u))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        return q

    Rg = [rot(0.8) for _ in range(n)]
    tg = [3.0 * rng.standard_normal(3) for _ in range(n)]
    edges = [(i, i + 1) for i in range(n - 1)]
    if hub >= 0:
        edges += [(hub, j) for j in range(n) if abs(j - hub) > 1]
    ids, vals = [], []
    for i, j in edges:
        Rij = Rg[i].T @ Rg[j] @ rot(0.05)
        tij = Rg[i].T @ (tg[j] - tg[i]) + 0.05 * rng.standard_normal(3)
        ids.append([0, i, 0, j])
        vals.append(np.r_[Rij.T.reshape(-1), tij, rng.uniform(50, 150), rng.uniform(5, 15), 1.0])
    return da.Dataset(3, n, np.array(ids), np.array(vals))


def _max_row_entries(Q):
    rp = np.asarray(Q.rp)
    return int(np.max(rp[1:] - rp[:-1]))


@pytest.mark.parametrize("hub", [True, False])
def test_phase_a_with_long_and_short_rows_is_bitwise_the_launches(built, hub):
    """9 poses (an odd count: the last workgroup holds one pose; five workgroups), r = 5: with a hub pose of degree 8 its
    matrix rows hold 36 entries, more than the 24 of the gather's first round trip; without it no row exceeds 12.  The
    one-launch run against the launches per iteration: X, the iteration counts, the exit reasons and fOpt bit for bit,
    with the default parameters and with long runs."""
    import dcora_amd as da
    n, r = 9, 5
    ds = _chain_graph(n, 4 if hub else -1, seed=11)
    Q = da.build_Q_pgo(ds)
    if hub:
        assert _max_row_entries(Q) > 24, _max_row_entries(Q)
    else:
        assert _max_row_entries(Q) <= 24, _max_row_entries(Q)
    rng = np.random.default_rng(5)
    k = (ds.d + 1) * n
    G = 0.3 * rng.standard_normal((r, k))
    X = da.manifold_project(r, ds.d, n, rng.uniform(-1, 1, (r, k)))
    for prm in (da.ROptParameters(), da.ROptParameters(RTR_tCG_iterations=60, gradnorm_tol=1e-9)):
        got = {}
        for form in ("launch", None):
            if form:
                os.environ["DCORA_SOLVER_TCG"] = form
            try:
                P = da.QuadraticProblem(r, ds.d, n, Q, G=G)
            finally:
                os.environ.pop("DCORA_SOLVER_TCG", None)
            want = "two launches" if form else "one launch per run"
            assert P.solver_info()["tcg"] == want, (hub, P.solver_info())
            opt = da.QuadraticOptimizer(P, prm)
            Xs = opt.optimize(X)
            got[form] = (Xs, opt.getOptResult())
            assert P.solver_info()["tcg"] == want   # (the run form did not give up)
            P.close()
        (Xa, ra), (Xb, rb) = got["launch"], got[None]
        for key in ("outer_iterations", "inner_iterations", "fOpt", "gradNormOpt", "fInit", "tCGStatus"):
            assert ra[key] == rb[key], (hub, key, ra[key], rb[key])
        assert ra["inner_iterations"] > 0
        assert np.array_equal(Xa, Xb), np.abs(Xa - Xb).max()
