"""Simultaneous updates in the range-aided session (dcora_ra_rbcd_iterate_set / _agent_colours / _set_acceleration: the
agents that fire together in the asynchronous mode, ref src/Agent.cpp:650-678, as synchronous ticks), with the statements
tests/test_parallel_rbcd.py makes for pose graphs: a tick over one colour equals the same agents updated one after the
other, a tick over adjacent agents equals each agent's solve from the common snapshot -- also against the oracle's local
solver driven from numpy -- the ground truth of the noiseless fixtures stays put, and bad calls are refused in the
argument checks.  tiers.pyfg's agent graph is K4, so the input on which two agents do run at once is its ring variant
(tests/ra_ring.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import common
from ra_ring import write_ring_variant
from test_raslam import ra_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


def _sets(col, nc):
    return [np.flatnonzero(col == c).astype(np.int32) for c in range(nc)]


def _lifted_start(orc, ra, r, seed, noise):  # as tests/test_ra_session.py
    rng = np.random.default_rng(seed)
    lift = np.linalg.qr(rng.standard_normal((r, ra.d)))[0]
    M = lift @ ra.gt + noise * rng.standard_normal((r, ra.k))
    return orc.project_to_manifold(r, ra.d, ra.n, M, l=ra.l, b=ra.b)


@pytest.mark.parametrize("which", ["ring", "tiers"])
def test_ra_coloured_tick_equals_one_after_the_other(env, tmp_path, which):
    """Measured on an MI355X: ring variant and tiers, all three sweeps: the two sessions' iterates and costs are bitwise
    equal (max |X_par - X_seq| = 0, |c2p - c2s| = 0) -- the same kernels run on both sides."""
    da, orc = env
    ra = da.RADataset(write_ring_variant(tmp_path)[0] if which == "ring" else ra_path("tiers"))
    r = 3
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    par = da.RaRbcdSession(ra, r, acceleration=False)
    seq = da.RaRbcdSession(ra, r, acceleration=False)
    par.set_X(X0)
    seq.set_X(X0)
    col, nc = par.colours()
    hcol, hnc = ra.colours()
    assert col.tolist() == hcol.tolist() and nc == hnc  # the host rule and the session's rule are one rule
    sets = _sets(col, nc)
    if which == "ring":
        assert col.tolist() == [0, 1, 0, 1]
        assert max(len(S) for S in sets) >= 2  # something does run concurrently
    else:
        assert col.tolist() == [0, 1, 2, 3]  # every set a singleton: a tick is iterate of that agent
    costs = []
    for sweep in range(3):
        for S in sets:
            par.iterate_set(S)
            for a in S:
                c2s = seq.iterate(int(a))[0]
        c2p = par.evaluate()[0]
        costs.append(c2p)
        dX = np.abs(par.get_X() - seq.get_X()).max()
        print("%s sweep %d: 2f par %.17g seq %.17g |dc| %.3g max|dX| %.3g" % (which, sweep, c2p, c2s, abs(c2p - c2s), dX))
        assert abs(c2p - c2s) <= 1e-12 * abs(c2s)
        assert dX < 1e-11
    # RTR accepts only descent steps; a sweep in which every step is rejected is possible on this conditioning
    assert costs[1] <= costs[0] and costs[2] <= costs[1] and costs[2] < costs[0], costs


def _oracle_snapshot_tick(da, orc, ra, X0, r, agents, opt):
    """numpy driver over the oracle's local solver (the style of oracle/flows.py oracle_ra_rbcd_loop): the agents of the
    set read one snapshot"""
    X = X0.copy()
    for rb in agents:
        dims3, own, Qaa, Cc = ra.agent_blocks(rb)
        reg = da.precond_regularization(Qaa)  # the session computes the same per-agent regularisation
        G = (Cc.tocsr() @ X0.T).T
        P = orc.Problem(r, ra.d, dims3[0], orc.CSR.from_scipy(sp.csr_matrix(Qaa.to_scipy())), G=G, reg=reg,
                        l=dims3[1], b=dims3[2])
        X[:, own] = P.optimize(X0[:, own], **opt)[0]
    return X


def test_ra_simultaneous_adjacent_agents_read_one_snapshot(env):
    da, orc = env
    ra = da.RADataset(ra_path("range_aided_slam_test_3d"))
    r = 4
    X0 = _lifted_start(orc, ra, r, 5, 0.05)
    opt = dict(RTR_iterations=3, RTR_tCG_iterations=50, gradnorm_tol=1e-2)
    prm = da.ROptParameters(**opt)
    s = da.RaRbcdSession(ra, r, acceleration=False, params=prm)
    one = da.RaRbcdSession(ra, r, acceleration=False, params=prm)
    s.set_X(X0)
    with pytest.raises(da.DcoraError, match="share measurements"):
        s.iterate_set([0, 1])
    assert np.array_equal(s.get_X(), X0)
    s.iterate_set([0, 1], allow_adjacent=True)
    Xs = s.get_X()
    for a, rb in enumerate(ra.robots):
        one.set_X(X0)
        one.iterate(a)
        own = ra.agent_columns[rb][1]
        assert np.abs(one.get_X()[:, own] - Xs[:, own]).max() < 1e-11
    Xo = _oracle_snapshot_tick(da, orc, ra, X0, r, ra.robots, opt)
    central = orc.Problem(r, ra.d, ra.n, orc.CSR.from_scipy(ra.Q.to_scipy()), reg=-1, l=ra.l, b=ra.b)
    fo, fp = central.f(Xo), central.f(Xs)
    print("2f oracle %.17g product %.17g rel(X) %.3g" % (2 * fo, 2 * fp, common.rel(Xs, Xo)))
    assert abs(fp - fo) <= 1e-7 * abs(fo)
    assert common.rel(Xs, Xo) < 1e-6


@pytest.mark.parametrize("name", ["range_aided_slam_test_2d", "range_aided_slam_test_3d"])
def test_ra_tick_keeps_the_ground_truth(env, name):
    """ref tests/testAgent.cpp:290-456 with the example's local parameters (RTR 200 x 200, tol 1e-4), both agents at once"""
    da, orc = env
    ra = da.RADataset(ra_path(name))
    prm = da.ROptParameters(RTR_iterations=200, RTR_tCG_iterations=200, gradnorm_tol=1e-4)
    s = da.RaRbcdSession(ra, ra.d, acceleration=False, params=prm)
    s.set_X(ra.gt)
    s.iterate_set([0, 1], allow_adjacent=True)
    assert np.abs(s.get_X() - ra.gt).max() < 1e-9  # OPTIMIZATION_TOL, ref tests/testAgent.cpp:20


def test_ra_ticks_refuse_acceleration_and_bad_sets(env):
    da, orc = env
    ra = da.RADataset(ra_path("range_aided_slam_test_3d"))
    X0 = _lifted_start(orc, ra, 4, 5, 0.05)
    acc = da.RaRbcdSession(ra, 4, acceleration=True)
    acc.set_X(X0)
    with pytest.raises(da.DcoraError, match="acceleration off"):
        acc.iterate_set([0])
    with pytest.raises(da.DcoraError, match="acceleration off"):
        acc.run_coloured(max_sweeps=1, rgrad_tol=0.0)
    acc.set_acceleration(False)
    for bad in ([0, 0], [acc.R], [-1]):
        with pytest.raises(da.DcoraError, match="out of range or twice"):
            acc.iterate_set(bad)
    c0 = acc.evaluate()[0]
    acc.iterate_set([0])
    acc.iterate_set([1])
    assert acc.evaluate()[0] < c0
    acc.set_acceleration(True)
    with pytest.raises(da.DcoraError, match="acceleration off"):
        acc.iterate_set([0])
    acc.iterate(0)  # the accelerated loop goes on from V = Y = X
