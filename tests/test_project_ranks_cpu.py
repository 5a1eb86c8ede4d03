"""The inputs of tests/test_project_ranks_gpu.py without a GPU: both rules of tests/session_project_inputs.py (eigen-gap
>= 0.25, least block singular value >= 0.5) for exactly the (d, r, n, nu) the rank tests use, and the numpy reference
inside the bounds those tests hold the device to -- so the reference alone stays inside every bound.  Also the index
rule the collective Gram sum rests on: the agents' blocks tile the columns, each column in exactly one block."""
import numpy as np
import pytest

import project_ranks_worker as prw
import session_project_inputs as spi

CASES = sorted({(d, r, n) for d, n, _, _ in prw.CHAIN_CASES for r in prw.CHAIN_RANKS})


@pytest.mark.parametrize("d,r,n", CASES)
def test_chain_points_are_well_conditioned(d, r, n):
    X = prw.chain_point(d, r, n)
    gap, smin = spi.eig_gap(X, d), spi.block_sigma_min(X, d, n, 0, True)
    print("d=%d r=%d n=%d nu=%g: eigen-gap %.3f, least block singular value %.4f" % (d, r, n, prw.CHAIN_NU, gap, smin))
    assert gap >= spi.GAP and smin >= spi.BLOCK_SIGMA_MIN


@pytest.mark.parametrize("d,r,n", CASES)
def test_reference_stays_inside_the_bounds(d, r, n):
    """float64 X X^T against the longdouble one within spi.gram_bound; the projected reference has proper rotations"""
    X = prw.chain_point(d, r, n)
    err = np.abs((X @ X.T).astype(spi.LD) - spi.gram_ld(X))
    assert (err <= spi.gram_bound(X)).all()
    ref = spi.project_reference(X, d, n, 0, True)
    assert (np.linalg.det(spi.rotation_blocks(ref["P"], d, n, 0, True)) > 1 - 64 * spi.EPS).all()
    assert ref["npos"] in (0, n)


@pytest.mark.parametrize("d,n,R", sorted({(d, n, R) for d, n, R, _ in prw.CHAIN_CASES}))
def test_per_agent_sum_is_the_gram_matrix(d, n, R):
    """sum_a X_a X_a^T over the pose-graph agents' contiguous blocks (n // R poses each, the last takes the rest) is
    X X^T within the bound, whatever the grouping: the blocks tile the columns"""
    r = 5
    X = prw.chain_point(d, r, n)
    per, w = n // R, d + 1
    ends = [(a + 1) * per if a < R - 1 else n for a in range(R)]
    cols = [np.arange(a * per * w, ends[a] * w) for a in range(R)]
    assert np.array_equal(np.concatenate(cols), np.arange(w * n))
    G = np.zeros((r, r))
    for c in cols:
        G = G + X[:, c] @ X[:, c].T
    assert (np.abs(G.astype(spi.LD) - spi.gram_ld(X)) <= spi.gram_bound(X)).all()


@pytest.mark.parametrize("d", spi.DIMS)
def test_reflect_family_on_a_chain(d):
    """the rotation part of spi.reflect_case in the SE ordering (what the rank test feeds a pose-graph job): the numpy
    reference counts m or n - m positive determinants and lands on the expected branch"""
    n = spi.REFLECT_DIMS["n"]
    for m in spi.REFLECT_KEEP + spi.REFLECT_FLIP:
        Xd, X = prw.reflect_chain_case(d, m)
        ref = spi.project_reference(X, d, n, 0, True)
        assert ref["npos"] in (m, n - m)
        kept, flipped = (spi.project_blocks(Xd, d, n, 0, True, f) for f in (False, True))
        want = m > n - m
        G = ref["P"].T @ ref["P"]
        dist = {False: np.abs(G - kept.T @ kept).max(), True: np.abs(G - flipped.T @ flipped).max()}
        assert dist[want] <= 1e-10 and dist[not want] > 1e-3, (m, dist)


def test_python_view_and_drivers():
    """Exchange.project and the two rank drivers that end with it; the plain rank drivers keep their arguments"""
    import inspect
    import dcora_amd as da
    from dcora_amd import driver
    assert callable(getattr(da.Exchange, "project", None))
    for plain, projected in ((driver.multi_robot_staircase_ranks, driver.multi_robot_staircase_ranks_projected),
                             (driver.raslam_staircase_ranks, driver.raslam_staircase_ranks_projected)):
        assert inspect.signature(plain).parameters["round_on_device"].default is False
        assert inspect.signature(projected).parameters["round_on_device"].default is True
    for name in ("project", "evaluate"):
        assert callable(getattr(driver._RanksJob, name, None)), name
