"""The inputs and numpy references of the session rounding tests (tests/session_round_inputs.py), checked without a GPU:
every point the GPU tests use is well conditioned, numpy's float64 rounding of it stays within the rule of its
longdouble one, the references agree with the CPU oracle's alignment on tests/golden/block_factors.npz, and the
range-aided iterate family the cost test uses tells normalised sphere columns from rotated ones."""
import numpy as np
import pytest

import block_factors as bf
import session_round_inputs as sri
from test_raslam import ra_path

EPS = bf.EPS


@pytest.mark.parametrize("d", sri.DIMS)
def test_every_point_is_well_conditioned_and_float64_numpy_keeps_the_rule(d):
    """numpy's float64 result is the references' own algorithm (float64 products, the Newton iteration of polar_ld) run
    in float64.  LAPACK's SVD is not used for it: np.linalg.svd leaves single 3 x 3 blocks of these inputs 27 eps from
    the longdouble factor (d = 3, r = 3, n = 16, anchor 15, block 14), which says something about gesdd and nothing
    about the conditioning of the projection."""
    fx = bf.load()
    worst = 0.0
    for r in sri.ranks_of(d):
        for n in sri.SIZES:
            X = sri.lifted_point(d, r, n, sri.seed_of(d, r, n))
            for j in sorted({0, n - 1}):
                anchor = sri.anchor_of(X, d, j)
                smin, cond = sri.sigma_range(X, anchor, d)
                assert smin >= 0.5, (d, r, n, j, smin)
                ref, t = sri.round_reference(X, anchor, d)
                assert float(bf.orth_err(ref.astype(np.float64)).max()) <= 4 * EPS
                tol = sri.oracle_tolerance(X, anchor, d)
                M = (anchor[:, :d].T @ X).reshape(d, n, d + 1)
                R64 = sri.polar_ld(np.ascontiguousarray(M[:, :, :d].transpose(1, 0, 2)), np.float64)
                err = float(bf.block_err(R64.astype(sri.LD), ref).max())
                worst = max(worst, err / tol)
                assert err <= 8 * tol, (d, r, n, j, err, tol)
                assert bf.orth_err(R64).max() <= 8 * float(fx["oracle_orth"])
                t64 = M[:, :, d] - (anchor[:, :d].T @ anchor[:, d])[:, None]
                assert (np.abs(t64 - t).max(axis=0) <= 2 * r * sri.translation_bound(X, anchor, d) / 8).all()
    print("d=%d: float64 numpy / max(oracle_err, eps cond) <= %.2f" % (d, worst))


@pytest.mark.parametrize("d,r", bf.SO_DR)
def test_references_agree_with_the_oracle_alignment_on_the_fixture(d, r):
    """the references of the fixture test: the 50-digit rotations of the fixture, longdouble products for translations"""
    from oracle import orc
    fx = bf.load()
    groups = bf.so_groups(fx, d, r)
    Yin = np.concatenate([g.inp for g in groups])
    nb = len(Yin)
    T = 10 * np.random.default_rng(60 + r * 10 + d).standard_normal((r, nb))
    anchor = bf.so_anchor(fx, d, r)
    X = bf.se_matrix(Yin, T)
    out = orc.align_lifted_trajectory_to_frame(X, anchor, d, nb, True)
    R, t = sri.traj_blocks(out, d)
    for g, err in bf.so_group_errors(groups, R):
        assert err <= 8 * g.tol(), (g.name, err, g.tol())
    _, t_ref = sri.frame_blocks_ld(X, anchor, d)
    assert (np.abs(t - t_ref).max(axis=0) <= sri.translation_bound(X, anchor, d)).all()
    # the longdouble polar factor is the fixture's rotation where the block is well conditioned and proper
    o = 0
    for g in groups:
        if g.sign > 0 and g.tail == 0:  # (sigma_min 0.5)
            blocks, _ = sri.frame_blocks_ld(bf.se_matrix(g.inp), anchor, d)
            assert float(bf.block_err(sri.polar_ld(blocks), g.ref.astype(sri.LD)).max()) <= 8 * g.tol(), g.name
            o += 1
    assert o >= 1


def test_chain_datasets_are_what_the_sessions_need():
    import dcora_amd as da
    for d, r, n in sri.size_cases():
        ds = sri.chain_dataset(da.Dataset, d, n, sri.seed_of(d, r, n))
        assert ds.n == n and ds.m >= n - 1 and 1 <= sri.robots_of(n) <= 3 and n // sri.robots_of(n) >= 1
        if ds.m:
            assert ds.ids[:, [1, 3]].max() < n and (ds.ids[:, 1] < ds.ids[:, 3]).all()
    assert {sri.robots_of(n) for n in sri.SIZES} == {1, 2, 3}


@pytest.mark.parametrize("name", ["range_aided_slam_test_2d"])
def test_random_range_aided_points_tell_normalised_spheres_from_rotated_ones(name):
    """the cost test's condition, on the CPU, at the random point its iterate starts from: the cost of the rounded
    point with the sphere columns left as rotated differs from the cost with unit columns by far more than the bound
    the device cost is held to.  (An iterate that starts from [X_odom; 0] never leaves the rank-d subspace, where
    R0^T s is a unit vector already: that family could not show the difference.)"""
    import dcora_amd as da
    from oracle import orc
    ra = da.RADataset(ra_path(name))
    d, n, l, b, r = ra.d, ra.n, ra.l, ra.b, ra.d + 2
    rng = np.random.default_rng(4)
    X = orc.project_to_manifold(r, d, n, rng.uniform(-1, 1, (r, ra.k)), l=l, b=b)
    Xse = sri.se_from_ra(X, d, n, l)
    anchor = sri.anchor_of(Xse, d, 0)
    T, S, Lm = orc.ra_states_in_local_frame(X, r, d, n, l, b)  # (frame of pose 0: rotations projected)
    Q = ra.Q.to_scipy()
    c_unit, bound = sri.cost_reference(sri.ra_point(T, S, Lm, d, n, True), Q, r)
    c_rot, _ = sri.cost_reference(sri.ra_point(T, S, Lm, d, n, False), Q, r)
    assert l > 0 and np.abs(np.linalg.norm(S, axis=0) - 1).max() > 1e-3
    assert abs(c_unit - c_rot) > 100 * bound, (float(c_unit), float(c_rot), float(bound))
    assert anchor.shape == (r, d + 1)
