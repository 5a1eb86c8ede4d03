"""Host side of robust range-aided sessions (no device): which pose-pose measurements of a range-aided dataset are loop
closures (dcora_radataset_loop_closures), re-weighting a dataset (dcora_radataset_set_pose_pose_weights) against the
residual formula in numpy, the loop-closure variant of tiers (tests/ra_loops.py), and the condition under which the GNC
fixture's verdict -- exactly the injected outliers -- is the reference algorithm's own, with room."""
import gzip

import numpy as np
import pytest

import ra_loops
from test_raslam import ra_path

FIXTURES = ["range_aided_slam_test_2d", "range_aided_slam_test_3d", "tiers"]


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    return dcora_amd


def _file_mask(path):
    """odometry read off the symbols: both poses of one robot and consecutive among that robot's pose numbers"""
    opener = gzip.open if str(path).endswith(".gz") else open
    numbers, edges = {}, []
    with opener(path, "rt") as src:
        for line in src:
            f = line.split()
            if not f:
                continue
            if f[0].startswith("VERTEX_SE"):
                numbers.setdefault(f[2][0], set()).add(int(f[2][1:]))
            elif f[0].startswith("EDGE_SE2") and f[0] != "EDGE_SE2_XY" or f[0] == "EDGE_SE3:QUAT":
                edges.append((f[2], f[3]))
    rank = {rb: {q: i for i, q in enumerate(sorted(v))} for rb, v in numbers.items()}
    mask = []
    for a, b in edges:
        odo = a[0] == b[0] and rank[b[0]][int(b[1:])] == rank[a[0]][int(a[1:])] + 1
        mask.append(not odo)
    return np.array(mask, bool)


def errors_numpy(ra, ids, vals, X):
    """kappa |Y1 R - Y2|^2 + tau |p2 - p1 - Y1 t|^2 of every pose-pose measurement from the RA columns of X"""
    d, n, l = ra.d, ra.n, ra.l
    e = np.zeros(len(ids))
    for q, (i, j) in enumerate(ids):
        R = vals[q, :d * d].reshape(d, d, order="F")
        t = vals[q, d * d:d * d + d]
        kappa, tau = vals[q, d * d + d], vals[q, d * d + d + 1]
        Y1, Y2 = X[:, d * i:d * i + d], X[:, d * j:d * j + d]
        p1, p2 = X[:, d * n + l + i], X[:, d * n + l + j]
        e[q] = kappa * np.sum((Y1 @ R - Y2) ** 2) + tau * np.sum((p2 - p1 - Y1 @ t) ** 2)
    return e


@pytest.mark.parametrize("name", FIXTURES)
def test_loop_closure_mask_is_the_files(da, name):
    ra = da.RADataset(ra_path(name))
    mask = ra.loop_closures()
    assert mask.dtype == bool and mask.shape == (ra.num_pose_pose,)
    assert np.array_equal(mask, _file_mask(ra_path(name)))
    if name == "tiers":
        assert not mask.any()
    else:
        assert int(mask.sum()) == 4 and all(ra.pose_robot[i] != ra.pose_robot[j] or abs(i - j) > 1
                                            for (i, j), f in zip(ra.pose_pose()[0], mask) if f)


@pytest.mark.parametrize("name", ["range_aided_slam_test_2d", "range_aided_slam_test_3d"])
def test_set_pose_pose_weights_against_numpy(da, name):
    ra = da.RADataset(ra_path(name))
    ids, vals = ra.pose_pose()
    m = ra.num_pose_pose
    assert np.all(vals[:, -1] == 1.0)
    rng = np.random.default_rng(3)
    w1, w2 = rng.uniform(0.1, 2.0, m), rng.uniform(0.1, 2.0, m)
    w2[[1, m - 1]] = 0.0
    for r in (ra.d, ra.d + 2):
        X = rng.standard_normal((r, ra.k))
        err = errors_numpy(ra, ids, vals, X)
        tr = []
        for w in (w1, w2):
            ra.set_pose_pose_weights(w)
            assert np.array_equal(ra.pose_pose()[1][:, -1], w)  # dcora_radataset_copy sees them
            Q = ra.Q.to_scipy()
            tr.append(np.trace(X @ Q @ X.T))
        want = float(np.sum((w1 - w2) * err))
        assert abs((tr[0] - tr[1]) - want) <= 1e-10 * max(abs(tr[0]), abs(tr[1]), abs(want))
    # a weight of 0 removes the entries: Q(w2) holds what Q without those two measurements holds
    ra.set_pose_pose_weights(w2)
    nnz_zero = ra.Q.nnz
    ra.set_pose_pose_weights(np.where(w2 == 0, 1.0, w2))
    assert ra.Q.nnz > nnz_zero
    Qz = ra.Q.to_scipy().tocsr()
    ra.set_pose_pose_weights(w2)
    Q0 = ra.Q.to_scipy().tocsr()
    for e in (1, m - 1):  # the translation block -tau of the measurement: there with a weight, not even an explicit zero without
        ci, cj = ra.d * ra.n + ra.l + ids[e][0], ra.d * ra.n + ra.l + ids[e][1]
        assert Qz[ci, cj] != 0 and cj in Qz[ci].indices
        assert cj not in Q0[ci].indices
    # bad weights are refused and leave the object as it was
    for bad in (-0.5, np.nan, np.inf):
        w = w1.copy()
        w[2] = bad
        with pytest.raises(da.DcoraError) as e:
            ra.set_pose_pose_weights(w)
        assert e.value.status == 1
        assert np.array_equal(ra.pose_pose_weights, w2) and np.array_equal(ra.pose_pose()[1][:, -1], w2)
    with pytest.raises(ValueError):
        ra.set_pose_pose_weights(w1[:-1])
    ra.set_pose_pose_weights(None)
    assert np.all(ra.pose_pose()[1][:, -1] == 1.0)


def test_loops_variant_is_what_it_says(da, tmp_path):
    kw = dict(P=40, seed=5, per_pair=2, intra=3, outliers=5)
    path, info = ra_loops.write_loops_variant(tmp_path, **kw)
    ra = da.RADataset(path)
    assert ra.n == 4 * 40 and ra.b == 1 and ra.robots == [0, 1, 2, 3]
    assert info["n_odometry"] == 4 * 39 and ra.num_range == info["n_ranges"] == ra.l
    kind = info["kind"]
    assert (kind.count("inter"), kind.count("intra"), kind.count("outlier")) == (12, 12, 5)
    assert ra.num_pose_pose == info["n_odometry"] + len(kind)
    mask = ra.loop_closures()
    assert not mask[:info["n_odometry"]].any() and mask[info["n_odometry"]:].all()
    assert np.array_equal(mask, _file_mask(path))
    inl, outl = ra_loops.closure_masks(info)
    assert int(inl.sum()) == 24 and int(outl.sum()) == 5 and not (inl & outl).any()
    # every agent pair is covered by a ground-truth closure; the agent graph is connected
    ids, vals = ra.pose_pose()
    pairs = {tuple(sorted((int(ra.pose_robot[i]), int(ra.pose_robot[j])))) for (i, j), f in zip(ids, inl) if f}
    assert {p for p in pairs if p[0] != p[1]} == {(a, b) for a in range(4) for b in range(a + 1, 4)}
    col, nc = ra.colours()
    assert nc == 4
    # a re-read gives the injected measurements, and the ground-truth closures are exact at the ground truth
    sym = {}
    for rb in range(4):
        own = sorted((int(s[1:]), s) for s in info["poses"] if s[0] == ra_loops.ROBOTS[rb])
        for q, (_, s) in enumerate(own):
            sym[s] = rb * 40 + q
    for q, (a, b, x, y, th) in enumerate(info["closures"]):
        e = info["n_odometry"] + q
        assert tuple(ids[e]) == (sym[a], sym[b])
        assert np.array_equal(vals[e, 4:6], [x, y])
        assert np.allclose(vals[e, :4], [np.cos(th), np.sin(th), -np.sin(th), np.cos(th)], rtol=0, atol=1e-15)
        assert vals[e, 6] == pytest.approx(ra_loops.KAPPA, rel=1e-15) and vals[e, 7] == pytest.approx(ra_loops.TAU, rel=1e-15)
    err = errors_numpy(ra, ids, vals, ra.gt)
    assert err[inl].max() < 1e-20 * ra_loops.TAU + 1e-18
    assert err[outl].min() > 100.0
    # the same arguments write the same file
    path2, info2 = ra_loops.write_loops_variant(tmp_path, tag="again.pyfg", **kw)
    assert open(path).read() == open(path2).read() and info2["closures"] == info["closures"]


def gnc_reference_schedule(da, orc, ra, r, updates, params):
    """the GNC schedule over the oracle's centralised solver: weights 1, then `updates` rounds of (solve with Q(w),
    residuals in numpy, RobustCost weights on the loop closures, mu stepped) -> final residuals and weights"""
    ids, vals = ra.pose_pose()
    lc = ra.loop_closures()
    w = np.ones(ra.num_pose_pose)
    X = np.zeros((r, ra.k))
    X[:ra.d] = ra.X_odom
    res = None
    for u in range(updates):
        ra.set_pose_pose_weights(w)
        P = orc.Problem(r, ra.d, ra.n, orc.CSR.from_scipy(ra.Q.to_scipy()), reg=0.1, l=ra.l, b=ra.b)
        X, _ = P.optimize(X, gradnorm_tol=1e-2, RTR_iterations=20, RTR_tCG_iterations=100)
        res = np.sqrt(errors_numpy(ra, ids, vals, X))
        w[lc] = orc.robust_weights(res[lc], updates=u, cost_type="GNC_TLS", **params)
    ra.set_pose_pose_weights(None)
    return res, w


def test_gnc_fixture_condition(da, tmp_path):
    """the verdict "exactly the injected outliers" holds for the reference algorithm alone, with room: after the schedule
    every closure's residual is at least a factor 2 away from GNCBarc on its side"""
    from oracle import orc
    path, info = ra_loops.write_loops_variant(tmp_path, **ra_loops.GNC_FIXTURE)
    ra = da.RADataset(path)
    inl, outl = ra_loops.closure_masks(info)
    res, w = gnc_reference_schedule(da, orc, ra, 3, 12, ra_loops.GNC_PARAMS)
    barc = ra_loops.GNC_PARAMS["GNCBarc"]
    print("inlier residuals <= %.3f, outlier residuals >= %.3f" % (res[inl].max(), res[outl].min()))
    assert res[inl].max() <= barc / 2 and res[outl].min() >= 2 * barc
    assert np.all(w[outl] < 1e-8) and np.all(w[inl] > 1 - 1e-8)
