"""Host rule of a robust multi-rank range-aided job (no device): which pose-pose measurements a rank weights and which
it owns (dcora_radataset_rank_edges, the rule RaRbcdSession::init_robust uploads by), against a count made from the
file's symbols alone: agent = position of the robot letter among the robots with poses, consecutive agents share a rank,
ceil(R / world_size) each; a measurement touches the ranks of both poses and is owned by the rank of its first."""
import gzip

import numpy as np
import pytest

import ra_loops
from test_raslam import ra_path


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    return dcora_amd


def _file_edges(path):
    """(robot letter of p1, robot letter of p2) of every pose-pose measurement, in file order, and the robots with poses"""
    opener = gzip.open if str(path).endswith(".gz") else open
    robots, edges = set(), []
    with opener(path, "rt") as src:
        for line in src:
            f = line.split()
            if not f:
                continue
            if f[0].startswith("VERTEX_SE"):
                robots.add(f[2][0])
            elif f[0].startswith("EDGE_SE2") and f[0] != "EDGE_SE2_XY" or f[0] == "EDGE_SE3:QUAT":
                edges.append((f[2][0], f[3][0]))
    return edges, sorted(robots)


def _expected(path, world):
    edges, robots = _file_edges(path)
    per = -(-len(robots) // world)
    rank_of = {rb: i // per for i, rb in enumerate(robots)}
    touches = np.zeros((world, len(edges)), bool)
    owns = np.zeros((world, len(edges)), bool)
    for e, (a, b) in enumerate(edges):
        touches[rank_of[a], e] = touches[rank_of[b], e] = True
        owns[rank_of[a], e] = True
    return touches, owns, len(robots)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("rank_edges")
    return {"range_aided_slam_test_2d": ra_path("range_aided_slam_test_2d"),
            "range_aided_slam_test_3d": ra_path("range_aided_slam_test_3d"),
            "loops": ra_loops.write_loops_variant(d, P=12, seed=4, per_pair=2, intra=1, outliers=2)[0]}


@pytest.mark.parametrize("name", ["range_aided_slam_test_2d", "range_aided_slam_test_3d", "loops"])
@pytest.mark.parametrize("world", [1, 2, 4])
def test_rank_edges_are_the_files(da, paths, name, world):
    ra = da.RADataset(paths[name])
    touches, owns, R = _expected(paths[name], world)
    assert touches.shape[1] == ra.num_pose_pose and R == len(ra.robots)
    got = [ra.rank_edges(k, world) for k in range(world)]
    for k in range(world):
        assert np.array_equal(got[k][0], touches[k]), (name, world, k)
        assert np.array_equal(got[k][1], owns[k]), (name, world, k)
        assert not np.any(got[k][1] & ~got[k][0])  # an owned measurement touches its owner
    # every pose-pose measurement has exactly one owner over the ranks, and is weighted by at most two
    assert np.array_equal(sum(o.astype(int) for _, o in got), np.ones(ra.num_pose_pose, int))
    ntouch = sum(t.astype(int) for t, _ in got)
    assert ntouch.min() >= 1 and ntouch.max() <= 2
    if world == 1:
        assert got[0][0].all() and got[0][1].all()
    if name == "loops" and world == 2:
        assert (ntouch == 2).any() and (ntouch == 1).any()  # closures shared by both ranks, and others
    if world > R:  # more ranks than robots: the ranks past the last agent's have no edges
        assert R == 2 and world == 4
        for k in range(R, world):
            assert not got[k][0].any() and not got[k][1].any()


def test_rank_edges_refuses_a_bad_rank(da, paths):
    ra = da.RADataset(paths["range_aided_slam_test_3d"])
    for rank, world in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(da.DcoraError) as e:
            ra.rank_edges(rank, world)
        assert e.value.status == 1
