"""Host side of the team protocol on range-aided sessions (no device): the loop-closure counts of Graph::statistics on a
RangeAidedSLAMGraph (dcora_radataset_loop_closure_stats; ref src/Graph.cpp:475-521 over private_lcs_ / shared_lcs_, which
by Graph::addMeasurement, :121-134, hold every measurement but pose-pose odometry) against an independent count in numpy:
with the file's weights, and with zeros and fractions planted on the pose-pose loop closures.  None of the stored fixtures
has a pose-landmark measurement, so one variant of the 2d fixture gets three written at run time: a private one and one
shared in either direction."""
import gzip

import numpy as np
import pytest

import ra_loops
from test_raslam import ra_path

NAMES = ["range_aided_slam_test_2d", "range_aided_slam_test_3d", "gnc", "2d_landmarks"]
LANDMARK_EDGES = ["EDGE_SE2_XY 0.0 A1 LA0 0.5 0.25 0.01 0.0 0.01\n", "EDGE_SE2_XY 0.0 A2 LB0 -0.5 1.0 0.01 0.0 0.01\n",
                  "EDGE_SE2_XY 0.0 B0 LA0 0.75 -0.5 0.01 0.0 0.01\n"]


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    return dcora_amd


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("ra_team")
    out = {"gnc": ra_loops.write_loops_variant(d, **ra_loops.GNC_FIXTURE)[0], "2d_landmarks": str(d / "2d_landmarks.pyfg")}
    with gzip.open(ra_path("range_aided_slam_test_2d"), "rt") as src, open(out["2d_landmarks"], "w") as dst:
        dst.writelines(src.readlines() + LANDMARK_EDGES)
    return out


def counted_measurements(ra):
    """every measurement but pose-pose odometry as (kind, owner robot of one end, of the other, weight)"""
    meas = ra.measurements()
    out = []
    ids, vals = meas["pose_pose"]
    for (i, j), v, lc in zip(ids, vals, ra.loop_closures()):
        if lc:
            out.append(("pose_pose", int(ra.pose_robot[i]), int(ra.pose_robot[j]), float(v[-1])))
    ids, vals = meas["pose_landmark"]
    for (i, j), v in zip(ids, vals):
        out.append(("pose_landmark", int(ra.pose_robot[i]), int(ra.landmark_robot[j]), float(v[-1])))
    ids, vals = meas["ranges"]
    owner = lambda kind, q: int(ra.landmark_robot[q] if kind else ra.pose_robot[q])
    for (t1, i, t2, j, _), v in zip(ids, vals):
        out.append(("range", owner(t1, i), owner(t2, j), float(v[-1])))
    return out


def stats_numpy(ra, robot):
    """a measurement counts at the owner of each end, once when both ends are one robot's; accepted iff its weight is
    exactly 1, rejected iff exactly 0"""
    mine = [w for _, a, b, w in counted_measurements(ra) if robot in (a, b)]
    return dict(accepted=sum(w == 1.0 for w in mine), rejected=sum(w == 0.0 for w in mine), total=len(mine))


def _dataset(da, name, paths):
    return da.RADataset(paths[name] if name in paths else ra_path(name))


@pytest.mark.parametrize("name", NAMES)
def test_loop_closure_stats_with_the_files_weights(da, paths, name):
    ra = _dataset(da, name, paths)
    counted = counted_measurements(ra)
    kinds = {k for k, _, _, _ in counted}
    assert {"range", "pose_pose"} <= kinds and ra.num_range > 0
    assert ("pose_landmark" in kinds) == (ra.num_pose_landmark > 0) == (name == "2d_landmarks")
    shared = [(a, b) for _, a, b, _ in counted if a != b]
    assert shared, "some measurement joins two robots"
    for robot in ra.robots:
        got = ra.loop_closure_stats(robot)
        assert got == stats_numpy(ra, robot), (robot, got)
        assert got["total"] > 0
    # a measurement shared by two robots appears at both: the totals count it twice, a private one once
    total = sum(ra.loop_closure_stats(q)["total"] for q in ra.robots)
    assert total == len(counted) + len(shared)
    # a robot that owns nothing has no loop closures
    assert ra.loop_closure_stats(max(ra.robots) + 1) == dict(accepted=0, rejected=0, total=0)


@pytest.mark.parametrize("name", NAMES)
def test_loop_closure_stats_with_zeros_and_fractions_planted(da, paths, name):
    ra = _dataset(da, name, paths)
    before = {q: ra.loop_closure_stats(q) for q in ra.robots}
    lc = np.flatnonzero(ra.loop_closures())
    assert len(lc) >= 4
    w = np.ones(ra.num_pose_pose)
    w[lc[0::3]] = 0.0
    w[lc[1::3]] = 0.25 + 0.5 * np.arange(len(lc[1::3])) / len(lc)
    w[np.flatnonzero(~ra.loop_closures())[0]] = 0.5  # odometry never counts, whatever its weight
    ra.set_pose_pose_weights(w)
    after = {q: ra.loop_closure_stats(q) for q in ra.robots}
    for robot in ra.robots:
        want = stats_numpy(ra, robot)
        assert after[robot] == want, (robot, after[robot], want)
        assert want["total"] == before[robot]["total"]  # fractions are counted in the total only
    assert sum(a["rejected"] for a in after.values()) > sum(b["rejected"] for b in before.values())
    assert sum(a["accepted"] + a["rejected"] for a in after.values()) < sum(a["total"] for a in after.values())
    ids = ra.pose_pose()[0]
    e = next(int(q) for q in lc[1::3] if ra.pose_robot[ids[q, 0]] != ra.pose_robot[ids[q, 1]])
    for robot in (int(ra.pose_robot[ids[e, 0]]), int(ra.pose_robot[ids[e, 1]])):  # a shared fraction: undecided at both
        assert after[robot]["accepted"] + after[robot]["rejected"] < after[robot]["total"]
    ra.set_pose_pose_weights(None)
    assert {q: ra.loop_closure_stats(q) for q in ra.robots} == before
