"""dcora_radataset_agent_colours: the colours of a range-aided problem's agents from the file alone (host only, no
device), by the greedy rule the sessions use (dcora_rbcd_agent_colours / dcora_ra_rbcd_agent_colours) on the adjacency
the owners of the measurements' endpoints give."""
import numpy as np
import pytest

from ra_ring import write_ring_variant
from test_raslam import ra_path


def test_tiers_is_k4_and_its_ring_variant_has_two_colours(built, tmp_path):
    import dcora_amd as da
    col, nc = da.RADataset(ra_path("tiers")).colours()
    assert col.tolist() == [0, 1, 2, 3] and nc == 4
    path, kept, gone = write_ring_variant(tmp_path)
    assert (kept, gone) == (5228, 2561)
    ring = da.RADataset(path)
    assert (ring.n, ring.l, ring.b, ring.k) == (9768, 5228, 1, 34533)
    assert [ring.agent_columns[rb][1].size for rb in ring.robots] == [8689, 8580, 9249, 8015]
    col, nc = ring.colours()
    assert col.tolist() == [0, 1, 0, 1] and nc == 2


@pytest.mark.parametrize("name", ["range_aided_slam_test_2d", "range_aided_slam_test_3d"])
def test_two_robots_that_range_each_other_take_two_colours(built, name):
    import dcora_amd as da
    col, nc = da.RADataset(ra_path(name)).colours()
    assert col.tolist() == [0, 1] and nc == 2


def test_host_colours_agree_with_the_coupling_blocks(built, tmp_path):
    """the host rule reads measurement endpoints, the sessions read the coupling blocks C_a = Q[own_a, rest]: the same
    adjacency, hence the same colours (checked here on the host from Q's pattern; on the device in test_ra_ticks_gpu)"""
    import dcora_amd as da
    path, _, _ = write_ring_variant(tmp_path)
    for ra in (da.RADataset(path), da.RADataset(ra_path("tiers"))):
        owner = np.full(ra.k, -1)
        for i, rb in enumerate(ra.robots):
            owner[ra.agent_columns[rb][1]] = i
        Q = ra.Q.to_scipy().tocoo()
        R = len(ra.robots)
        adj = [set() for _ in range(R)]
        for a, b in zip(owner[Q.row], owner[Q.col]):
            if a != b and a >= 0 and b >= 0:
                adj[a].add(int(b))
        want = []
        for a in range(R):
            used = {want[b] for b in adj[a] if b < a}
            want.append(min(c for c in range(R) if c not in used))
        assert ra.colours()[0].tolist() == want
