"""The column-slot map of a workgroup tiling (dcora_amd/csrc/column_slots.h), without a device: the program
tests/cpp/column_slots.cpp under ASan + UBSan, the same map through the library's debug entry against a numpy
enumeration, and the figures of the headline data the one-launch tCG run's gather is sized by: on sphere2500 split over 5
agents (the driver's contiguous partition) the rows of a 2-pose workgroup name at most 8 pose blocks (32 columns), those of
a 12-pose workgroup at most 38 (152 columns)."""
import os
import subprocess

import numpy as np
import pytest

import common

ROOT = os.path.dirname(common.HERE)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")


def test_the_map_under_asan_ubsan(tmp_path):
    out = str(tmp_path / "column_slots")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "dcora_amd", "csrc"),
           os.path.join(common.HERE, "cpp", "column_slots.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    run = subprocess.run([out], capture_output=True, text=True, timeout=120, env=ENV)
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    assert run.returncode == 0 and run.stdout.rstrip().endswith("all ok"), run.stdout[-3000:] + run.stderr[-2000:]


def _numpy_map(rp, ci, n, dh, pb, cap_cols):
    """per workgroup (sorted distinct poses named, overflow), per entry the slot (65535 in an overflow workgroup)"""
    lists, slot = [], np.full(len(ci), 65535, np.int64)
    for p0 in range(0, n, pb):
        e0, e1 = rp[p0 * dh], rp[min(n, p0 + pb) * dh]
        poses = np.unique(np.r_[ci[e0:e1] // dh, np.arange(p0, min(n, p0 + pb))])
        over = len(poses) > cap_cols // dh
        lists.append((poses, over))
        if not over:
            slot[e0:e1] = np.searchsorted(poses, ci[e0:e1] // dh) * dh + ci[e0:e1] % dh
    return lists, slot


def _check(Q, n, dh, pb, cap_cols):
    import dcora_amd as da
    rp, ci = np.asarray(Q.rp), np.asarray(Q.ci)
    got = da.column_slots(rp, ci, n, dh, pb, cap_cols)
    lists, slot = _numpy_map(rp, ci, n, dh, pb, cap_cols)
    assert len(lists) == len(got["count"])
    for w, (poses, over) in enumerate(lists):
        assert got["count"][w] == len(poses) and bool(got["overflow"][w]) == over, (w, got["count"][w], len(poses))
        mine = got["list"][got["lp"][w]:got["lp"][w + 1]]
        assert np.array_equal(mine, [] if over else poses), (w, mine, poses)
    assert np.array_equal(got["slot"], slot)
    return got


def _agent_Q(ds, lo, hi):
    """Q of the agent that owns the poses [lo, hi) of ds: its private measurements fix the pattern (a shared loop closure
    only adds to the diagonal blocks of its ends)"""
    import dcora_amd as da
    ids = np.asarray(ds.ids)
    mine = (ids[:, 1] >= lo) & (ids[:, 1] < hi) & (ids[:, 3] >= lo) & (ids[:, 3] < hi)
    loc = ids[mine].copy()
    loc[:, 1] -= lo
    loc[:, 3] -= lo
    loc[:, 0] = loc[:, 2] = 0
    return da.build_Q_pgo(ds, n=hi - lo, ids=loc, vals=np.asarray(ds.vals)[mine])


@pytest.fixture(scope="module")
def sphere_agents(built):
    ds = common.product_dataset("sphere2500")
    per = ds.n // 5
    return [(_agent_Q(ds, a * per, ds.n if a == 4 else (a + 1) * per), (ds.n if a == 4 else (a + 1) * per) - a * per)
            for a in range(5)]


def test_the_entry_point_against_numpy_on_small_graphs(built):
    import dcora_amd as da
    rng = np.random.default_rng(5)
    for n, extra in ((2, 0), (3, 0), (33, 12), (50, 60)):
        edges = [(i, i + 1) for i in range(n - 1)]
        edges += [tuple(sorted(rng.choice(n, 2, replace=False))) for _ in range(extra)]
        edges += [(7, j) for j in range(9, n, 2)] if n == 50 else []   # a hub of about 20 neighbours
        ids = np.array([[0, i, 0, j] for i, j in edges])
        vals = np.tile(np.r_[np.eye(3).reshape(-1), 0.1, 0.2, 0.3, 100.0, 10.0, 1.0], (len(edges), 1))
        Q = da.build_Q_pgo(da.Dataset(3, n, ids, vals))
        for pb, cap in ((2, 64), (2, 16), (16, 256), (12, 256), (10, 256), (12, 48)):
            got = _check(Q, n, 4, pb, cap)
            if n == 50 and (pb, cap) == (2, 64):
                assert got["overflow"].sum() == 1 and got["overflow"][7 // 2] == 1   # the hub's workgroup, no other


def test_sphere2500_names_32_and_152_columns_at_most(sphere_agents):
    """the figures the caps are set against (at least 64 columns for the 2-pose tiling, 256 for the evaluation's)"""
    most2 = most12 = 0
    counts2 = []
    for Q, n in sphere_agents:
        two, twelve = _check(Q, n, 4, 2, 64), _check(Q, n, 4, 12, 256)
        assert two["overflow"].sum() == 0 and twelve["overflow"].sum() == 0
        most2, most12 = max(most2, two["count"].max()), max(most12, twelve["count"].max())
        counts2 += list(two["count"])
    print("2-pose workgroups name %d pose blocks at most, %.2f columns on average; 12-pose workgroups %d blocks"
          % (most2, 4 * np.mean(counts2), most12))
    assert 4 * most2 == 32 and 4 * most12 == 152
