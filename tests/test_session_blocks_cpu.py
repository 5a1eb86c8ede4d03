"""The two host-only pieces the session core states once, under ASan + UBSan (CPU only; each a stand-alone program with
its own main, compiled as tests/test_host_sanitizers.py compiles san_host_csr.cpp):
  rank_change.h   the re-ranks of one rank change and their roll-back, driven with stand-in problems that count their
                  rerank calls and fail at a chosen call (tests/cpp/rank_change.cpp)
  agent_block.h   the global indices of a block's poses, unit spheres and landmarks, from column lists built from chosen
                  indices (tests/cpp/agent_block_states.cpp) and from the columns of every robot of the two range-aided
                  fixtures, held against the ownership the dataset assigns"""
import os
import subprocess

import numpy as np
import pytest

import common
from test_raslam import ra_path

ROOT = os.path.dirname(common.HERE)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")


def _compile(tmp_path, name):
    exe = str(tmp_path / name)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "dcora_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(common.HERE, "cpp", name + ".cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return exe


def _run(cmd):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=ENV)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    assert "FAILED" not in out.stdout, out.stdout
    return out.stdout


@pytest.fixture(scope="module")
def states_exe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("agent_block"), "agent_block_states")


def test_rank_change_rolls_back_what_it_re_ranked(tmp_path):
    """a failure at each of the four positions (1 central, 3 agents); commit; destruction with and without it; an owner
    that goes away; a roll-back whose own rerank fails: 4 + 1 + 1 + 1 + 4 groups"""
    out = _run([_compile(tmp_path, "rank_change")])
    assert out.count("ok ") == 11, out


def test_block_states_from_chosen_indices(states_exe):
    """d = 2 and 3: the SE ordering (twice), the range-aided one with l, b > 0, a landmark without a unit sphere and the
    reverse, a non-contiguous non-monotone pose set in each, a contiguous range from col0, the columns themselves"""
    out = _run([states_exe])
    assert out.count("ok ") == 14, out


@pytest.mark.parametrize("name", ["range_aided_slam_test_2d", "range_aided_slam_test_3d"])
def test_block_states_of_the_fixtures_are_the_datasets_ownership(built, states_exe, name):
    import dcora_amd as da
    ra = da.RADataset(ra_path(name))
    assert len(ra.robots) >= 2
    for robot in ra.robots:
        (na, la, ba), own = ra.agent_blocks(robot)[:2]
        out = _run([states_exe, "query"] + [str(x) for x in (ra.d, ra.n, ra.l, na, la, ba)] + [str(c) for c in own])
        got = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
        for key, owner in (("pose", ra.pose_robot), ("sphere", ra.sphere_robot), ("landmark", ra.landmark_robot)):
            want = np.flatnonzero(np.asarray(owner) == robot).tolist()
            print(name, "robot", robot, key, got[key], "owned:", want)
            assert sorted(got[key]) == want and len(set(got[key])) == len(got[key]), (name, robot, key)
        assert (len(got["pose"]), len(got["sphere"]), len(got["landmark"])) == (na, la, ba)
