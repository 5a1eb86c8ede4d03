"""The exchange's host protocol as dcora_amd/csrc/exchange_slots.h states it, compiled with a program of its own
(tests/cpp/san_host_exchange.cpp) under ASan + UBSan and run as a plain executable, no GPU: the rehearsal in forked
ranks, a rank that leaves mid-run, and the segment's layout against the totals of the commit before the layout moved
(tests/golden/exchange_segment_totals.txt)."""
import os
import subprocess

import pytest

import common

ROOT = os.path.dirname(common.HERE)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("san") / "san_host_exchange")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "dcora_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(common.HERE, "cpp", "san_host_exchange.cpp"), "-lpthread", "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return out


def run(exe, *args, timeout=120):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=ENV)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    return out


@pytest.mark.parametrize("world,R", [(3, 8), (4, 5)])
def test_exchange_rehearsal_under_asan_ubsan(exe, world, R):
    """no report, and every rank prints the closed-form checksum of test_dist_cpu.py (4 ranks / 5 agents: one rank
    hosts nothing); the rehearsal checks every payload and every sum over the ranks itself"""
    rounds = 50
    out = run(exe, "run", world, R, rounds)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    want = sum((q + 0.5 * a) * (a + 1) + (0.25 * q - a) for q in range(1, rounds + 1) for a in range(R))
    got = [float(line.split()[2]) for line in out.stdout.splitlines() if line.startswith("checksum")]
    assert len(got) == world and all(abs(g - want) <= 1e-9 * abs(want) for g in got) and "ok 1" in out.stdout, out.stdout


def test_a_rank_that_exits_mid_run_is_given_up_on_within_the_timeout(exe):
    """rank 1 of three leaves after 2000 rounds of a run without end: the others return the timed-out or the
    peer-failed code within the timeout (3 s, plus what the 2000 rounds and the start took)"""
    timeout_s = 3.0
    out = run(exe, "die", 3, 6, timeout_s)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    gave_up = {int(f[1]): (int(f[2]), float(f[3])) for f in (line.split() for line in out.stdout.splitlines())
               if f and f[0] == "gave_up"}
    assert sorted(gave_up) == [0, 2], out.stdout
    for rc, seconds in gave_up.values():
        assert rc in (1, 2) and seconds < timeout_s + 2.0, out.stdout  # kWaitPeerFailed, kWaitTimeout


def test_segment_layout_keeps_alignment_order_and_the_totals_it_had(exe):
    """for every shape of the fixture (world = 1, R = 1, w = 0, kMaxRanks x kMaxAgents among them): the program's own
    checks of alignment, overlap and extent pass, and the total is what map_segment computed before the refactor"""
    with open(os.path.join(common.HERE, "golden", "exchange_segment_totals.txt")) as f:
        shapes = [[int(x) for x in line.split()] for line in f if line.strip() and not line.startswith("#")]
    assert len(shapes) >= 5
    for *shape, total in shapes:
        out = run(exe, "layout", *shape)
        assert out.returncode == 0 and out.stdout.split() == ["total", str(total)], (shape, out.stdout)
