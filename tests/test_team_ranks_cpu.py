"""The team protocol's transport between the ranks of a job, host half (dcora_exchange_host_selftest_team; no GPU): the
status slots of the shared segment, their sequence and read words and the bounded waits are the code the GPU ranks run
(dcora_amd/csrc/exchange_slots.h, exchange.hip), host stores stand in for the ranked k_rel_change.  Real processes, ranks
that drift apart, a rank without agents, a rank that dies; and the same header under ASan + UBSan as a plain program."""
import os
import subprocess
import sys
import threading
import types
import uuid

import numpy as np
import pytest

import common
import team_rules_ref as ref

ROOT = os.path.dirname(common.HERE)
R, ROUNDS = 5, 60


def script_checksum(R, rounds):
    """the rehearsal's script (exchange_slots.h, team_rehearsal) through the rules as tests/team_rules_ref.py states them,
    folded in the library's order"""
    p = types.SimpleNamespace(max_num_iters=1 << 30, rel_change_tol=5e-3, robust_opt_num_weight_updates=3,
                              robust_opt_num_resets=0, robust_opt_inner_iters=7, robust_opt_min_convergence_ratio=0.8)
    status = [None] * R
    updates = inner = latest = 0
    total = 0.0
    for q in range(1, rounds + 1):
        agents = [a for a in range(R) if a % 2 == (q // 3) % 2] if q % 3 == 0 else [q % R]
        inner += 1
        for a in agents:
            rel = 0.001 * float((7 * q + 3 * a) % 11)
            ready = ref.ready_to_terminate(p, True, updates, (q + a) % 5 != 0, rel, 4, min(updates, 2), 6)
            status[a] = dict(state=ref.INITIALIZED, iteration_number=q, ready_to_terminate=ready, relative_change=rel)
        term = ref.should_terminate(p, True, q, updates, status)
        upd = ref.should_update_weights(p, True, updates, inner, latest, status)
        for a, st in enumerate(status):
            if st is not None:
                total += (a + 1) * (float(st["iteration_number"]) + 0.5 * int(st["ready_to_terminate"]) +
                                    st["relative_change"])
        total += 1000.0 * int(term) + 2000.0 * int(upd)
        if upd:
            updates, inner, latest = updates + 1, 0, q
            status = [None] * R
    return total, updates


def _team_rank(rank, world, job, R, rounds, skew_us, tmpdir, timeout_s=None, die_after_s=None):
    import ctypes as C
    if timeout_s is not None:
        os.environ["DCORA_EXCHANGE_TIMEOUT_S"] = str(timeout_s)
    sys.path.insert(0, os.path.dirname(common.HERE))
    from dcora_amd import capi
    if die_after_s is not None:  # this rank leaves the job in the middle of its run
        threading.Timer(die_after_s, lambda: os._exit(9)).start()
    cs = C.c_double()
    rc = capi.lib().dcora_exchange_host_selftest_team(job.encode(), rank, world, R, rounds, skew_us, C.byref(cs))
    msg = capi.lib().dcora_last_error().decode()
    np.save(os.path.join(tmpdir, "cs%d.npy" % rank), np.array([rc, cs.value]))
    if rc:
        raise RuntimeError("rank %d: status %d: %s" % (rank, rc, msg))


def test_the_script_exercises_the_rules():
    """(so that the checksum cannot agree emptily) the scripted run re-weights by the inner-iteration cap and by
    agreement, and holds ready and unready statuses"""
    want, updates = script_checksum(R, ROUNDS)
    assert updates == 3 and want > 0


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("skew_us", [0, 500])
def test_every_rank_holds_the_same_statuses_and_decisions(built, tmp_path, world, skew_us):
    """4 processes / 5 agents leave one rank without agents: it collects, settles and decides all the same.  The
    checksum folds every status and both decisions of every round: the same on every rank, for both skews (the same
    expected value), and equal to the rules restated in Python on the same script."""
    import torch.multiprocessing as mp
    job = "tcpu%s" % uuid.uuid4().hex[:10]
    mp.spawn(_team_rank, args=(world, job, R, ROUNDS, skew_us, str(tmp_path)), nprocs=world, join=True)
    want, _ = script_checksum(R, ROUNDS)
    for k in range(world):
        rc, cs = np.load(tmp_path / ("cs%d.npy" % k))
        assert rc == 0 and cs == want, (k, rc, cs, want)
    assert not os.path.exists("/dev/shm/dcora_" + job)


def test_a_rank_that_exits_mid_run_takes_the_others_out(built, tmp_path):
    """rank 1 of three leaves in the middle of a run that would go on for hours: the statuses and read words it owes
    never arrive, the other two give up within DCORA_EXCHANGE_TIMEOUT_S with an error, never hang"""
    import multiprocessing as mp
    import time
    world, rounds, timeout_s = 3, 50_000_000, 3.0
    job = "tcpu%s" % uuid.uuid4().hex[:10]
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_team_rank, args=(k, world, job, 6, rounds, 100, str(tmp_path), timeout_s,
                                                  1.0 if k == 1 else None)) for k in range(world)]
    for p in procs:
        p.start()
    t0 = time.time()
    procs[1].join(60)
    assert procs[1].exitcode == 9
    for k in (0, 2):
        procs[k].join(timeout_s + 20)
        assert procs[k].exitcode is not None, "rank %d still runs %.0f s after the start" % (k, time.time() - t0)
        assert procs[k].exitcode != 0
        rc, _ = np.load(tmp_path / ("cs%d.npy" % k))
        assert rc != 0


def test_team_transport_under_asan_ubsan(tmp_path):
    """exchange_slots.h -- slots, read words, waits, the rehearsal -- compiled with a program of its own under ASan + UBSan
    and run as a plain executable in 3 processes: no report, every rank's checksum the scripted one"""
    exe = str(tmp_path / "san_host_team")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "dcora_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(common.HERE, "cpp", "san_host_team.cpp"), "-lpthread", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    out = subprocess.run([exe, "3", str(R), str(ROUNDS), "200"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    want, _ = script_checksum(R, ROUNDS)
    got = [float(line.split()[2]) for line in out.stdout.splitlines() if line.startswith("checksum")]
    assert got == [want] * 3 and "ok 1" in out.stdout, out.stdout
