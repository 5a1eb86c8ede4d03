"""What the team protocol costs the ranks of a running range-aided job (dcora_exchange_team_enable_ra on an exchange of
dcora_exchange_create_ra: per dcora_exchange_rbcd_iterate one launch of k_rel_change's ranked range-aided form on the
rank hosting the selected agent, one status slot waited for and read on every rank).  tools/ra_team_status_cost.py's
problem -- the ring variant of tiers (tests/ra_ring.py, four agents, r = 3) -- and its method: every rank holds two jobs,
the team off and on, timed in alternated windows of greedy iterations from the same start point after a warm-up of both.

The tool starts one process per rank, ALL ON DEVICE 0: the ranks share one GPU, so the figures say what the protocol
costs there and nothing about a job with one GPU per rank.  Every rank enters a window from a barrier and reports its own
host clock; the job's figure of a window is the slowest rank's.

    python tools/ra_team_ranks_cost.py [--ranks 2] [--windows 5] [--iters 100] [--out FILE] [--lib ...]

The spread of the `off` windows among themselves is the noise floor the gap is read against.

--trace-only runs one job that did not opt in -- creation, set_X, one window -- and nothing else: the program of a kernel
trace whose total number of kernel calls over the ranks is set against the same run of another build
(--lib PATH/libdcora_hip.so: tools/lib_window.py's use_library; every rank process writes its own trace file):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/ra_team_ranks_cost.py --trace-only"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time
import uuid

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def window(ex, X0, iters):
    """-> seconds of `iters` greedy dcora_exchange_rbcd_iterate from X0, the costs, the selected agents"""
    ex.set_X(X0)
    ex.barrier()
    cost, sel = [], []
    selected = 0
    t0 = time.perf_counter()
    for _ in range(iters):
        c2, _, _, nxt = ex.iterate(selected)
        cost.append(c2)
        sel.append(selected)
        selected = nxt
    return time.perf_counter() - t0, np.array(cost), np.array(sel)


def rank_main(a):
    if a.lib:
        from lib_window import use_library
        use_library(a.lib)
    import dcora_amd as da
    rank, world, r = a.rank, a.ranks, a.r
    ra = da.RADataset(a.path)
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    jobs = {}
    for name in ("off",) if a.trace_only else ("off", "on"):
        s = da.RaRbcdSession(ra, r, rank=rank, world_size=world)
        jobs[name] = (s, da.Exchange(s, a.job + name))
    if "on" in jobs:
        jobs["on"][1].enable_team_ra()
    t = {name: [] for name in jobs}
    same = True
    for w in range(0 if a.trace_only else -1, a.windows):  # window -1: warm-up of both
        outs = {name: window(ex, X0, a.iters) for name, (_, ex) in jobs.items()}
        for name, o in outs.items():
            if w >= 0:
                t[name].append(o[0])
        if len(outs) == 2:
            same = same and np.array_equal(outs["off"][1], outs["on"][1]) and np.array_equal(outs["off"][2],
                                                                                            outs["on"][2])
    ready = sum(bool(st and st["ready_to_terminate"]) for st in
                (jobs["on"][1].agent_status(q) for q in range(jobs["on"][0].R))) if "on" in jobs else 0
    for s, ex in jobs.values():
        ex.barrier()
        ex.close()
        s.close()
    np.savez(a.rank_out, same=same, ready=ready, **{"t_" + name: np.array(v) for name, v in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("-r", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of the library (tools/lib_window.py's use_library)")
    ap.add_argument("--rank", type=int, default=-1, help=argparse.SUPPRESS)  # (a rank process of this tool)
    ap.add_argument("--job", default="", help=argparse.SUPPRESS)
    ap.add_argument("--path", default="", help=argparse.SUPPRESS)
    ap.add_argument("--rank-out", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rank >= 0:
        rank_main(a)
        return
    if a.lib:
        from lib_window import use_library
        use_library(a.lib)
    import dcora_amd as da
    from ra_ring import write_ring_variant
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the device")
    if a.trace_only:
        a.windows = 1
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tmp = tempfile.mkdtemp(prefix="ra_team_ranks_")
    path = write_ring_variant(tmp)[0]
    ra = da.RADataset(path)
    say("tiers ring variant, %d agents, k = %d, r = %d; %d ranks, all on device 0 (the ranks share one GPU; one GPU per "
        "rank is NOT measured)" % (len(ra.robots), ra.k, a.r, a.ranks))
    job = "tc%s" % uuid.uuid4().hex[:10]
    outs = [os.path.join(tmp, "rank%d.npz" % k) for k in range(a.ranks)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.abspath(__file__), "--ranks", str(a.ranks), "--windows", str(a.windows), "--iters",
           str(a.iters), "-r", str(a.r), "--job", job, "--path", path] + (["--trace-only"] if a.trace_only else []) + (
               ["--lib", a.lib] if a.lib else [])
    procs = [subprocess.Popen(cmd + ["--rank", str(k), "--rank-out", outs[k]], env=env) for k in range(a.ranks)]
    try:
        for p in procs:
            p.wait(timeout=600)
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        raise
    if any(p.returncode != 0 for p in procs):
        raise SystemExit("a rank failed: %s" % [p.returncode for p in procs])
    res = [np.load(o) for o in outs]
    if a.trace_only:
        say("one job without a team: creation, set_X, %d iterations of dcora_exchange_rbcd_iterate" % a.iters)
        return
    us = {name: 1e6 * np.max([q["t_" + name] for q in res], axis=0) / a.iters for name in ("off", "on")}
    say("%d alternated windows of %d greedy dcora_exchange_rbcd_iterate each, after one warm-up window of both jobs; "
        "us per iterate, slowest rank of every window" % (a.windows, a.iters))
    fmt = lambda v: "median %8.1f  min %8.1f  max %8.1f  raw %s" % (statistics.median(v), min(v), max(v),
                                                                  " ".join("%.1f" % x for x in v))
    say("team off  %s" % fmt(list(us["off"])))
    say("team on   %s" % fmt(list(us["on"])))
    gap = statistics.median(us["on"]) - statistics.median(us["off"])
    spread = float(us["off"].max() - us["off"].min())
    say("on - off (medians) %+.1f us per iterate; spread of the off windows among themselves %.1f us: the difference is "
        "%s" % (gap, spread, "resolved" if abs(gap) > spread else "NOT resolved by this measurement"))
    say("both jobs ran the same costs and selected agents in every window: %s; agents ready to terminate at the end: %d"
        % (all(bool(q["same"]) for q in res), int(res[0]["ready"])))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
