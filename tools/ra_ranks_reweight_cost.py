"""What a collective weight update costs on the ranks of a range-aided job (dcora_ra_rbcd_create_robust_ranks,
dcora_exchange_update_weights), beside what a user without it pays on the same ranks: destroy + create + set_X of every
rank's session and exchange with the same weights.  tools/ra_reweight_cost.py's problem -- full tiers.pyfg (4 robots x
2442 poses) with synthetic loop closures (tests/ra_loops.py) -- and its method: the two ways alternate, each figure is the
median of five repetitions after one warm-up of each, the preconditioner cache is cleared before every timed call.

The tool starts one process per rank, ALL ON DEVICE 0: the ranks share one GPU, so the figures say what the calls cost
there and nothing about a job with one GPU per rank.  Every rank enters a timed call from a barrier and reports its own
host clock; the job's figure of a repetition is the slowest rank's.

    python tools/ra_ranks_reweight_cost.py [--ranks W] [--out profiles/ra_ranks_reweight_cost.txt]
"""
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


def rank_main(a):
    import dcora_amd as da
    import ra_loops
    from dcora_amd import driver
    from dcora_amd import robust as rb
    rank, world, r = a.rank, a.ranks, a.r
    ra, twin = da.RADataset(a.path), da.RADataset(a.path)
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    params = rb.RobustCostParameters("GNC_TLS", **ra_loops.GNC_PARAMS)
    t0 = time.perf_counter()
    A, exA = da.ra_robust_ranked_session(ra, a.job, r, robust=params, rank=rank, world_size=world)
    t_create = 1e3 * (time.perf_counter() - t0)
    exA.set_X(X0)
    driver.exchange_run(exA, max_iters=8, rgrad_tol=0.0)
    B = exB = None
    t_in, t_fresh, counts = [], [], []
    for rep in range(-1, a.reps):  # rep -1: warm-up of both
        da.precond_cache_clear()
        exA.barrier()
        t0 = time.perf_counter()
        c = exA.update_weights()
        dt = 1e3 * (time.perf_counter() - t0)
        if rep >= 0:
            t_in.append(dt)
        counts.append([c["accepted"], c["rejected"], c["undecided"]])
        w, X = exA.get_weights(), exA.gather_X()
        twin.set_pose_pose_weights(w)
        da.precond_cache_clear()
        exA.barrier()
        t0 = time.perf_counter()
        if B is not None:
            exB.close()
            B.close()
        B = da.RaRbcdSession(twin, r, rank=rank, world_size=world)
        exB = da.Exchange(B, "%sf%d" % (a.job, rep + 1))
        exB.set_X(X)
        dt = 1e3 * (time.perf_counter() - t0)
        if rep >= 0:
            t_fresh.append(dt)
        driver.exchange_run(exA, max_iters=4, rgrad_tol=0.0)
    exA.barrier()
    exB.close()
    B.close()
    exA.close()
    A.close()
    np.savez(a.rank_out, t_in=np.array(t_in), t_fresh=np.array(t_fresh), counts=np.array(counts), create=t_create)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--poses", type=int, default=2442, help="poses kept per robot (2442: all of tiers)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("-r", type=int, default=3)
    ap.add_argument("--rank", type=int, default=-1, help=argparse.SUPPRESS)  # (a rank process of this tool)
    ap.add_argument("--job", default="", help=argparse.SUPPRESS)
    ap.add_argument("--path", default="", help=argparse.SUPPRESS)
    ap.add_argument("--rank-out", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rank >= 0:
        rank_main(a)
        return
    import dcora_amd as da
    import ra_loops
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the device")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tmp = tempfile.mkdtemp(prefix="ra_ranks_")
    path, info = ra_loops.write_loops_variant(tmp, P=a.poses, seed=11, per_pair=20, intra=20, outliers=20)
    ra = da.RADataset(path)
    ks = [len(ra.agent_columns[q][1]) for q in ra.robots]
    say("tiers, %d poses per robot, %d ranges, %d closures (%d outliers): k = %d, k_a = %s, r = %d" % (
        a.poses, ra.num_range, len(info["kind"]), info["kind"].count("outlier"), ra.k, ks, a.r))
    say("%d ranks, all on device 0 (the ranks share one GPU)" % a.ranks)
    job = "rc%s" % uuid.uuid4().hex[:10]
    outs = [os.path.join(tmp, "rank%d.npz" % k) for k in range(a.ranks)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--ranks", str(a.ranks), "--reps", str(a.reps),
                               "-r", str(a.r), "--rank", str(k), "--job", job, "--path", path, "--rank-out", outs[k]],
                              env=env) for k in range(a.ranks)]
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
    say("robust sessions and exchanges created in %s ms (by rank)" % " ".join("%.1f" % float(q["create"]) for q in res))
    for rep, c in enumerate(res[0]["counts"]):
        say("  rep %2d: accepted %d, rejected %d, undecided %d" % (rep - 1, c[0], c[1], c[2]))
    fmt = lambda v: "median %9.1f ms  min %9.1f  max %9.1f  raw %s" % (
        statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v))
    say("slowest rank of every repetition:")
    say("collective update_weights               %s" % fmt(list(np.max([q["t_in"] for q in res], axis=0))))
    say("destroy + create + set_X on every rank  %s" % fmt(list(np.max([q["t_fresh"] for q in res], axis=0))))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
