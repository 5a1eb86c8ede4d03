"""GNC round set-up across ranks: one collective Exchange.update_weights of a robust multi-rank job
(dcora_rbcd_create_robust_ranks) on sphere2500 / 5 agents, against the single-process session's
RbcdSession.update_weights on the same problem (tools/gnc_update_timing.py measures the latter as well).

The tool starts one process per rank, all on device 0 (ranks sharing one GPU), plus the single-process session in
this process.  Between two timed updates every side runs a few RBCD iterations (not timed).  Times are host clocks
around calls that end in a device synchronise (the collective one also in the ranks' last allreduce); the first
update of each side is a warm-up.  Each rank reports its own clock; the job's figure is the slowest rank per round.

    python tools/gnc_ranks_timing.py [--ranks W] [--rounds K]

Prints one JSON line: ms per update (median, min, max) for the ranks and for the single process."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import uuid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import common  # noqa: E402
import dcora_amd as da  # noqa: E402
from dcora_amd import driver  # noqa: E402
from dcora_amd import robust as rb  # noqa: E402

NAME, R, r, BETWEEN = "sphere2500", 5, 5, 5
GNC = dict(GNCBarc=10.0, GNCMuStep=2.0)


def stats(ms):
    ms = np.asarray(ms[1:] if len(ms) > 1 else ms)  # (the first round warms up)
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max()), "rounds": int(ms.size)}


def rank_main(rank, world, job, rounds, out):
    ds = common.product_dataset(NAME)
    X0 = common.random_point(r, ds.d, ds.n, 3, da.manifold_project)
    s, ex = da.robust_ranked_session(ds, job, num_robots=R, r=r, robust=rb.RobustCostParameters("GNC_TLS", **GNC),
                                     rank=rank, world_size=world)
    ex.set_X(X0)
    ms = []
    for _ in range(rounds):
        driver.exchange_run(ex, max_iters=BETWEEN, rgrad_tol=0.0)
        ex.barrier()  # (every rank enters the timed call together)
        t0 = time.perf_counter()
        ex.update_weights()
        ms.append(1e3 * (time.perf_counter() - t0))
    w = ex.get_weights()
    ex.close()
    s.close()
    np.savez(out, ms=np.array(ms), w=w)


def single(rounds):
    ds = common.product_dataset(NAME)
    X0 = common.random_point(r, ds.d, ds.n, 3, da.manifold_project)
    s = da.RbcdSession(ds, num_robots=R, r=r, robust=rb.RobustCostParameters("GNC_TLS", **GNC))
    s.set_X(X0)
    ms = []
    for _ in range(rounds):
        s.run(max_iters=BETWEEN, rgrad_tol=0.0)
        t0 = time.perf_counter()
        s.update_weights()
        ms.append(1e3 * (time.perf_counter() - t0))
    w = s.get_weights()
    s.close()
    return ms, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--rank", type=int, default=-1, help=argparse.SUPPRESS)  # (a rank process of this tool)
    ap.add_argument("--job", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the device")
    if a.rank >= 0:
        rank_main(a.rank, a.ranks, a.job, a.rounds, a.out)
        return
    tmp = tempfile.mkdtemp(prefix="gnc_ranks_")
    job = "gt%s" % uuid.uuid4().hex[:12]
    outs = [os.path.join(tmp, "rank%d.npz" % k) for k in range(a.ranks)]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--ranks", str(a.ranks), "--rounds",
                               str(a.rounds), "--rank", str(k), "--job", job, "--out", outs[k]])
             for k in range(a.ranks)]
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
    job_ms = np.max(np.stack([q["ms"] for q in res]), axis=0)
    one_ms, w_one = single(a.rounds)
    out = {"case": "%s/%d" % (NAME, R), "ranks": a.ranks, "placement": "ranks sharing one GPU",
           "update_weights_ms_ranks": stats(list(job_ms)), "update_weights_ms_single_process": stats(one_ms),
           "weights_equal": bool(all(np.array_equal(q["w"], w_one) for q in res))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
