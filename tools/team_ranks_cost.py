"""What the team protocol costs a multi-rank job per iteration: sphere2500 / 5 agents / r = 5 on two ranks that share
one GPU, every rank holding two jobs -- the team off and on (Exchange.enable_team: on the hosting rank the ranked
k_rel_change behind the selected agent's update, on every rank one bounded spin on the agent's status slot before the
evaluation) -- timed in alternating windows of RBCD iterations from the same start point, after a warm-up of both.

    python tools/team_ranks_cost.py [--windows 5] [--iters 300] [--lib PATH/libdcora_hip.so]

Starts one process per rank (itself with --rank) and prints rank 0's JSON line: iterations per second of every window,
their medians and spreads, the on/off gap.  The spread of the `off` windows among themselves is the noise floor the
gap is read against; tools/team_status_cost.py gives the single-process figure (one launch).  --lib measures another
build of the library (tools/lib_window.py's use_library): a process loads one, so the caller alternates runs."""
import argparse
import json
import os
import subprocess
import sys
import time
import uuid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORLD, R, RANK = 2, 5, 5


def spread(v):
    import numpy as np
    v = np.asarray(v)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "rel_spread": float((v.max() - v.min()) / np.median(v))}


def rank_main(a):
    import numpy as np
    if a.lib:
        from lib_window import use_library
        use_library(a.lib)
    import common
    import dcora_amd as da
    from dcora_amd import driver
    ds = common.product_dataset("sphere2500")
    X0 = common.random_point(RANK, ds.d, ds.n, 3, da.manifold_project)
    jobs = {}
    for key in ("off", "on"):
        s = da.RbcdSession(ds, num_robots=R, r=RANK, rank=a.rank, world_size=WORLD)
        ex = da.Exchange(s, a.job + key)
        if key == "on":
            ex.enable_team()
        jobs[key] = (s, ex)

    def window(key):
        s, ex = jobs[key]
        ex.set_X(X0)
        s.synchronize()
        ex.barrier()
        t0 = time.perf_counter()
        out = driver.exchange_run(ex, max_iters=a.iters, rgrad_tol=0.0)
        s.synchronize()
        return out["iters"] / (time.perf_counter() - t0), out

    for key in jobs:  # warm-up
        window(key)
    rates = {"off": [], "on": []}
    same = True
    for _ in range(a.windows):
        r0, o0 = window("off")
        r1, o1 = window("on")
        rates["off"].append(r0)
        rates["on"].append(r1)
        same = same and np.array_equal(o0["cost"], o1["cost"]) and np.array_equal(o0["selected"], o1["selected"])
    if a.rank == 0:
        so, sn = spread(rates["off"]), spread(rates["on"])
        us_off, us_on = 1e6 / so["median"], 1e6 / sn["median"]
        info = jobs["on"][1].info()
        print(json.dumps({"lib": a.lib or "built", "case": "sphere2500/5 agents/r=5, 2 ranks on one GPU", "transport": info["transport"],
                          "wait": info["wait"], "iters_per_window": a.iters, "windows": a.windows,
                          "iters_per_s_off": rates["off"], "iters_per_s_on": rates["on"], "off": so, "on": sn,
                          "us_per_iter_off": us_off, "us_per_iter_on": us_on, "gap_us_per_iter": us_on - us_off,
                          "off_spread_us_per_iter": 1e6 / so["min"] - 1e6 / so["max"], "same_bits": bool(same)}),
              flush=True)
    for s, ex in jobs.values():
        ex.barrier()
        ex.close()
        s.close()


def launch_ranks(script, args):
    """one process per rank of `script` with `args`, --rank and a fresh --job (tools/cert_ranks_timing.py shares this)"""
    job = "tc%s" % uuid.uuid4().hex[:10]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.abspath(script)] + args + ["--rank", str(k), "--job", job],
                              env=env) for k in range(WORLD)]
    rcs = []
    for p in procs:
        try:
            rcs.append(p.wait(timeout=420))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    if any(rcs):
        raise SystemExit("a rank failed: %r" % rcs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--job", default="")
    a = ap.parse_args()
    if a.rank >= 0:
        return rank_main(a)
    launch_ranks(__file__, ["--windows", str(a.windows), "--iters", str(a.iters)] + (["--lib", a.lib] if a.lib else []))


if __name__ == "__main__":
    main()
