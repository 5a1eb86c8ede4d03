"""What the agents' status costs a running session: sphere2500 / 5 agents / r = 5, two sessions in one process -- the
team protocol off and on (RbcdSession.enable_team: one k_rel_change launch per RBCD iteration, no synchronisation) --
timed in alternating windows of RBCD iterations from the same start point, after a warm-up of both.

    python tools/team_status_cost.py [--windows 5] [--iters 300] [--trace-only]

Prints one JSON line: iterations per second of every window, their medians and spreads, the on/off gap.  The spread
of the `off` windows among themselves is the noise floor the gap is read against.

The kernel's own time comes from a separate kernel trace of the same program (--trace-only runs one window of each
session and nothing else, so the trace shows k_rel_change launched by the `on` session only: as many calls as its
iterations):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/team_status_cost.py --trace-only"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import common  # noqa: E402
import dcora_amd as da  # noqa: E402


def window(s, X0, iters):
    s.set_X(X0)
    s.synchronize()
    t0 = time.perf_counter()
    out = s.run(max_iters=iters, rgrad_tol=0.0)
    s.synchronize()
    dt = time.perf_counter() - t0
    return out["iters"] / dt, out


def spread(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "rel_spread": float((v.max() - v.min()) / np.median(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the device")
    ds = common.product_dataset("sphere2500")
    R, r = 5, 5
    X0 = common.random_point(r, ds.d, ds.n, 3, da.manifold_project)
    off = da.RbcdSession(ds, num_robots=R, r=r)
    on = da.RbcdSession(ds, num_robots=R, r=r)
    on.enable_team()
    if a.trace_only:
        _, o0 = window(off, X0, a.iters)
        _, o1 = window(on, X0, a.iters)
        print(json.dumps({"trace_only": True, "iters_off": int(o0["iters"]), "iters_on": int(o1["iters"]),
                          "same_bits": bool(np.array_equal(o0["cost"], o1["cost"]))}), flush=True)
        return
    for s in (off, on):  # warm-up
        window(s, X0, a.iters)
    rates = {"off": [], "on": []}
    same = True
    for _ in range(a.windows):
        r0, o0 = window(off, X0, a.iters)
        r1, o1 = window(on, X0, a.iters)
        rates["off"].append(r0)
        rates["on"].append(r1)
        same = same and np.array_equal(o0["cost"], o1["cost"]) and np.array_equal(o0["selected"], o1["selected"])
    so, sn = spread(rates["off"]), spread(rates["on"])
    us_off, us_on = 1e6 / so["median"], 1e6 / sn["median"]
    print(json.dumps({"case": "sphere2500/5 agents/r=5", "iters_per_window": a.iters, "windows": a.windows,
                      "iters_per_s_off": rates["off"], "iters_per_s_on": rates["on"], "off": so, "on": sn,
                      "us_per_iter_off": us_off, "us_per_iter_on": us_on, "gap_us_per_iter": us_on - us_off,
                      "off_spread_us_per_iter": 1e6 / so["min"] - 1e6 / so["max"], "same_bits": bool(same)}), flush=True)
    off.close()
    on.close()


if __name__ == "__main__":
    main()
