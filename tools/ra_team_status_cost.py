"""What the agents' status costs a running range-aided session: the ring variant of tiers (tests/ra_ring.py, four agents,
r = 3), two sessions in one process -- the team protocol off and on (RaRbcdSession.enable_team: one launch of
k_rel_change's range-aided form per RBCD iteration, no synchronisation) -- timed in alternating windows of RBCD
iterations from the same start point, after a warm-up of both.  After tools/team_status_cost.py.

    python tools/ra_team_status_cost.py [--windows 5] [--iters 200] [--trace-only off|on|both]

Prints one JSON line: iterations per second of every window, their medians and spreads, the on/off gap.  The spread
of the `off` windows among themselves is the noise floor the gap is read against: a range-aided iteration is paced from
the host and takes a millisecond or more, so that is all the comparison can claim.

The kernel's own time and the launch counts come from a separate kernel trace of the same program.  --trace-only runs
one window of the named session(s) and nothing else: with `both` the trace shows k_rel_change launched by the `on`
session only, as many calls as its iterations; with `off` the total number of kernel calls is what a session that did
not opt in launches (creation + one window), to set against the same run of another build:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/ra_team_status_cost.py --trace-only both"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import dcora_amd as da  # noqa: E402
from ra_ring import write_ring_variant  # noqa: E402


def window(s, X0, iters):
    s.set_X(X0)  # (synchronises the session's stream)
    t0 = time.perf_counter()
    out = s.run(max_iters=iters, rgrad_tol=0.0)  # (every iteration ends with a synchronising evaluation)
    dt = time.perf_counter() - t0
    return out["iters"] / dt, out


def spread(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "rel_spread": float((v.max() - v.min()) / np.median(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--trace-only", choices=["off", "on", "both"])
    a = ap.parse_args()
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the device")
    with tempfile.TemporaryDirectory() as tmp:
        ra = da.RADataset(write_ring_variant(tmp)[0])
        r = 3
        X0 = np.zeros((r, ra.k))
        X0[:ra.d] = ra.X_odom
        want = a.trace_only or "both"
        off = da.RaRbcdSession(ra, r) if want in ("off", "both") else None
        on = da.RaRbcdSession(ra, r) if want in ("on", "both") else None
    if on is not None:
        on.enable_team()
    if a.trace_only:
        outs = {name: window(s, X0, a.iters)[1] for name, s in (("off", off), ("on", on)) if s is not None}
        rec = {"trace_only": a.trace_only}
        rec.update({"iters_" + name: int(o["iters"]) for name, o in outs.items()})
        if len(outs) == 2:
            rec["same_bits"] = bool(np.array_equal(outs["off"]["cost"], outs["on"]["cost"]))
        print(json.dumps(rec), flush=True)
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
    print(json.dumps({"case": "tiers ring variant/4 agents/r=3", "iters_per_window": a.iters, "windows": a.windows,
                      "iters_per_s_off": rates["off"], "iters_per_s_on": rates["on"], "off": so, "on": sn,
                      "us_per_iter_off": us_off, "us_per_iter_on": us_on, "gap_us_per_iter": us_on - us_off,
                      "off_spread_us_per_iter": 1e6 / so["min"] - 1e6 / so["max"], "same_bits": bool(same)}), flush=True)
    off.close()
    on.close()


if __name__ == "__main__":
    main()
