"""Range-aided block updates per second on one device: do two local solves side by side (a coloured tick) beat the same
two solves one after the other?  On the ring variant of tiers.pyfg (tests/ra_ring.py: agent graph A-B-C-D-A, colours
[0, 1, 0, 1], so every tick of a sweep runs two agents), at r = 3 and r = 5, acceleration off, three loops that do the
same arithmetic (the sessions' iterates agree bit for bit, which the tool checks):

    a  RaRbcdSession.iterate(agent), the agents one after the other (each call ends in the central evaluation)
    s  iterate_set([agent]) for the same agents one after the other, one evaluate() per sweep: ticks without concurrency
    b  iterate_set(colour) per colour, one evaluate() per sweep: the coloured sweeps

A window is 20 sweeps from the odometry start (set_X before every window, so every window of every loop is the same
work), timed with a host clock around calls that end in a device synchronise; 5 warm-up sweeps; the loops' windows
alternate; the figure is the median of 5 windows, R block updates per sweep.

    python tools/ra_tick_timing.py [--loops a,s,b] [--ranks 3,5] [--windows 5] [--sweeps 20] [--warmup 5]

Loop a uses nothing the library lacked before the coloured range-aided ticks, so `--loops a` also runs on an older build.
Prints one JSON line per rank."""
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


def sweep(s, loop, sets):
    if loop == "a":
        for S in sets:
            for a in S:
                s.iterate(int(a))
        return
    for S in sets:
        if loop == "b":
            s.iterate_set(S)
        else:
            for a in S:
                s.iterate_set([int(a)])
    s.evaluate()


def case(ra, r, loops, windows, sweeps, warmup):
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    col, nc = ra.colours()
    sets = [np.flatnonzero(col == c).astype(np.int32) for c in range(nc)]
    sess = {lp: da.RaRbcdSession(ra, r, acceleration=False) for lp in loops}
    R = next(iter(sess.values())).R
    for lp, s in sess.items():
        s.set_X(X0)
        for _ in range(warmup):
            sweep(s, lp, sets)
    secs = {lp: [] for lp in loops}
    for _ in range(windows):
        for lp, s in sess.items():  # the loops' windows alternate
            s.set_X(X0)
            t0 = time.perf_counter()
            for _ in range(sweeps):
                sweep(s, lp, sets)
            s.get_X()  # (ends in a synchronise of the session's stream)
            secs[lp].append(time.perf_counter() - t0)
    X = {lp: s.get_X() for lp, s in sess.items()}
    first = X[loops[0]]
    out = {"case": "tiers ring variant", "r": r, "agents": R, "colours": [int(c) for c in col], "sweeps_per_window": sweeps,
           "windows": windows, "same_bits": bool(all(np.array_equal(first, x) for x in X.values()))}
    for lp in loops:
        rate = sweeps * R / np.asarray(secs[lp])
        out[lp] = {"block_updates_per_s": float(np.median(rate)), "min": float(rate.min()), "max": float(rate.max())}
    for s in sess.values():
        s.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", default="a,s,b")
    ap.add_argument("--ranks", default="3,5")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    loops = [lp for lp in a.loops.split(",") if lp]
    if not loops or any(lp not in ("a", "s", "b") for lp in loops):
        raise SystemExit("--loops takes a, s and b")
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the device")
    with tempfile.TemporaryDirectory() as tmp:
        ra = da.RADataset(write_ring_variant(tmp)[0])
        for r in (int(x) for x in a.ranks.split(",")):
            case(ra, r, loops, a.windows, a.sweeps, a.warmup)


if __name__ == "__main__":
    main()
