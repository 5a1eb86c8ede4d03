"""The RBCD iteration with G formed by the local solve's start-point evaluation against every step as a launch of its
own (DCORA_CHAIN, read when a session is created): sphere2500 / 5 agents / r = 5, one session per chain in ONE process,
timed in alternated windows from the same start point after a warm-up of every session.

    python tools/rbcd_chain_ab.py [--windows 5]

Two windows, both driven like bench.py drives the loop (one dcora_rbcd_iterate per iteration from Python):
  sustained: 300 iterations after 30 untimed ones;
  driver:    iterations 7 .. 26 from the start point (bench.py --steps 20 --warmup 5), the median of 5 replays.

Prints one JSON line: microseconds per iteration of every window and chain, median / min / max per chain, the gap of
every chain to `launches` and the spread (max - min) of `launches` it is read against, and whether every chain ended
every window on the same bits (X, 2 f, |grad|)."""
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


def session(ds, R, r, chain):
    if chain != "default":
        os.environ["DCORA_CHAIN"] = chain
    try:
        return da.RbcdSession(ds, num_robots=R, r=r)
    finally:
        os.environ.pop("DCORA_CHAIN", None)


def window(s, X0, skip, count):
    """us per iteration of iterations skip + 1 .. skip + count from X0, and what the last one left"""
    s.set_X(X0)
    sel = 0
    for _ in range(skip):
        sel = s.iterate(sel)[3]
    s.synchronize()
    t0 = time.perf_counter()
    c2 = gn = 0.0
    for _ in range(count):
        c2, gn, _, sel = s.iterate(sel)
    s.synchronize()
    dt = time.perf_counter() - t0
    return 1e6 * dt / count, (s.get_X(), c2, gn, sel)


def stats(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the device")
    ds = common.product_dataset("sphere2500")
    R, r = 5, 5
    X0 = common.random_point(r, ds.d, ds.n, 3, da.manifold_project)
    chains = ["launches", "default"]
    S = {c: session(ds, R, r, c) for c in chains}
    kinds = {"sustained": (30, 300, 1), "driver": (6, 20, 5)}
    out = {"case": "sphere2500/5 agents/r=5", "windows": a.windows, "same_bits": True}
    for kind, (skip, count, replays) in kinds.items():
        for s in S.values():  # warm-up
            window(s, X0, skip, count)
        us = {c: [] for c in chains}
        for _ in range(a.windows):
            ends = {}
            for c in chains:  # alternated
                samples = []
                for _ in range(replays):
                    t, ends[c] = window(S[c], X0, skip, count)
                    samples.append(t)
                us[c].append(float(np.median(samples)))
            ref = ends["launches"]
            for c in chains:
                e = ends[c]
                out["same_bits"] = bool(out["same_bits"] and np.array_equal(e[0], ref[0]) and e[1:] == ref[1:])
        st = {c: stats(us[c]) for c in chains}
        out[kind] = {"iterations": [skip + 1, skip + count], "us_per_iteration": us, "stats": st,
                     "launches_spread_us": st["launches"]["max"] - st["launches"]["min"],
                     "gain_us": {c: st["launches"]["median"] - st[c]["median"] for c in chains if c != "launches"}}
    print(json.dumps(out), flush=True)
    for s in S.values():
        s.close()


if __name__ == "__main__":
    main()
