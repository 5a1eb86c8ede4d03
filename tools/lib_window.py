"""One build of the library on the headline loop (sphere2500 / 5 agents / r = 5), for A/B against another build: a process
loads ONE libdcora_hip.so, so the caller alternates processes.

    python tools/lib_window.py [--lib PATH/libdcora_hip.so] [--replays 3]

Two windows from the same start point, driven like bench.py drives the loop (rbcd_chain_ab.py's):
  sustained: 300 iterations after 30 untimed ones, `--replays` times;
  driver:    iterations 7 .. 26 from the start point, the median of 5 replays, `--replays` times.

Prints one JSON line: microseconds per iteration of every replay and a digest of what the last iteration of each window
left (X, 2 f, |grad|, the selection): two builds that compute the same thing print the same digests."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def window(s, X0, skip, count):
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
    h = hashlib.sha256(np.ascontiguousarray(s.get_X()).tobytes())
    h.update(np.array([c2, gn, sel], dtype=np.float64).tobytes())
    return 1e6 * dt / count, h.hexdigest()[:16]


def use_library(path):
    """point the package at another build of the library, before its first use (record_eval_chains.py shares this)"""
    import ctypes
    from dcora_amd import capi
    capi.LIB_PATH = os.path.abspath(path)
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in [n for n in capi.SIGNATURES if not hasattr(L, n)]:  # (an older build lacks the newer entries)
        del capi.SIGNATURES[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--replays", type=int, default=3)
    a = ap.parse_args()
    from dcora_amd import capi
    if a.lib:
        use_library(a.lib)
    import common
    import dcora_amd as da
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the device")
    ds = common.product_dataset("sphere2500")
    R, r = 5, 5
    X0 = common.random_point(r, ds.d, ds.n, 3, da.manifold_project)
    s = da.RbcdSession(ds, num_robots=R, r=r)
    out = {"lib": capi.LIB_PATH, "case": "sphere2500/5 agents/r=5"}
    for kind, (skip, count, inner) in {"sustained": (30, 300, 1), "driver": (6, 20, 5)}.items():
        window(s, X0, skip, count)  # warm-up
        us, dig = [], set()
        for _ in range(a.replays):
            samples = []
            for _ in range(inner):
                t, d = window(s, X0, skip, count)
                samples.append(t)
                dig.add(d)
            us.append(float(np.median(samples)))
        out[kind] = {"us_per_iteration": us, "digest": sorted(dig)}
    print(json.dumps(out), flush=True)
    s.close()


if __name__ == "__main__":
    main()
