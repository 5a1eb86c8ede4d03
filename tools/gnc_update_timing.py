"""GNC round set-up: one in-place weight update of a live session (RbcdSession.update_weights) against what the
session-per-round flow (driver.multi_robot_gnc_example) pays for the same round -- X to the host, residuals on the
device, weights on the host, a new session with the new weights and set_X.

Both sides rebuild the same matrices and preconditioners for the same weights: the weights of update u come from
GNC-TLS after u updates, so every round is a preconditioner cache miss on both sides.  Between two timed rounds the
session runs a few RBCD iterations (not timed).  Times are host clocks around calls that end in a device
synchronise; the first round of each side is a warm-up.

    python tools/gnc_update_timing.py [--rounds K] [--lattice-rounds K] [--skip-lattice]

Prints one JSON line per case: ms per update_weights and ms per re-creation round (median, min, max)."""
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
from dcora_amd import driver, synth  # noqa: E402
from dcora_amd import robust as rb  # noqa: E402


def stats(ms):
    ms = np.asarray(ms[1:] if len(ms) > 1 else ms)  # (the first round warms up)
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max()), "rounds": int(ms.size)}


def case(name, ds, R, rounds, iters_between):
    r = 5
    params = rb.RobustCostParameters("GNC_TLS", GNCBarc=10.0, GNCMuStep=2.0)
    lc = driver.loop_closure_mask(ds, R)
    X0 = common.random_point(r, ds.d, ds.n, 3, da.manifold_project)
    da.precond_cache_clear()
    t0 = time.perf_counter()
    s = da.RbcdSession(ds, num_robots=R, r=r, robust=params)
    create_ms = 1e3 * (time.perf_counter() - t0)
    s.set_X(X0)
    upd_ms, rec_ms = [], []
    for u in range(rounds):
        s.run(max_iters=iters_between, rgrad_tol=0.0)
        t0 = time.perf_counter()
        s.update_weights()
        upd_ms.append(1e3 * (time.perf_counter() - t0))
    w_final = s.get_weights()
    # the updated session against a fresh one with its weights (acceleration off on both): the same iterations
    s.set_acceleration(False)
    X = s.get_X()
    f = da.RbcdSession(da.Dataset(ds.d, ds.n, ds.ids, np.column_stack([ds.vals[:, :-1], w_final])), num_robots=R, r=r,
                       acceleration=False)
    f.set_X(X)
    a, b = s.run(max_iters=3, rgrad_tol=0.0), f.run(max_iters=3, rgrad_tol=0.0)
    fresh_equal = bool(np.array_equal(a["cost"], b["cost"]) and np.array_equal(s.get_X(), f.get_X()))
    f.close()
    s.set_acceleration(True)
    # the session-per-round flow of multi_robot_gnc_example on the same iterate, with this round's weights
    for u in range(rounds):
        s.run(max_iters=iters_between, rgrad_tol=0.0)
        wds = da.Dataset(ds.d, ds.n, ds.ids, ds.vals.copy())
        w = wds.vals[:, -1]
        w[lc] = 1.0
        t0 = time.perf_counter()
        X = s.get_X()
        e = rb.measurement_errors(wds, X)
        w[lc] = rb.robust_weights(np.sqrt(e[lc]), params, num_updates=rounds + u)
        f = da.RbcdSession(wds, num_robots=R, r=r)
        f.set_X(X)
        rec_ms.append(1e3 * (time.perf_counter() - t0))
        f.close()
    s.close()
    out = {"case": name, "agents": R, "poses": ds.n, "measurements": ds.m, "robust_create_ms": create_ms,
           "update_weights_ms": stats(upd_ms), "recreate_round_ms": stats(rec_ms),
           "rejected_after_updates": int(np.sum(w_final[lc] < 1e-8)), "equals_fresh_session": fresh_equal}
    out["speedup_median"] = out["recreate_round_ms"]["median"] / out["update_weights_ms"]["median"]
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--lattice-rounds", type=int, default=4)
    ap.add_argument("--skip-lattice", action="store_true")
    a = ap.parse_args()
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the device")
    case("sphere2500/5", common.product_dataset("sphere2500"), 5, a.rounds, 5)
    if not a.skip_lattice:
        case("lattice100k/8", synth.lattice_se3(), 8, a.lattice_rounds, 2)


if __name__ == "__main__":
    main()
