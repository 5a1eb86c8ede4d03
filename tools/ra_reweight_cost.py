"""What a weight update costs inside a live range-aided session, beside what a user without it pays: destroy + create +
set_X of a session with the same weights.  Full tiers.pyfg (4 robots x 2442 poses) with synthetic loop closures
(tests/ra_loops.py); each figure is the median of five alternated repetitions after one warm-up of each, the
preconditioner cache cleared before every timed call (a re-weight changes every agent's matrix: neither way finds its
inverse cached).  Below them, where the time of a rebuild goes: the per-agent regularisation (device Lanczos) and the
per-agent preconditioner (sparse partitioned inverse) timed on their own, and the host assembly.

    python tools/ra_reweight_cost.py [--out profiles/ra_reweight_cost.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--poses", type=int, default=2442, help="poses kept per robot (2442: all of tiers)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("-r", type=int, default=3)
    a = ap.parse_args()
    import dcora_amd as da
    import ra_loops
    from dcora_amd import robust as rb
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tmp = tempfile.mkdtemp()
    path, info = ra_loops.write_loops_variant(tmp, P=a.poses, seed=11, per_pair=20, intra=20, outliers=20)
    ra, twin = da.RADataset(path), da.RADataset(path)
    r = a.r
    ks = [len(ra.agent_columns[q][1]) for q in ra.robots]
    say("tiers, %d poses per robot, %d ranges, %d closures (%d outliers): k = %d, k_a = %s, r = %d" % (
        a.poses, ra.num_range, len(info["kind"]), info["kind"].count("outlier"), ra.k, ks, r))
    X0 = np.zeros((r, ra.k))
    X0[:ra.d] = ra.X_odom
    params = rb.RobustCostParameters("GNC_TLS", **ra_loops.GNC_PARAMS)
    t0 = time.perf_counter()
    A = da.RaRbcdSession(ra, r, robust=params)
    say("robust session created in %.1f ms" % (1e3 * (time.perf_counter() - t0)))
    A.set_X(X0)
    A.run(max_iters=8, rgrad_tol=0.0)
    B = None
    t_in, t_fresh = [], []
    for rep in range(-1, a.reps):  # rep -1: warm-up of both
        da.precond_cache_clear()
        t0 = time.perf_counter()
        counts = A.update_weights()
        dt = 1e3 * (time.perf_counter() - t0)
        if rep >= 0:
            t_in.append(dt)
        w, X = A.get_weights(), A.get_X()
        twin.set_pose_pose_weights(w)
        da.precond_cache_clear()
        t0 = time.perf_counter()
        if B is not None:
            B.close()
        B = da.RaRbcdSession(twin, r)
        B.set_X(X)
        dt = 1e3 * (time.perf_counter() - t0)
        if rep >= 0:
            t_fresh.append(dt)
        A.run(max_iters=4, rgrad_tol=0.0)
        say("  rep %2d: %s, mu %.3g" % (rep, counts, A.robust_info()["mu"]))
    fmt = lambda v: "median %9.1f ms  min %9.1f  max %9.1f  raw %s" % (
        statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v))
    say("in-place update_weights         %s" % fmt(t_in))
    say("destroy + create + set_X        %s" % fmt(t_fresh))
    # where a rebuild's time goes, stage by stage, with the weights as they stand
    t0 = time.perf_counter()
    twin.set_pose_pose_weights(A.get_weights())
    t_q = 1e3 * (time.perf_counter() - t0)
    t_blocks = t_reg = t_pre = 0.0
    for q in ra.robots:
        t0 = time.perf_counter()
        dims3, own, Qaa, C = twin.agent_blocks(q)
        t_blocks += 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        reg = da.precond_regularization(Qaa)
        t_reg += 1e3 * (time.perf_counter() - t0)
        da.precond_cache_clear()
        t0 = time.perf_counter()
        P = da.QuadraticProblem(r, ra.d, dims3[0], Qaa, reg=reg, l=dims3[1], b=dims3[2], layout=da.capi.LAYOUT_RA)
        t_pre += 1e3 * (time.perf_counter() - t0)
        P.close()
    say("stages on their own (4 agents summed, through the Python view: each includes its copies across the ABI):")
    say("  dataset handle + build_Q_ra + copy      %9.1f ms" % t_q)
    say("  extract_agent_blocks                    %9.1f ms" % t_blocks)
    say("  device_precond_regularization (Lanczos) %9.1f ms" % t_reg)
    say("  problem + preconditioner, cache cleared %9.1f ms" % t_pre)
    A.close()
    B.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
