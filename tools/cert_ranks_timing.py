"""What a refused certificate costs a two-rank job (tools/cert_timing.py times the single session's): sphere2500 /
5 agents / r = 5 on two ranks that share one GPU, ten RBCD iterations from a random point, then dcora_exchange_certify
`--reps` times -- the PSD test fails, so the Lanczos stage runs with every inner product through allreduce_sum.

    python tools/cert_ranks_timing.py [--reps 5] [--lib PATH/libdcora_hip.so]

Prints rank 0's JSON line: the milliseconds of every call, their median and spread, the matvecs and lambda_min of the
last (two builds that compute the same thing print the same two)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from team_ranks_cost import R, RANK, WORLD, launch_ranks, spread  # noqa: E402


def rank_main(a):
    if a.lib:
        from lib_window import use_library
        use_library(a.lib)
    import common
    import dcora_amd as da
    from dcora_amd import driver
    ds = common.product_dataset("sphere2500")
    X0 = common.random_point(RANK, ds.d, ds.n, 3, da.manifold_project)
    s = da.RbcdSession(ds, num_robots=R, r=RANK, rank=a.rank, world_size=WORLD)
    ex = da.Exchange(s, a.job)
    ex.set_X(X0)
    driver.exchange_run(ex, max_iters=10, rgrad_tol=0.0)
    Q = da.build_Q_pgo(ds) if a.rank == 0 else None
    ms, cert = [], None
    for _ in range(a.reps + 1):  # (the first call is the warm-up)
        ex.barrier()
        t0 = time.perf_counter()
        cert = ex.certify(Q, 1e-3, (ds.d + 1) * ds.n)
        ms.append(1e3 * (time.perf_counter() - t0))
    if a.rank == 0:
        print(json.dumps({"lib": a.lib or "built", "case": "sphere2500/5 agents/r=5, 2 ranks on one GPU, refused",
                          "certify_ms": ms[1:], "ms": spread(ms[1:]), "certified": cert[0], "lambda_min": cert[2],
                          "matvecs": cert[4], "distributed": cert[5]}), flush=True)
    ex.barrier()
    ex.close()
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--job", default="")
    a = ap.parse_args()
    if a.rank >= 0:
        return rank_main(a)
    launch_ranks(__file__, ["--reps", str(a.reps)] + (["--lib", a.lib] if a.lib else []))


if __name__ == "__main__":
    main()
