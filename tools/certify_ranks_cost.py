"""What a certificate costs a two-rank job, live against what a caller does today.  Two ranks share one GPU.

  live : dcora_exchange_certify_live -- the ranks' device matrices, the values to rank 0 through the segment's X area
  today: collective dcora_exchange_get_weights (robust job), Q rebuilt on the host from them (build_Q_pgo / the
         range-aided builder), then dcora_exchange_certify with that Q on rank 0

Cases: sphere2500 / 5 agents / r = 5, a refused point (20 RBCD iterations from a random start) and an accepted one (the
optimum of a centralised solve); tiers / 4 robots / r = 3, refused (4 iterations from the odometry start).  The two
paths alternate inside one job, `--reps` timed calls each after one warm-up call each, a host clock around calls that
end synchronised (both leave through an all-reduce over the ranks), a barrier in front of every call.

    python tools/certify_ranks_cost.py [--reps 10]

Prints one JSON line per case (rank 0's): the milliseconds of each path with their spread, the rounds through the X
area, and what both paths computed.  With one GPU per rank the figure is not measured by this tool."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from team_ranks_cost import R, RANK, WORLD, launch_ranks, spread  # noqa: E402

ETA = 1e-3


def time_paths(ex, rank, reps, today_q, k, case):
    live_ms, today_ms, live, today = [], [], None, None
    for i in range(reps + 1):  # (the first call of each path is the warm-up: tables, analysis, first transfers)
        ex.barrier()
        t0 = time.perf_counter()
        live = ex.certify_live(ETA)
        live_ms.append(1e3 * (time.perf_counter() - t0))
        ex.barrier()
        t0 = time.perf_counter()
        Q = today_q()
        today = ex.certify(Q if rank == 0 else None, ETA, k)
        today_ms.append(1e3 * (time.perf_counter() - t0))
    if rank == 0:
        print(json.dumps({"case": case, "reps": reps, "live_ms": spread(live_ms[1:]), "today_ms": spread(today_ms[1:]),
                          "rounds": live[6]["rounds"], "live_ms_to_verdict_rank0": live[6]["ms"],
                          "certified": [bool(live[0]), bool(today[0])], "lambda_min": [live[2], today[2]],
                          "matvecs": [int(live[4]), int(today[4])], "distributed": [bool(live[5]), bool(today[5])]}),
              flush=True)


def rank_main(a):
    import numpy as np
    import common
    import dcora_amd as da
    from dcora_amd import driver
    from dcora_amd import robust as rb
    from test_raslam import ra_path
    gnc = rb.RobustCostParameters("GNC_TLS", GNCBarc=10.0, GNCMuStep=2.0)
    ds = common.product_dataset("sphere2500")
    k = (ds.d + 1) * ds.n

    def q_pgo(ex):
        def today():
            ds.vals[:, -1] = ex.get_weights()
            return da.build_Q_pgo(ds) if a.rank == 0 else None
        return today

    for tag, X0, iters in (("refused", np.load(os.path.join(a.dir, "X_random.npy")), 20),
                           ("accepted", np.load(os.path.join(a.dir, "X_optimum.npy")), 0)):
        s, ex = da.robust_ranked_session(ds, a.job + tag, num_robots=R, r=RANK, robust=gnc, rank=a.rank, world_size=WORLD)
        ex.set_X(X0)
        if iters:
            driver.exchange_run(ex, max_iters=iters, rgrad_tol=0.0)
        time_paths(ex, a.rank, a.reps, q_pgo(ex), k, "sphere2500/5 agents/r=5, 2 ranks on one GPU, " + tag)
        ex.barrier()
        ex.close()
        s.close()

    ra = da.RADataset(ra_path("tiers"))
    X0 = np.zeros((3, ra.k))
    X0[:ra.d] = ra.X_odom
    s, ex = da.ra_robust_ranked_session(ra, a.job + "tiers", 3, robust=gnc, rank=a.rank, world_size=WORLD)
    ex.set_X(X0)
    driver.exchange_run(ex, max_iters=4, rgrad_tol=0.0)

    def q_ra():
        ra.set_pose_pose_weights(ex.get_weights())
        return ra.Q
    time_paths(ex, a.rank, a.reps, q_ra, ra.k, "tiers/4 robots/r=3, 2 ranks on one GPU, refused")
    ex.barrier()
    ex.close()
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--job", default="")
    ap.add_argument("--dir", default="")
    a = ap.parse_args()
    if a.rank >= 0:
        return rank_main(a)
    # the two start points of sphere2500, computed once and handed to every rank as files (the same bits everywhere)
    import numpy as np
    import common
    import dcora_amd as da
    ds = common.product_dataset("sphere2500")
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "X_random.npy"), common.random_point(RANK, ds.d, ds.n, 3, da.manifold_project))
        X0 = np.zeros((RANK, (ds.d + 1) * ds.n))
        X0[:ds.d] = da.chordal_initialization(ds)
        P = da.QuadraticProblem(RANK, ds.d, ds.n, da.build_Q_pgo(ds))
        opt = da.QuadraticOptimizer(P, da.ROptParameters(RTR_iterations=200, RTR_tCG_iterations=400, gradnorm_tol=1e-6))
        np.save(os.path.join(d, "X_optimum.npy"), opt.optimize(X0))
        print("# centralised solve of sphere2500: |rgrad| %.3g" % opt.getOptResult()["gradNormOpt"], flush=True)
        P.close()
        launch_ranks(__file__, ["--reps", str(a.reps), "--dir", d])


if __name__ == "__main__":
    main()
