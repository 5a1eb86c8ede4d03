"""one rank of a multi-process job that certifies itself through dcora_exchange_certify_live; started by
tests/test_certify_ranks_gpu.py and by nothing else.  argv: rank world job scenario out_dir.  The scenario's inputs
(datasets by name, start points, weights) lie in out_dir/spec.npz; the rank writes out_dir/rank<k>.npz.

Every certificate a scenario takes is stored as a record "c<i>_*": what certify_live returned, what
dcora_exchange_certify returned for the host Q of the job's weights in the same place, and the gathered X."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

ETA = 1e-3
GNC = dict(GNCBarc=10.0, GNCMuStep=2.0)


def main():
    rank, world, job, scenario, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    import common
    import dcora_amd as da
    from dcora_amd import capi, driver
    from dcora_amd import robust as rb
    from test_raslam import ra_path
    spec = np.load(os.path.join(out_dir, "spec.npz"), allow_pickle=False)
    name = str(spec["name"])
    R, r, iters = int(spec["R"]), int(spec["r"]), int(spec["iters"])
    device = rank % max(da.device_count(), 1)
    out = {}
    count = [0]

    def greedy(ex, n, selected=0):
        cost, sel = [], []
        for _ in range(n):
            c2, g, bn, nxt = ex.iterate(selected)
            cost.append(c2)
            sel.append(selected)
            selected = nxt
        return cost, sel, selected

    def record(ex, Qhost, k):
        """certify_live, then the host path's collective entry on Qhost (rank 0's) at the same iterate"""
        i = count[0]
        count[0] += 1
        cert, th, lm, v, mv, dist, info = ex.certify_live(ETA)
        hcert, hth, hlm, hv, hmv, hdist = ex.certify(Qhost if rank == 0 else None, ETA, k)
        out.update({"c%d_ok" % i: cert, "c%d_theta" % i: th, "c%d_lambda" % i: lm, "c%d_v" % i: v, "c%d_matvecs" % i: mv,
                    "c%d_distributed" % i: dist, "c%d_info10" % i: info["info10"], "c%d_X" % i: ex.gather_X(),
                    "c%d_host_ok" % i: hcert, "c%d_host_theta" % i: hth, "c%d_host_lambda" % i: hlm,
                    "c%d_host_distributed" % i: hdist, "c%d_host_matvecs" % i: hmv})

    if scenario == "driver":
        ds = common.product_dataset(name)
        X0 = spec["X0"]
        for mode in ("host", "live"):
            res = driver.multi_robot_staircase_ranks(ds, X0, num_robots=R, r_min=r, r_max=r + 6, max_iters=iters,
                                                     rgrad_tol=float(spec["rgrad_tol"]), rank=rank, world_size=world,
                                                     device=device, job_name=job + mode, certificate=mode)
            out[mode + "_rank"] = res["rank"]
            out[mode + "_certified"] = res["certified"]
            out[mode + "_cost_2f"] = res["levels"][-1]["cost_2f"]
            out[mode + "_ranks"] = np.array([lev["rank"] for lev in res["levels"]])
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
        return

    if scenario.startswith("ra"):
        ra = da.RADataset(ra_path(name))
        k = ra.k
        s = da.RaRbcdSession(ra, r, acceleration=True, restart_interval=30, rank=rank, world_size=world, device=device)
        ex = da.Exchange(s, job)
        ex.set_X(spec["X0"])
        greedy(ex, iters)
        record(ex, ra.Q, k)
    else:
        ds = common.product_dataset(name)
        k = (ds.d + 1) * ds.n
        if scenario == "weights":
            ds = da.Dataset(ds.d, ds.n, spec["ids"], spec["vals"])
            s, ex = da.robust_ranked_session(ds, job, num_robots=R, r=r, robust=rb.RobustCostParameters("GNC_TLS", **GNC),
                                             rank=rank, world_size=world, device=device)
        else:
            s = da.RbcdSession(ds, num_robots=R, r=r, rank=rank, world_size=world, device=device)
            if scenario == "lift":
                s.reserve_rank(6)
            ex = da.Exchange(s, job)
        out["mode"] = ex.info()["mode"]
        ex.set_X(spec["X0"])
        Q = da.build_Q_pgo(ds)
        if scenario in ("refused", "accepted"):
            greedy(ex, iters)
            record(ex, Q, k)
        elif scenario == "weights":
            for w in (None, spec["w2"]):
                if w is not None:
                    ex.set_weights(w)
                now = ex.get_weights()
                out["w%d" % count[0]] = now
                with_w = da.Dataset(ds.d, ds.n, ds.ids.copy(), ds.vals.copy())
                with_w.vals[:, -1] = now
                record(ex, da.build_Q_pgo(with_w), k)
        elif scenario == "lift":
            greedy(ex, iters)
            record(ex, Q, k)
            escaped, _ = ex.lift(out["c0_theta"], out["c0_v"])
            out["escaped"], out["r_after"] = escaped, s.r
            record(ex, Q, k)
        elif scenario in ("alone", "alone_plain"):
            cost, sel, nxt = greedy(ex, 8)
            if scenario == "alone":
                a = ex.certify_live(ETA)
                b = ex.certify_live(ETA)
                out["same_bits"] = (a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])
                                    and a[4] == b[4] and a[5] == b[5] and a[6]["logdet"] == b[6]["logdet"]
                                    and a[6]["rounds"] == b[6]["rounds"])  # (the rest of info10 is times)
                out["refused"] = not a[0]
            c2, s2, _ = greedy(ex, 8, nxt)
            out.update(cost=np.array(cost + c2), selected=np.array(sel + s2), X=ex.gather_X())
        elif scenario == "usage":
            greedy(ex, iters)
            L = capi.lib()
            th = C.c_double()
            codes = [L.dcora_exchange_certify_live(ex.h, ETA, None, C.byref(th), None, None, None, None, None)]
            cert = C.c_int(7)
            codes.append(L.dcora_exchange_certify_live(ex.h, float("nan"), C.byref(cert), None, None, None, None, None,
                                                       None))
            codes.append(L.dcora_exchange_certify_live(ex.h, -1.0, C.byref(cert), None, None, None, None, None, None))
            out["codes"] = np.array(codes)
            c2, g, bn, nxt = ex.evaluate()  # the exchange keeps working
            out["finite_after"] = bool(np.isfinite(c2) and np.isfinite(g))
            record(ex, Q, k)
        elif scenario == "cache":
            greedy(ex, iters)
            da.chol_cache_clear()
            if rank == 0:
                da.cert_prepare(Q, ds.d, ds.n, block=ds.d + 1, device=device)
            record(ex, Q, k)
        else:
            raise SystemExit("unknown scenario " + scenario)
    ex.barrier()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    ex.close()
    s.close()


if __name__ == "__main__":
    main()
