"""one rank of a robust multi-rank RBCD job (dcora_rbcd_create_robust_ranks, dcora_exchange_update_weights / _set_weights
/ _get_weights); started by tests/test_gnc_ranks_gpu.py and by nothing else.  argv: rank world job dir.  dir holds
job.json (what to run), ids.npy / vals.npy (the dataset with its outliers), X0.npy, and optionally fixed.npy / X1.npy;
the rank writes rank<k>.npz there."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    rank, world, job, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import dcora_amd as da
    from dcora_amd import capi, driver
    from dcora_amd import robust as rb
    cfg = json.load(open(os.path.join(out_dir, "job.json")))
    ds = da.Dataset(cfg["d"], cfg["n"], np.load(os.path.join(out_dir, "ids.npy")), np.load(os.path.join(out_dir, "vals.npy")))
    X0 = np.load(os.path.join(out_dir, "X0.npy"))
    fixed = np.load(os.path.join(out_dir, "fixed.npy")) if cfg.get("fixed") else None
    R, r, mode = cfg["R"], cfg["r"], cfg["mode"]
    params = rb.RobustCostParameters("GNC_TLS", **cfg["gnc"])
    out = {}
    if mode == "driver":
        res = driver.multi_robot_gnc_ranks(ds, X0, num_robots=R, r=r, robust=params,
                                           num_weight_updates=cfg["rounds"], inner_iters=cfg["inner"],
                                           rgrad_tol=cfg["rgrad_tol"], max_final_iters=cfg["final"], rank=rank,
                                           world_size=world, job_name=job)
        out = dict(X=res["X"], weights=res["weights"], ds_weights=ds.vals[:, -1],
                   cost=res["final"]["cost_2f"], rejected=np.array([q["rejected"] for q in res["rounds"]]))
    else:
        s, ex = da.robust_ranked_session(ds, job, num_robots=R, r=r, robust=params, fixed_weight=fixed, rank=rank,
                                         world_size=world)
        ex.set_X(X0)
        runs, counts, W, local, info = [], [], [], [], []
        if mode == "compare":
            out["W0"] = ex.get_weights()
            out["local0"] = s.get_weights()
            for _ in range(cfg["rounds"]):
                runs.append(driver.exchange_run(ex, max_iters=cfg["inner"], rgrad_tol=0.0))
                c = ex.update_weights()
                counts.append([c["accepted"], c["rejected"], c["undecided"]])
                W.append(ex.get_weights())
                local.append(s.get_weights())
                i = s.robust_info()
                info.append([i["mu"], i["updates"]])
            runs.append(driver.exchange_run(ex, max_iters=cfg["final"], rgrad_tol=0.0))
        elif mode == "refusals":
            runs.append(driver.exchange_run(ex, max_iters=7, rgrad_tol=0.0))
            w0, Xa = ex.get_weights(), ex.gather_X()
            bad = []
            for v in (np.nan, -0.5, np.inf):
                w = w0.copy()
                w[cfg["edge"]] = v
                bad.append(w)
            w = w0.copy()
            w[cfg["zero_edge"]] = 0.5
            bad.append(w)
            st = []
            for w in bad:
                try:
                    ex.set_weights(w)
                    st.append(0)
                except capi.DcoraError as e:
                    st.append(e.status)
            for call in (lambda: s.update_weights(), lambda: s.set_weights(w0)):
                try:
                    call()
                    st.append(0)
                except capi.DcoraError as e:
                    st.append(e.status)
            out["status"] = np.array(st)
            out["unchanged"] = bool(np.array_equal(ex.get_weights(), w0, equal_nan=True) and
                                    np.array_equal(ex.gather_X(), Xa))
            # the job goes on as if nothing had been tried
            runs.append(driver.exchange_run(ex, max_iters=12, rgrad_tol=0.0))
            c = ex.update_weights()
            counts.append([c["accepted"], c["rejected"], c["undecided"]])
            W.append(ex.get_weights())
            runs.append(driver.exchange_run(ex, max_iters=5, rgrad_tol=0.0))
            out["X_after"] = ex.gather_X()
            # robustOptNumResets: every rank's X back to the last set_X
            X1 = np.load(os.path.join(out_dir, "X1.npy"))
            ex.set_X(X1)
            driver.exchange_run(ex, max_iters=6, rgrad_tol=0.0)
            ex.update_weights(reset_to_initial=True)
            out["X_reset"] = ex.gather_X()
            i = s.robust_info()
            info.append([i["mu"], i["updates"]])
        out.update(counts=np.array(counts), W=np.array(W), local=np.array(local), info=np.array(info),
                   cost=np.concatenate([q["cost"] for q in runs]),
                   gradnorm=np.concatenate([q["gradnorm"] for q in runs]),
                   selected=np.concatenate([q["selected"] for q in runs]), X=ex.gather_X())
        ex.barrier()
        ex.close()
        s.close()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)


if __name__ == "__main__":
    main()
