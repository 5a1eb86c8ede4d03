"""one rank of a robust multi-rank range-aided RBCD job (dcora_ra_rbcd_create_robust_ranks, dcora_exchange_update_weights
/ _set_weights / _get_weights); started by tests/test_ra_gnc_ranks_gpu.py and by nothing else.  argv: rank world job
dir.  dir holds job.json (what to run, the pyfg file's path in it), X0.npy, and optionally w_file.npy (the pose-pose
weights the dataset starts with) / fixed.npy / X1.npy; the rank writes rank<k>.npz there."""
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
    load = lambda name: np.load(os.path.join(out_dir, name))
    ra = da.RADataset(cfg["path"])
    if cfg.get("w_file"):
        ra.set_pose_pose_weights(load("w_file.npy"))
    X0 = load("X0.npy")
    fixed = load("fixed.npy") if cfg.get("fixed") else None
    r, mode = cfg["r"], cfg["mode"]
    params = rb.RobustCostParameters(cfg["cost"], **cfg["robust"])
    out = {}
    if mode == "driver":
        res = driver.gnc_ra_ranks(ra, X0, r, robust=params, num_weight_updates=cfg["rounds"], inner_iters=cfg["inner"],
                                  rgrad_tol=cfg["rgrad_tol"], max_final_iters=cfg["final"], rank=rank,
                                  world_size=world, job_name=job)
        out = dict(X=res["X"], weights=res["weights"], ra_weights=ra.pose_pose_weights, cost=res["final"]["cost_2f"],
                   loop_closures=res["loop_closures"], rejected=np.array([q["rejected"] for q in res["rounds"]]))
    else:
        s, ex = da.ra_robust_ranked_session(ra, job, r, robust=params, fixed_weight=fixed, rank=rank, world_size=world,
                                            restart_interval=cfg.get("restart", 30))
        ex.set_X(X0)
        runs, counts, W, local, info = [], [], [], [], []
        run = lambda iters: runs.append(driver.exchange_run(ex, max_iters=iters, rgrad_tol=0.0))

        def update(**kw):
            c = ex.update_weights(**kw)
            counts.append([c["accepted"], c["rejected"], c["undecided"]])
            W.append(ex.get_weights())
            local.append(s.get_weights())
            i = s.robust_info()
            info.append([i["mu"], i["updates"]])

        out["W0"] = ex.get_weights()
        out["local0"] = s.get_weights()
        if mode == "compare":
            for _ in range(cfg["rounds"]):
                run(cfg["inner"])
                update()
            run(cfg["final"])
        elif mode == "refusals":
            run(5)
            w0, Xa = ex.get_weights(), ex.gather_X()
            bad = []
            for v in (np.nan, -0.5, np.inf):
                w = w0.copy()
                w[cfg["edge"]] = v
                bad.append(w)
            w = w0.copy()
            w[cfg["zero_edge"]] = 0.5
            bad.append(w)
            st, texts = [], []
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
                    texts.append(str(e))
            try:  # the team protocol stays refused on a range-aided exchange
                ex.enable_team()
                st.append(0)
            except capi.DcoraError as e:
                st.append(e.status)
            out["status"] = np.array(st)
            out["names_the_collective"] = all("dcora_exchange_" in t for t in texts) and len(texts) == 2
            out["unchanged"] = bool(np.array_equal(ex.get_weights(), w0) and np.array_equal(s.get_weights(),
                                                                                          out["local0"], equal_nan=True)
                                    and np.array_equal(ex.gather_X(), Xa))
            # the job goes on as if nothing had been tried
            run(6)
            update()
            run(5)
            out["X_after"] = ex.gather_X()
            # robustOptNumResets: every rank's X back to the last set_X
            X1 = load("X1.npy")
            ex.set_X(X1)
            driver.exchange_run(ex, max_iters=4, rgrad_tol=0.0)
            ex.update_weights(reset_to_initial=True)
            out["X_reset"] = ex.gather_X()
            out["updates"] = s.robust_info()["updates"]
        cat = lambda key: np.concatenate([q[key] for q in runs])
        out.update(counts=np.array(counts), W=np.array(W), local=np.array(local), info=np.array(info),
                   cost=cat("cost"), gradnorm=cat("gradnorm"), selected=cat("selected"), X=ex.gather_X(),
                   mode=ex.info()["mode"])
        ex.barrier()
        ex.close()
        s.close()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)


if __name__ == "__main__":
    main()
