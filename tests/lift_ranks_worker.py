"""one rank of a multi-rank RBCD job that climbs the staircase collectively (dcora_rbcd_reserve_rank /
dcora_ra_rbcd_reserve_rank, dcora_exchange_lift); started by tests/test_lift_ranks_gpu.py and by nothing else.
argv: rank world job dir.  dir holds job.json (what to run), X0.npy and, where the job lifts, v.npy; the rank writes
rank<k>.npz there.  job.json: kind "pgo" (name, R) or "ra" (path), r, reserve (0: none), mode and the mode's own keys."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def pgo_dataset(da, cfg):
    """the named fixture, or the one the test wrote (ids.npy / vals.npy: a fixture with injected outliers)"""
    import common
    ids = os.path.join(cfg["dir"], "ids.npy")
    if os.path.exists(ids):
        return da.Dataset(cfg["d"], cfg["n"], np.load(ids), np.load(os.path.join(cfg["dir"], "vals.npy")))
    return common.product_dataset(cfg["name"])


def open_job(da, cfg, rank, world, job, robust=None):
    """(session, exchange) of this rank: plain sessions reserve between their creation and their exchange's, robust
    ones through the reserved creators"""
    kw = dict(rank=rank, world_size=world, restart_interval=cfg.get("restart_interval", 30))
    if cfg["kind"] == "pgo":
        ds = pgo_dataset(da, cfg)
        if robust is not None:
            return da.robust_ranked_session(ds, job, num_robots=cfg["R"], r=cfg["r"], robust=robust,
                                            r_reserve=cfg["reserve"], **kw)
        s = da.RbcdSession(ds, num_robots=cfg["R"], r=cfg["r"], **kw)
    else:
        ra = da.RADataset(cfg["path"])
        if robust is not None:
            return da.ra_robust_ranked_session(ra, job, cfg["r"], robust=robust, r_reserve=cfg["reserve"], **kw)
        s = da.RaRbcdSession(ra, cfg["r"], **kw)
    if cfg["reserve"]:
        s.reserve_rank(cfg["reserve"])
    return s, da.Exchange(s, job)


def run_after(driver, s, ex, greedy, sweeps):
    """what the job does next: greedy iterations, then coloured sweeps with acceleration off"""
    out = {}
    g = driver.exchange_run(ex, max_iters=greedy, rgrad_tol=0.0)
    out.update(g_cost=g["cost"], g_gradnorm=g["gradnorm"], g_selected=g["selected"], X_greedy=ex.gather_X())
    if sweeps:
        s.set_acceleration(False)
        c = ex.run_coloured(max_sweeps=sweeps, rgrad_tol=0.0)
        out.update(c_cost=c["cost"], c_gradnorm=c["gradnorm"], X_sweeps=ex.gather_X())
    return out


def status_of(call):
    from dcora_amd import capi
    try:
        call()
        return 0
    except capi.DcoraError as e:
        return e.status


def main():
    rank, world, job, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import dcora_amd as da
    from dcora_amd import driver
    cfg = json.load(open(os.path.join(out_dir, "job.json")))
    cfg["dir"] = out_dir
    X0 = np.load(os.path.join(out_dir, "X0.npy"))
    v = np.load(os.path.join(out_dir, "v.npy")) if os.path.exists(os.path.join(out_dir, "v.npy")) else None
    mode, tol = cfg["mode"], cfg.get("tol", {})
    out = {}
    if mode == "staircase":
        fn = driver.multi_robot_staircase_ranks if cfg["kind"] == "pgo" else driver.raslam_staircase_ranks
        if cfg["kind"] == "pgo":
            res = fn(pgo_dataset(da, cfg), X0, rank=rank, world_size=world, job_name=job, **cfg["kw"])
        else:
            res = fn(da.RADataset(cfg["path"]), X0, rank=rank, world_size=world, job_name=job, **cfg["kw"])
        out = dict(X=res["X"], rank=res["rank"], certified=res["certified"],
                   ranks=np.array([lv["rank"] for lv in res["levels"]]),
                   escaped=np.array([bool(lv["escaped"]) for lv in res["levels"][:-1]]),
                   cost_2f=res["levels"][-1]["cost_2f"])
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
        return
    if mode == "robust":
        # a robust job with its team enabled, two collective weight updates, the job's own certificate, the lift, what
        # survived it, then the next rounds and the next update
        from dcora_amd import robust as rb
        s, ex = open_job(da, cfg, rank, world, job, robust=rb.RobustCostParameters("GNC_TLS", **cfg["gnc"]))
        (ex.enable_team if cfg["kind"] == "pgo" else ex.enable_team_ra)(max_num_iters=cfg["team_iters"])
        ex.set_X(X0)
        for _ in range(2):
            driver.exchange_run(ex, max_iters=5, rgrad_tol=0.0)
            ex.update_weights()
        w, rinfo, tinfo = ex.get_weights(), s.robust_info(), ex.team_info()
        lcs = [ex.loop_closure_stats(a) for a in range(s.R)]
        Xr = ex.gather_X()
        if cfg["kind"] == "pgo":
            ds = pgo_dataset(da, cfg)
            ds.vals[:, -1] = w
            Q = da.build_Q_pgo(ds) if rank == 0 else None
        else:
            ra = da.RADataset(cfg["path"])
            ra.set_pose_pose_weights(w)
            Q = ra.Q if rank == 0 else None
        cert, theta, lmin, vv, _, _ = ex.certify(Q, cfg["eta"], s.k)
        escaped, info = ex.lift(theta, vv, **tol)
        after_r, after_t = s.robust_info(), ex.team_info()
        out.update(cert=cert, theta=theta, v=vv, X_before=Xr, escaped=escaped, trials=info["trials"],
                   alpha=info["alpha"], r=s.r, X=ex.gather_X(), w_before=w, w_after=ex.get_weights(),
                   mu=np.array([rinfo["mu"], after_r["mu"]]), updates=np.array([rinfo["updates"], after_r["updates"]]),
                   team=np.array([[t["weight_updates"], t["resets"], t["inner_iter"]] for t in (tinfo, after_t)]),
                   params_kept=bool(ex.team.max_num_iters == cfg["team_iters"]),
                   lcs_kept=bool(lcs == [ex.loop_closure_stats(a) for a in range(s.R)]),
                   statuses_cleared=bool(all(ex.agent_status(a) is None for a in range(s.R))))
        g = driver.exchange_run(ex, max_iters=12, rgrad_tol=0.0)
        c = ex.update_weights()
        i = s.robust_info()
        out.update(g_cost=g["cost"], g_selected=g["selected"], X_run=ex.gather_X(), w_next=ex.get_weights(),
                   counts=np.array([c["accepted"], c["rejected"], c["undecided"]]), mu_next=i["mu"],
                   updates_next=i["updates"])
        ex.barrier()
        ex.close()
        s.close()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
        return
    launches_job0 = da.debug_launch_count()
    s, ex = open_job(da, cfg, rank, world, job)
    ex.set_X(X0)
    if cfg.get("pre"):  # a job in mid-flight: sequences, counters and a last solve to forget
        driver.exchange_run(ex, max_iters=cfg["pre"], rgrad_tol=0.0)
        if cfg.get("reset_after_pre", True):
            ex.set_X(X0)
    if mode == "lift":  # lift (or not: the twin / the fresh job), then go on
        if cfg.get("lift", True):
            launches0 = da.debug_launch_count()
            escaped, info = ex.lift(cfg["theta"], v, **tol)
            out.update(escaped=escaped, trials=info["trials"], alpha=info["alpha"], f_before=info["f_before"],
                       f_after=info["f_after"], lift_launches=da.debug_launch_count() - launches0)
        out.update(r=s.r, X=ex.gather_X())
        launches0 = da.debug_launch_count()
        out.update(run_after(driver, s, ex, cfg.get("greedy", 0), cfg.get("sweeps", 0)))
        out["launches"] = da.debug_launch_count() - launches0
        out["launches_job"] = da.debug_launch_count() - launches_job0  # creation, set_X and every run so far
    elif mode == "refusals":
        Xa = ex.gather_X()
        bad_v = v.copy()
        bad_v[7] = np.nan
        calls = [lambda: ex.lift(cfg["theta"], bad_v, **tol), lambda: ex.lift(np.nan, v, **tol),
                 lambda: ex.lift(cfg["theta"], v, gradient_tolerance=np.inf),
                 lambda: ex.lift(cfg["theta"], v, preconditioned_gradient_tolerance=np.nan),
                 lambda: ex.lift(cfg["theta"], None, **tol),
                 lambda: ex.lift(cfg["theta"], v, **tol),          # beyond the reserve (the job has none, or is at it)
                 lambda: s.reserve_rank(cfg["r"] + 1),              # an exchange exists
                 lambda: s.lift(cfg["theta"], v)]                   # the session's own entry keeps refusing
        out["status"] = np.array([status_of(c) for c in calls])
        out["unchanged"] = bool(np.array_equal(ex.gather_X(), Xa) and s.r == cfg["r"])
        out.update(run_after(driver, s, ex, cfg.get("greedy", 5), 0))
        out.update(r=s.r, X=ex.gather_X())
    ex.barrier()
    ex.close()
    s.close()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)


if __name__ == "__main__":
    main()
