"""one rank of a multi-rank RBCD job that projects to rank d collectively (dcora_exchange_project); started by
tests/test_project_ranks_gpu.py and by nothing else.
argv: rank world job dir.  dir holds job.json (what to run) and X0.npy; the rank writes rank<k>.npz there.  job.json:
kind "chain" (d, n, seed, R: sri.chain_dataset), "pgo" (name, R) or "ra" (path), r, mode and the mode's own keys."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from lift_ranks_worker import pgo_dataset, run_after  # noqa: E402

# ---- the chain cases of the rank tests, shared with tests/test_project_ranks_cpu.py: (d, n, agents, ranks).  Agent blocks
# just past one Gram chunk of 768 columns (800; 771, 771, 771, 777), and 9 poses on 3 and on 5 agents (with 4 ranks the
# last rank hosts nothing and the last agent holds 5 poses)
CHAIN_CASES = [(3, 800, 4, 2), (2, 1030, 4, 2), (3, 9, 3, 2), (2, 9, 5, 2), (2, 9, 5, 4)]
CHAIN_RANKS = [5, 16]
CHAIN_NU = 1e-3


def chain_cfg(d, n, R, r):
    import session_round_inputs as sri
    return dict(kind="chain", d=d, n=n, R=R, r=r, seed=sri.seed_of(d, r, n))


def chain_point(d, r, n, nu=CHAIN_NU):
    import session_project_inputs as spi
    return spi.lifted_point(d, r, n, spi.seed_of(d, r, n, nu), nu)


def reflect_chain_case(d, m):
    """spi.reflect_case's poses as a pose graph: (Xd d x (d + 1) n in the SE ordering, X = lift Xd at r = 5).  The
    rotation blocks (m of n = 9 improper) and the translations of the range-aided family, its unit spheres and
    landmarks dropped; the lift is recovered from the family's own X"""
    import session_project_inputs as spi
    n, l = spi.REFLECT_DIMS["n"], spi.REFLECT_DIMS["l"]
    Xd_ra, X_ra = spi.reflect_case(d, m)
    pick = np.concatenate([np.r_[d * i:d * i + d, d * n + l + i] for i in range(n)])
    return Xd_ra[:, pick].copy(), X_ra[:, pick].copy()


def dataset(da, cfg):
    if cfg["kind"] == "chain":
        import session_round_inputs as sri
        return sri.chain_dataset(da.Dataset, cfg["d"], cfg["n"], cfg["seed"])
    if cfg["kind"] == "pgo":
        return pgo_dataset(da, cfg)
    return da.RADataset(cfg["path"])


def open_job(da, cfg, r, rank, world, job, robust=None):
    kw = dict(rank=rank, world_size=world, restart_interval=cfg.get("restart_interval", 30))
    data = dataset(da, cfg)
    if cfg["kind"] == "ra":
        if robust is not None:
            return da.ra_robust_ranked_session(data, job, r, robust=robust, **kw)
        s = da.RaRbcdSession(data, r, **kw)
    else:
        if robust is not None:
            return da.robust_ranked_session(data, job, num_robots=cfg["R"], r=r, robust=robust, **kw)
        s = da.RbcdSession(data, num_robots=cfg["R"], r=r, **kw)
    return s, da.Exchange(s, job)


def project_facts(out):
    basis = out["basis"] if out["basis"] is not None else np.zeros((0, 0))
    return dict(projected=out["projected"], reflected=out["reflected"], positive_dets=out["positive_dets"],
                sigma=out["sigma"], basis=basis, gram=out["gram"], cost_2f=out["cost_2f"], gradnorm=out["gradnorm"],
                gram_chunk=out["gram_chunk"])


def robust_mode(da, driver, cfg, rank, world, job, X0, out):
    """a robust job with its team enabled, two collective weight updates, the projection, what survived it, the next
    rounds and the next update; then the certificate of the matrices the ranks hold, and a lift from rank d.
    fresh: the rank-d job that made two updates of its own and was handed the weights (w.npy) and the point (X0)"""
    from dcora_amd import robust as rb
    params = rb.RobustCostParameters("GNC_TLS", **cfg["gnc"])
    fresh = cfg.get("fresh", False)
    s, ex = open_job(da, cfg, cfg["r"], rank, world, job, robust=params)
    (ex.enable_team if cfg["kind"] != "ra" else ex.enable_team_ra)(max_num_iters=cfg["team_iters"])
    ex.set_X(X0)
    if fresh:
        ex.update_weights()
        ex.update_weights()
        ex.set_weights(np.load(os.path.join(cfg["dir"], "w.npy")))
        ex.set_X(X0)
    else:
        for _ in range(2):
            driver.exchange_run(ex, max_iters=5, rgrad_tol=0.0)
            ex.update_weights()
    w, rinfo, tinfo = ex.get_weights(), s.robust_info(), ex.team_info()
    lcs = [ex.loop_closure_stats(a) for a in range(s.R)]
    if not fresh:
        out["X_before"] = ex.gather_X()
        out.update(project_facts(ex.project()))
    after_r, after_t = s.robust_info(), ex.team_info()
    out.update(r=s.r, X=ex.gather_X(), w_before=w, w_after=ex.get_weights(),
               mu=np.array([rinfo["mu"], after_r["mu"]]), updates=np.array([rinfo["updates"], after_r["updates"]]),
               team=np.array([[t["weight_updates"], t["resets"], t["inner_iter"]] for t in (tinfo, after_t)]),
               params_kept=bool(ex.team.max_num_iters == cfg["team_iters"]),
               lcs=np.array([[q["accepted"], q["rejected"], q["total"]] for q in lcs]).ravel(), lcs_kept=bool(lcs == [ex.loop_closure_stats(a) for a in range(s.R)]),
               statuses_cleared=bool(all(ex.agent_status(a) is None for a in range(s.R))))
    g = driver.exchange_run(ex, max_iters=12, rgrad_tol=0.0)
    out.update(g_cost=g["cost"], g_selected=g["selected"], X_run=ex.gather_X())
    if "X_sync" in cfg:  # (a weight of exactly 0: the third update starts from one point on both sides)
        ex.set_X(np.load(os.path.join(cfg["dir"], cfg["X_sync"])))
    c = ex.update_weights()
    i = s.robust_info()
    out.update(w_next=ex.get_weights(), counts=np.array([c["accepted"], c["rejected"], c["undecided"]]),
               mu_next=i["mu"], updates_next=i["updates"])
    cert, theta, lmin, v, _, _, _ = ex.certify_live(cfg["eta"])
    out.update(cert=cert, theta=theta, v=v)
    if not fresh and not cert:
        escaped, _ = ex.lift(theta, v, **cfg.get("tol", {}))
        out.update(lift_escaped=escaped, r_lifted=s.r)
    ex.barrier()
    ex.close()
    s.close()


def main():
    rank, world, job, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import dcora_amd as da
    from dcora_amd import capi, driver
    cfg = json.load(open(os.path.join(out_dir, "job.json")))
    cfg["dir"] = out_dir
    X0 = np.load(os.path.join(out_dir, "X0.npy"))
    mode = cfg["mode"]
    out = {}
    if mode == "staircase":
        name = ("raslam_staircase_ranks" if cfg["kind"] == "ra" else "multi_robot_staircase_ranks") + \
            ("_projected" if cfg.get("projected") else "")
        fn = getattr(driver, name)
        res = fn(dataset(da, cfg), X0, rank=rank, world_size=world, job_name=job, **cfg["kw"])
        out = {key: val for key, val in res.items() if key != "levels" and val is not None}
        out["keys"] = np.array(sorted(res))
        out["none_keys"] = np.array(sorted(key for key, val in res.items() if val is None) + [""])
        out["level_costs"] = np.array([lv["cost_2f"] for lv in res["levels"]])
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
        return
    if mode == "robust":
        robust_mode(da, driver, cfg, rank, world, job, X0, out)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
        return
    if mode == "reflect":  # one job per member of the reflect family: X0 holds the points one after another
        import session_project_inputs as spi
        r = spi.REFLECT_DIMS["r"]
        for i in range(X0.shape[0] // r):
            s, ex = open_job(da, cfg, r, rank, world, "%s_%d" % (job, i))
            ex.set_X(X0[i * r:(i + 1) * r])
            pr = ex.project()
            out.update({"%s_%d" % (key, i): val for key, val in project_facts(pr).items()})
            out["X_%d" % i] = ex.gather_X()
            ex.barrier()
            ex.close()
            s.close()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
        return
    # mode "project": a job, in mid-flight where asked, projects (or not: the twin / the fresh job), then goes on
    launches_job0 = da.debug_launch_count()
    if cfg.get("sums"):
        capi.check(capi.lib().dcora_debug_exchange_project_sums(1))
    s, ex = open_job(da, cfg, cfg["r"], rank, world, job)
    ex.set_X(X0)
    if cfg.get("pre"):
        driver.exchange_run(ex, max_iters=cfg["pre"], rgrad_tol=0.0)
    if cfg.get("null_call"):  # a refused call: no handle
        out["null_status"] = capi.lib().dcora_exchange_project(None, None, None, None, None, None)
    if cfg.get("project", True):
        out["X_before"] = ex.gather_X()
        out.update(project_facts(ex.project()))
        out["eval_after"] = ex.evaluate()[0]
    elif cfg.get("evaluate"):
        out["eval_after"] = ex.evaluate()[0]
    out.update(r=s.r, X=ex.gather_X())
    launches0 = da.debug_launch_count()
    if cfg.get("greedy"):
        out.update(run_after(driver, s, ex, cfg["greedy"], cfg.get("sweeps", 0)))
    out["launches"] = da.debug_launch_count() - launches0
    out["launches_job"] = da.debug_launch_count() - launches_job0
    ex.barrier()
    ex.close()
    s.close()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)


if __name__ == "__main__":
    main()
