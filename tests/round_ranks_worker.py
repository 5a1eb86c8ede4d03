"""one rank of a multi-rank RBCD job that rounds collectively (dcora_exchange_round); started by
tests/test_round_ranks_gpu.py and by nothing else.  argv: rank world job dir.  dir holds job.json and X0.npy; the rank
writes rank<k>.npz there.  job.json: kind "pgo" (name, R) or "ra" (path), r, pre (greedy iterations after set_X),
round (false: the twin that never rounds), greedy (iterations afterwards)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def status_of(call):
    from dcora_amd import capi
    try:
        call()
        return 0
    except capi.DcoraError as e:
        return e.status


def main():
    rank, world, job, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import common
    import dcora_amd as da
    import session_round_inputs as sri
    from dcora_amd import capi, driver
    cfg = json.load(open(os.path.join(out_dir, "job.json")))
    X0 = np.load(os.path.join(out_dir, "X0.npy"))
    kw = dict(rank=rank, world_size=world)
    if cfg["kind"] == "pgo":
        ds = common.product_dataset(cfg["name"])
        d, n = ds.d, ds.n
        s = da.RbcdSession(ds, num_robots=cfg["R"], r=cfg["r"], **kw)
        X0se = X0
    else:
        ra = da.RADataset(cfg["path"])
        d, n = ra.d, ra.n
        s = da.RaRbcdSession(ra, cfg["r"], **kw)
        X0se = sri.se_from_ra(X0, d, n, ra.l)
    launches0 = da.debug_launch_count()
    ex = da.Exchange(s, job)
    ex.set_X(X0)
    driver.exchange_run(ex, max_iters=cfg["pre"], rgrad_tol=0.0)
    out = {}
    if cfg.get("round", True):
        explicit = sri.anchor_of(X0se, d, 1 % n)
        for label, call in (("first", lambda: ex.round()), ("last", lambda: ex.round(anchor_pose=n - 1)),
                            ("explicit", lambda: ex.round(anchor=explicit)), ("again", lambda: ex.round())):
            res = call()
            for key, val in res.items():
                out["%s_%s" % (label, key)] = val
        bad = explicit.copy()
        bad[0, d] = np.nan
        calls = [lambda: ex.round(anchor_pose=-1), lambda: ex.round(anchor_pose=n), lambda: ex.round(anchor=bad),
                 lambda: capi.check(capi.lib().dcora_exchange_round(ex.h, 0, None, None, None, None)),
                 lambda: s.round()]  # the session's own entry refuses a rank of a job
        out["status"] = np.array([status_of(c) for c in calls])
    out["X"] = ex.gather_X()
    g = driver.exchange_run(ex, max_iters=cfg.get("greedy", 5), rgrad_tol=0.0)
    out.update(g_cost=g["cost"], g_gradnorm=g["gradnorm"], g_selected=g["selected"], X_greedy=ex.gather_X(),
               launches=da.debug_launch_count() - launches0)
    ex.barrier()
    ex.close()
    s.close()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)


if __name__ == "__main__":
    main()
