"""one rank of a multi-rank RBCD job that runs the team protocol through its exchange (dcora_exchange_team_enable and the
entries around it); started by tests/test_team_ranks_gpu.py, which also borrows the recording helpers for its
single-process references.  argv: rank world job dir.  dir holds job.json (what to run), ids.npy / vals.npy (the
dataset), X0.npy; the rank writes rank<k>.npz there."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

STOP = {"all_ready": 1, "max_iters": 2}


def statuses(t, R):
    """every agent's status of a session or an exchange as rows of (known, agent_id, state, instance_number,
    iteration_number, ready_to_terminate, relative_change); an unknown one is a row of zeros"""
    out = np.zeros((R, 7))
    for q in range(R):
        st = t.agent_status(q)
        if st is not None:
            out[q] = [1, st["agent_id"], st["state"], st["instance_number"], st["iteration_number"],
                      int(st["ready_to_terminate"]), st["relative_change"]]
    return out


def team_view(t, R):
    i = t.team_info()
    return dict(status=statuses(t, R), decide=np.array([int(t.should_terminate()), int(t.should_update_weights())]),
                info=np.array([i["inner_iter"], i["latest_weight_update_iteration"], i["weight_updates"], i["resets"]]),
                lc=np.array([[c["accepted"], c["rejected"], c["total"]]
                             for c in (t.loop_closure_stats(q) for q in range(R))]))


def stack(views):
    return {k: np.array([v[k] for v in views]) for k in views[0]}


def greedy_rounds(it, team, R, rounds):
    """`rounds` greedy rounds through it.iterate (a session or an exchange), the team's view (of `team`, or None)
    recorded after every round"""
    cost, gn, sel, views = [], [], [], []
    selected = 0
    for _ in range(rounds):
        c2, g, _, nxt = it.iterate(selected)
        cost.append(c2), gn.append(g), sel.append(selected)
        if team is not None:
            views.append(team_view(team, R))
        selected = nxt
    out = dict(cost=np.array(cost), gradnorm=np.array(gn), selected=np.array(sel))
    if views:
        out.update(stack(views))
    return out


def tick_sweeps(s, tick, team, R, sweeps):
    """`sweeps` sweeps of one tick per colour (tick: the session's iterate_set or the exchange's tick), the team's view
    after every tick"""
    col, nc = s.colours()
    views = []
    for _ in range(sweeps):
        for c in range(nc):
            tick(np.nonzero(col == c)[0])
            views.append(team_view(team, R))
    return dict(stack(views), colours=np.asarray(col))


def run_team_record(t, R, get_weights, get_X):
    out = t.run_team()
    rec = dict(iters=out["iters"], cost=out["cost"], gradnorm=out["gradnorm"], selected=out["selected"],
               updated=out["updated"], weight_updates=out["weight_updates"], stop=STOP[out["stop_reason"]])
    rec.update({"final_" + k: v for k, v in team_view(t, R).items()})
    rec.update(W=get_weights(), X=get_X())
    return rec


def main():
    rank, world, job, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import dcora_amd as da
    from dcora_amd import capi, driver
    from dcora_amd import robust as rb
    cfg = json.load(open(os.path.join(out_dir, "job.json")))
    ds = da.Dataset(cfg["d"], cfg["n"], np.load(os.path.join(out_dir, "ids.npy")), np.load(os.path.join(out_dir, "vals.npy")))
    X0 = np.load(os.path.join(out_dir, "X0.npy"))
    R, r, mode = cfg["R"], cfg["r"], cfg["mode"]
    team = cfg.get("team", {})
    out = {}
    if mode == "driver":
        res = driver.multi_robot_team_ranks(ds, X0, num_robots=R, r=r, robust=rb.RobustCostParameters("GNC_TLS", **cfg["gnc"]),
                                            team=da.team_params(**team), rank=rank, world_size=world, job_name=job)
        out = dict(X=res["X"], weights=res["weights"], ds_weights=ds.vals[:, -1], iters=res["final"]["iterations"],
                   weight_updates=res["final"]["weight_updates"], stop=STOP[res["final"]["stop_reason"]],
                   ready=np.array([bool(st and st["ready_to_terminate"]) for st in res["statuses"]]))
    else:
        if "gnc" in cfg:
            s, ex = da.robust_ranked_session(ds, job, num_robots=R, r=r, robust=rb.RobustCostParameters("GNC_TLS", **cfg["gnc"]),
                                             rank=rank, world_size=world)
        else:
            s = da.RbcdSession(ds, num_robots=R, r=r, rank=rank, world_size=world, acceleration=cfg.get("accel", True))
            ex = da.Exchange(s, job)
        if mode == "refusals":
            ex.team = da.team_params()
            st = []
            for call in (lambda: ex.agent_status(0), lambda: ex.loop_closure_stats(0), ex.should_terminate,
                         ex.should_update_weights, ex.team_info, ex.run_team):
                try:
                    call()
                    st.append(0)
                except capi.DcoraError as e:
                    st.append(e.status)
            ex.set_X(X0)
            out.update(greedy_rounds(ex, None, R, cfg["rounds"]))  # the job iterates as if nothing had been tried
            ex.enable_team()
            try:
                ex.agent_status(R)
                st.append(0)
            except capi.DcoraError as e:
                st.append(e.status)
            out.update(greedy_rounds(ex, ex, R, 2))  # ... and the team works once enabled
            out["refused"] = np.array(st)
        else:
            if cfg.get("enable", True):
                ex.enable_team(**team)
            ex.set_X(X0)
            if mode == "greedy":
                out = greedy_rounds(ex, ex if cfg.get("enable", True) else None, R, cfg["rounds"])
                out["launches"] = s.debug_launches()
            elif mode == "ticks":
                out = tick_sweeps(s, ex.tick, ex, R, cfg["sweeps"])
            elif mode == "run_team":
                out = run_team_record(ex, R, ex.get_weights, ex.gather_X)
        out["X"] = ex.gather_X()
        ex.barrier()
        ex.close()
        s.close()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)


if __name__ == "__main__":
    main()
