"""one rank of a multi-rank range-aided RBCD job that runs the team protocol through its exchange
(dcora_exchange_team_enable_ra and the entries around it on an exchange of dcora_exchange_create_ra or of
dcora_ra_rbcd_create_robust_ranks); started by tests/test_ra_team_ranks_gpu.py and by nothing else.  The recording
helpers are those of tests/team_ranks_worker.py: they ask a session and an exchange the same questions.  argv: rank
world job dir.  dir holds job.json (what to run, the pyfg file's path in it) and X0.npy; the rank writes rank<k>.npz
there."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import team_ranks_worker as tw  # noqa: E402


def rounds_with_launches(da, ex, team, R, rounds, count=False, gather=False):
    """tw.greedy_rounds through the exchange; if asked, with the process's launch counter around every round and with
    the gathered X after every round"""
    cost, gn, sel, views, launches, Xs = [], [], [], [], [], []
    selected = 0
    for _ in range(rounds):
        n0 = da.debug_launch_count() if count else 0
        c2, g, _, nxt = ex.iterate(selected)
        launches.append(da.debug_launch_count() - n0 if count else 0)
        cost.append(c2), gn.append(g), sel.append(selected)
        if team is not None:
            views.append(tw.team_view(team, R))
        if gather:
            Xs.append(ex.gather_X())
        selected = nxt
    out = dict(cost=np.array(cost), gradnorm=np.array(gn), selected=np.array(sel), launches=np.array(launches))
    if views:
        out.update(tw.stack(views))
    if gather:
        out["Xs"] = np.array(Xs)
    return out


def status_of(call, capi):
    try:
        call()
        return 0
    except capi.DcoraError as e:
        return e.status


def main():
    rank, world, job, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import dcora_amd as da
    from dcora_amd import capi, driver
    from dcora_amd import robust as rb
    cfg = json.load(open(os.path.join(out_dir, "job.json")))
    ra = da.RADataset(cfg["path"])
    X0 = np.load(os.path.join(out_dir, "X0.npy"))
    r, mode = cfg["r"], cfg["mode"]
    team = cfg.get("team", {})
    params = rb.RobustCostParameters("GNC_TLS", **cfg["gnc"]) if "gnc" in cfg else None
    out = {}
    if mode == "driver":
        res = driver.ra_team_ranks(ra, X0, r, robust=params, team=da.team_params(**team), rank=rank, world_size=world,
                                   job_name=job)
        out = dict(X=res["X"], weights=res["weights"], ra_weights=ra.pose_pose_weights, loop_closures=res["loop_closures"],
                   iters=res["final"]["iterations"], weight_updates=res["final"]["weight_updates"],
                   stop=tw.STOP[res["final"]["stop_reason"]], selected=res["run"]["selected"], updated=res["run"]["updated"],
                   ready=np.array([bool(st and st["ready_to_terminate"]) for st in res["statuses"]]),
                   lc=np.array([[c["accepted"], c["rejected"], c["total"]] for c in res["loop_closure_stats"]]))
    else:
        if params is not None:
            s, ex = da.ra_robust_ranked_session(ra, job, r, robust=params, rank=rank, world_size=world)
        else:
            s = da.RaRbcdSession(ra, r, rank=rank, world_size=world, acceleration=cfg.get("accel", True))
            ex = da.Exchange(s, job)
        R = s.R
        if mode == "refusals":
            st = []
            # the session's own entry on a rank of a job points to the exchange
            try:
                s.enable_team()
                st.append(0)
            except capi.DcoraError as e:
                st.append(e.status if "dcora_exchange_team_enable" in str(e) else -1)
            # a robust ranked session with an exchange that was not created for it (no weights area)
            other = da.Exchange(s, job + "x")
            st.append(status_of(other.enable_team_ra, capi))
            other.set_X(X0)
            st.append(status_of(lambda: other.iterate(0), capi))  # ... which stays usable
            other.barrier()
            other.close()
            ex.set_X(X0)
            out.update(tw.greedy_rounds(ex, None, R, cfg["rounds"]))  # the job iterates as if nothing had been tried
            ex.enable_team_ra(**team)
            more = tw.greedy_rounds(ex, ex, R, 2)  # ... and the team works once enabled
            out.update({"more_" + k: v for k, v in more.items()})
            out["refused"] = np.array(st)
        else:
            enabled = cfg.get("enable", True)
            if enabled:
                ex.enable_team_ra(**team)
            ex.set_X(X0)
            if mode == "greedy":
                out = rounds_with_launches(da, ex, ex if enabled else None, R, cfg["rounds"], cfg.get("count", False),
                                           cfg.get("gather", False))
            elif mode == "ticks":
                out = tw.tick_sweeps(s, ex.tick, ex, R, cfg["sweeps"])
            elif mode == "run_team":
                out = tw.run_team_record(ex, R, ex.get_weights, ex.gather_X)
        out["X"] = ex.gather_X()
        out["hosted"] = np.array([q for q in range(R) if q // ((R + world - 1) // world) == rank], np.int32)
        out["transport"] = ex.info()["mode"]
        ex.barrier()
        ex.close()
        s.close()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)


if __name__ == "__main__":
    main()
