"""The synchronous multi-robot driver of the reference (examples/MultiRobotExample.cpp:121-372) over the C ABI:

    for r = r_min, r_min + 1, ...:
        agents at rank r, X = current point                       (:172-217)
        RBCD++ until |rgrad| < tol or max_iters                   (:223-307)   dcora_rbcd_run
            (mode="coloured": sweeps of simultaneous updates, one tick per colour of the agent graph, non-accelerated --
             the agents that fire together of src/Agent.cpp:650-678 as a schedule --      dcora_rbcd_run_coloured)
        S = Q - Lambda(X);  fastVerification(S, min_eig_tol)      (:320-334)   dcora_cert_*
        certified: done;  else escapeSaddle into rank r + 1       (:352-366)   dcora_problem_escape_saddle

Everything numerical runs on the device; this file is the control flow of the example program."""
import sys
import threading
import time

import numpy as np

from . import (QuadraticProblem, RbcdSession, build_Q_pgo, cert_prepare, dual_certificate, fast_verification,
               lambda_min_certified, suboptimality_gap)


def multi_robot_example(ds, X0, num_robots=5, r_min=5, r_max=100, max_iters=1000, rgrad_tol=0.1, min_eig_tol=1e-3,
                        gradient_tolerance=1e-6, preconditioned_gradient_tolerance=1e-6, acceleration=True,
                        params=None, device=0, refine_gap=False, mode="rbcd++"):
    """X0: r_min x (d+1) n start point.  Returns a dict: X (final rank x k), rank, certified, theta, per-level
    records (rank, iterations, cost 2f, gradnorm, seconds of RBCD / certification / escape, mode) and the traces.
    mode: "rbcd++" (the reference driver's greedy accelerated passes) or "coloured" (each level runs run_coloured on a
    non-accelerated session: `iterations` counts sweeps, max_iters caps them, `selected` holds -1)."""
    _check_mode(mode)
    d, n = ds.d, ds.n
    k = (d + 1) * n
    Q = build_Q_pgo(ds)
    X = np.asarray(X0, dtype=np.float64)
    if X.shape != (r_min, k):
        raise ValueError("X0 must be r_min x (d+1) n")
    levels, cost, gradnorm, selected, rank = [], [], [], [], []
    certified, theta, total = False, 0.0, 0
    r = r_min
    prep = None
    while r < r_max:
        ts = time.perf_counter()
        if prep is None:
            # the certificate S = Q - Lambda has Q's pattern: its PSD test is analysed (ordering, fronts, device image)
            # on another host thread while the agents iterate -- inside the clock of the first level, like the agents'
            # own set-up; the reference analyses inside isSparseSymmetricMatrixPSD, after the loop
            prep = threading.Thread(target=cert_prepare, args=(Q, d, n), kwargs=dict(block=d + 1, device=device),
                                    daemon=True)
            prep.start()
        s = RbcdSession(ds, num_robots=num_robots, r=r, acceleration=acceleration and mode == "rbcd++", params=params,
                        device=device)
        s.set_X(X)
        t0 = time.perf_counter()
        out = _run_level(s, mode, max_iters, rgrad_tol)
        t1 = time.perf_counter()
        Xopt = s.get_X()
        total += out["iters"]
        cost.append(out["cost"])
        gradnorm.append(out["gradnorm"])
        selected.append(out["selected"])
        rank.append(np.full(out["iters"], r, np.int32))
        S = dual_certificate(r, d, n, Xopt, Q, device=device)
        prep.join()
        psd, theta, v, lmin = fast_verification(S, min_eig_tol, block=d + 1, device=device)
        t2 = time.perf_counter()
        s.close()  # (the agents live through the certification, as in the reference's driver)
        lev = {"rank": r, "iterations": int(out["iters"]), "cost_2f": float(out["cost"][-1]),
               "gradnorm": float(out["gradnorm"][-1]), "setup_s": t0 - ts, "rbcd_s": t1 - t0,
               "certification_s": t2 - t1,
               "certified": bool(psd), "theta": float(theta), "mode": mode}
        # bound on f(X) - f* implied by the certificate (this library's addition, include/dcora_hip.h)
        lev["suboptimality_gap_f"], lev["n_eff"] = suboptimality_gap(r, d, n, Xopt, psd, min_eig_tol, lmin)
        if psd and refine_gap:  # a verified lower bound of lambda_min(S) instead of the -eta the test guarantees
            tg = time.perf_counter()
            lam, _ = lambda_min_certified(S, min_eig_tol, block=d + 1)
            lev["lambda_min_S"] = lam
            lev["suboptimality_gap_f_refined"] = suboptimality_gap(r, d, n, Xopt, psd, min_eig_tol,
                                                                   lambda_bound=min(lam, 0.0))[0]
            lev["gap_refinement_s"] = time.perf_counter() - tg
        levels.append(lev)
        X = Xopt
        if psd:
            certified = True
            break
        if theta >= -min_eig_tol / 2:  # :333-335: the eigenvalue computation did not reach the precision to escape
            raise RuntimeError("escape direction computation did not converge to the desired precision")
        Pn = QuadraticProblem(r + 1, d, n, Q, device=device)
        Xn = Pn.escapeSaddle(Xopt, theta, v, gradient_tolerance, preconditioned_gradient_tolerance)
        Pn.close()
        lev["escape_s"] = time.perf_counter() - t2
        if Xn is None:  # :367-370: no descent found along the escape direction
            lev["escaped"] = False
            break
        lev["escaped"] = True
        X = Xn
        r += 1
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)
    return {"X": X, "rank": X.shape[0], "certified": certified, "theta": float(theta), "total_iters": int(total),
            "suboptimality_gap_f": levels[-1]["suboptimality_gap_f"] if levels else None, "levels": levels, "cost": cat(cost, float), "gradnorm": cat(gradnorm, float),
            "selected": cat(selected, np.int32), "rank_trace": cat(rank, np.int32)}


def _staircase_session(s, X0, k, r_min, r_max, max_iters, rgrad_tol, min_eig_tol, gradient_tolerance,
                       preconditioned_gradient_tolerance, mode, ts, gap=None, before_certify=None,
                       round_on_device=False, project_on_device=False):
    """The staircase of the two drivers above in ONE session of either kind: each level is run / run_coloured, certify
    (the session's own, on the device) and lift (the escape into the next rank in place) -- the reference makes a new
    set of agents per level (examples/MultiRobotExample.cpp:352-366), this keeps them.  The level records are the
    existing drivers'; the iterate comes to the host once, after the last level (gap(X, psd, lmin) -> the bound of
    that level's record; the earlier levels carry None).
    round_on_device: the solve's last step on the device too -- s.round(cost=True) before the session closes: the result
    also carries trajectory (unit_spheres and landmarks on a range-aided session), rounded_cost_2f and rounded_gradnorm
    (None on a multi-rank job, where no rank holds the whole problem), in the frame of pose 0 of the final iterate.
    project_on_device: how CORA ends a certified solve (ref examples/SingleRobotExample_RASLAM.cpp:220-234), on the
    session too -- after a certified level s.project() takes the session to rank d in place, the level's own run
    parameters refine the point there, and round_on_device then rounds the refined point.  The result also carries
    sigma (the singular values of the certified X), projected_cost_2f, refined_cost_2f and refine_iters (None where no
    level was certified); every other key is what it is without the option."""
    X = np.asarray(X0, dtype=np.float64)
    if X.shape != (r_min, k):
        raise ValueError("X0 must be r_min x k")
    levels, cost, gradnorm, selected, rank = [], [], [], [], []
    certified, theta, total = False, 0.0, 0
    try:
        s.set_X(X)
        while s.r < r_max:
            r = s.r
            t0 = time.perf_counter()
            out = _run_level(s, mode, max_iters, rgrad_tol)
            t1 = time.perf_counter()
            total += out["iters"]
            cost.append(out["cost"])
            gradnorm.append(out["gradnorm"])
            selected.append(out["selected"])
            rank.append(np.full(out["iters"], r, np.int32))
            if before_certify is not None:
                before_certify()
            psd, theta, v, lmin, _ = s.certify(min_eig_tol)
            t2 = time.perf_counter()
            lev = {"rank": r, "iterations": int(out["iters"]), "cost_2f": float(out["cost"][-1]),
                   "gradnorm": float(out["gradnorm"][-1]), "setup_s": t0 - ts, "rbcd_s": t1 - t0,
                   "certification_s": t2 - t1, "certified": bool(psd), "theta": float(theta), "mode": mode,
                   "suboptimality_gap_f": None, "n_eff": None, "lambda_min": float(lmin)}
            levels.append(lev)
            if psd:
                certified = True
                break
            if theta >= -min_eig_tol / 2:  # :333-335: the eigenvalue computation did not reach the precision to escape
                raise RuntimeError("escape direction computation did not converge to the desired precision")
            escaped, info = s.lift(theta, v, gradient_tolerance, preconditioned_gradient_tolerance)
            lev["escape_s"] = time.perf_counter() - t2
            lev["escaped"] = escaped
            lev["lift"] = info
            if not escaped:  # :367-370: no descent found along the escape direction
                break
            ts = time.perf_counter()
        X = s.get_X()
        projected = None
        if project_on_device:
            projected = dict(sigma=None, projected_cost_2f=None, refined_cost_2f=None, refine_iters=None)
            if certified:
                pr = s.project()
                refine = _run_level(s, mode, max_iters, rgrad_tol)
                refined = float(refine["cost"][-1]) if refine["iters"] else s.evaluate()[0]
                projected = dict(sigma=pr["sigma"], projected_cost_2f=pr["cost_2f"], refined_cost_2f=refined,
                                 refine_iters=int(refine["iters"]))
        rounded = s.round(cost=True) if round_on_device else None
    finally:
        s.close()
    if levels and gap is not None:
        last = levels[-1]
        last["suboptimality_gap_f"], last["n_eff"] = gap(X, last["certified"], last.pop("lambda_min"))
    for lev in levels:
        lev.pop("lambda_min", None)
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)
    res = {"X": X, "rank": X.shape[0], "certified": certified, "theta": float(theta), "total_iters": int(total),
           "suboptimality_gap_f": levels[-1]["suboptimality_gap_f"] if levels else None, "levels": levels,
           "cost": cat(cost, float), "gradnorm": cat(gradnorm, float), "selected": cat(selected, np.int32),
           "rank_trace": cat(rank, np.int32)}
    if projected is not None:
        res.update(projected)
    if rounded is not None:
        for key in ("trajectory", "unit_spheres", "landmarks"):
            if key in rounded:
                res[key] = rounded[key]
        res["rounded_cost_2f"], res["rounded_gradnorm"] = rounded.get("cost_2f"), rounded.get("gradnorm")
    return res


def multi_robot_staircase_session(ds, X0, num_robots=5, r_min=5, r_max=100, max_iters=1000, rgrad_tol=0.1,
                                  min_eig_tol=1e-3, gradient_tolerance=1e-6, preconditioned_gradient_tolerance=1e-6,
                                  acceleration=True, params=None, device=0, mode="rbcd++", robust=None, fixed=None,
                                  round_on_device=False, project_on_device=False):
    """multi_robot_example's staircase (same arguments, same outputs) in ONE RbcdSession: the levels are run /
    run_coloured, RbcdSession.certify and RbcdSession.lift, so the agents, their matrices and preconditioners -- and,
    with robust=..., the weights and the GNC state -- live through every level, and the iterate stays on the device
    until the last one.  r_max is capped by the session's largest rank, 16.  round_on_device: RbcdSession.round ends the
    solve (trajectory, rounded_cost_2f, rounded_gradnorm in the result).  project_on_device: after a certified level
    RbcdSession.project takes the session to rank d in place and the level's run parameters refine the point there
    (sigma, projected_cost_2f, refined_cost_2f, refine_iters in the result; the rounding is then of the refined point)."""
    _check_mode(mode)
    d, n = ds.d, ds.n
    ts = time.perf_counter()
    # the certificate's analysis on another host thread while the agents iterate, as multi_robot_example starts it
    prep = threading.Thread(target=lambda: cert_prepare(build_Q_pgo(ds), d, n, block=d + 1, device=device), daemon=True)
    prep.start()
    s = RbcdSession(ds, num_robots=num_robots, r=r_min, acceleration=acceleration and mode == "rbcd++", params=params,
                    device=device, robust=robust, fixed_weight=fixed)
    return _staircase_session(
        s, X0, (d + 1) * n, r_min, min(r_max, 16), max_iters, rgrad_tol, min_eig_tol, gradient_tolerance,
        preconditioned_gradient_tolerance, mode, ts, before_certify=prep.join,
        gap=lambda X, psd, lmin: suboptimality_gap(X.shape[0], d, n, X, psd, min_eig_tol, lmin),
        round_on_device=round_on_device, project_on_device=project_on_device)


def raslam_staircase_session(ra, X0, r_min=None, r_max=100, max_iters=1000, rgrad_tol=0.1, min_eig_tol=1e-3,
                             gradient_tolerance=1e-4, preconditioned_gradient_tolerance=1e-4, acceleration=True,
                             params=None, device=0, mode="rbcd++", robust=None, fixed=None, round_on_device=False,
                             project_on_device=False):
    """multi_robot_raslam_example's staircase (same arguments, same outputs, plus the traces) in ONE RaRbcdSession:
    RaRbcdSession.certify and RaRbcdSession.lift between the levels' runs.  round_on_device: RaRbcdSession.round ends
    the solve (trajectory, unit_spheres, landmarks, rounded_cost_2f, rounded_gradnorm in the result).  project_on_device:
    RaRbcdSession.project and a refinement at rank d after a certified level, as multi_robot_staircase_session."""
    from . import RaRbcdSession, ROptParameters
    _check_mode(mode)
    r_min = ra.d if r_min is None else r_min
    if params is None:
        params = ROptParameters(RTR_iterations=200, RTR_tCG_iterations=200, gradnorm_tol=1e-4)
    ts = time.perf_counter()
    s = RaRbcdSession(ra, r_min, acceleration=acceleration and mode == "rbcd++", params=params, device=device,
                      robust=robust, fixed_weight=fixed)
    return _staircase_session(s, X0, ra.k, r_min, min(r_max, 16), max_iters, rgrad_tol, min_eig_tol,
                              gradient_tolerance, preconditioned_gradient_tolerance, mode, ts,
                              round_on_device=round_on_device, project_on_device=project_on_device)


def _check_mode(mode):
    if mode not in ("rbcd++", "coloured"):
        raise ValueError('mode must be "rbcd++" or "coloured"')


def _run_level(s, mode, max_iters, rgrad_tol):
    """one level's loop on a session of either kind -> the record of its run()"""
    if mode == "rbcd++":
        return s.run(max_iters=max_iters, rgrad_tol=rgrad_tol)
    out = s.run_coloured(max_sweeps=max_iters, rgrad_tol=rgrad_tol)
    out["selected"] = np.full(out["iters"], -1, np.int32)
    return out


def loop_closure_mask(ds, num_robots):
    """measurements the robust outer loop reweights: everything but odometry, i.e. but consecutive poses of one
    robot under the driver's contiguous partition (ref src/Graph.cpp activeLoopClosures / odometry split)"""
    per = ds.n // num_robots
    rob = np.minimum(ds.ids[:, [1, 3]] // per, num_robots - 1)
    return ~((rob[:, 0] == rob[:, 1]) & (ds.ids[:, 3] == ds.ids[:, 1] + 1))


def multi_robot_gnc_example(ds, X0, num_robots=5, r=5, robust=None, num_weight_updates=10, inner_iters=30,
                            rgrad_tol=0.1, max_final_iters=1000, acceleration=True, params=None, fixed=None,
                            device=0):
    """The agents' robust outer loop (ref src/Agent.cpp:1280-1441) around the RBCD session, for all agents at once:

        initializeRobustOptimization: weight 1 on every loop closure that is not fixed, RobustCost reset   (:1332-1346)
        repeat robustOptNumWeightUpdates times:
            RBCD++ for at most robustOptInnerIters iterations (or until |rgrad| < tol)                    (:1280-1330)
            updateMeasurementWeights: residual = sqrt(computeMeasurementError) on the lifted iterate,
                weight = RobustCost::weight(residual); data matrices rebuilt; RobustCost::update;
                warm start (robustOptNumResets = 0); acceleration re-initialised                          (:1397-1441)
        RBCD++ to convergence with the final weights

    ds.vals[:, -1] (the weights) is updated in place.  Returns X, weights, per-round records."""
    from . import robust as rb
    robust = robust or rb.RobustCostParameters("GNC_TLS")
    lc = _gnc_mask(ds, num_robots, fixed)
    w = ds.vals[:, -1]
    w[lc] = 1.0
    at = {}  # the iterate between the rounds' sessions

    def run(iters):
        s = RbcdSession(ds, num_robots=num_robots, r=r, acceleration=acceleration, params=params, device=device)
        s.set_X(at["X"])
        out = s.run(max_iters=iters, rgrad_tol=rgrad_tol)
        at["X"] = s.get_X()
        s.close()
        return out

    def reweight(u):
        e = rb.measurement_errors(ds, at["X"], device=device)
        w[lc] = rb.robust_weights(np.sqrt(e[lc]), robust, num_updates=u)
        return int(np.sum(w[lc] > 1 - 1e-8)), int(np.sum(w[lc] < 1e-8))

    return _gnc_loop(ds, lc, X0, num_weight_updates, inner_iters, max_final_iters, set_X=lambda X: at.update(X=X),
                     run=run, reweight=reweight, read=lambda: (at["X"], w), close=lambda: None)


def _gnc_mask(ds, num_robots, fixed):
    lc = loop_closure_mask(ds, num_robots)
    if fixed is not None:
        lc &= ~np.asarray(fixed, bool)
    return lc


def _counts(c):
    return c["accepted"], c["rejected"]


def _gnc_loop(ds, lc, X0, num_weight_updates, inner_iters, max_final_iters, set_X, run, reweight, read, close,
              store=None):
    """The one flow of the GNC drivers: set_X(X0); num_weight_updates rounds of run(inner_iters) -- the record
    of RbcdSession.run -- then reweight(round) -> (accepted, rejected); run(max_final_iters) with the final weights;
    read() -> X, weights; close(), whatever happened.  ds.vals[:, -1] receives the weights (or store(weights))."""
    rounds = []
    try:
        set_X(np.asarray(X0, dtype=np.float64))
        for u in range(num_weight_updates):
            out = run(inner_iters)
            accepted, rejected = reweight(u)
            rounds.append({"iterations": int(out["iters"]), "cost_2f": float(out["cost"][-1]),
                           "accepted": accepted, "rejected": rejected})
        out = run(max_final_iters)
        X, w = read()
    finally:
        close()
    if store is None:
        ds.vals[:, -1] = w
    else:
        store(w)
    return {"X": X, "weights": w.copy(), "loop_closures": lc, "rounds": rounds,
            "final": {"iterations": int(out["iters"]), "cost_2f": float(out["cost"][-1]),
                      "gradnorm": float(out["gradnorm"][-1])}}


def multi_robot_gnc_session(ds, X0, num_robots=5, r=5, robust=None, num_weight_updates=10, inner_iters=30,
                            rgrad_tol=0.1, max_final_iters=1000, acceleration=True, params=None, fixed=None,
                            device=0):
    """multi_robot_gnc_example's flow (same arguments, same outputs) in ONE session, as the reference's agents run it
    (ref src/Agent.cpp:1280-1441): the session is created robust (weight 1 on every loop closure that is not fixed),
    and each round's updateMeasurementWeights runs in place -- residuals and weights on the device from the session's
    iterate, data matrices and preconditioners rebuilt, acceleration re-initialised, the iterate kept.

    ds.vals[:, -1] (the weights) is updated in place.  Returns X, weights, per-round records."""
    from . import robust as rb
    s = RbcdSession(ds, num_robots=num_robots, r=r, acceleration=acceleration, params=params, device=device,
                    robust=robust or rb.RobustCostParameters("GNC_TLS"), fixed_weight=fixed)
    return _gnc_loop(ds, _gnc_mask(ds, num_robots, fixed), X0, num_weight_updates, inner_iters, max_final_iters,
                     set_X=s.set_X, run=lambda iters: s.run(max_iters=iters, rgrad_tol=rgrad_tol),
                     reweight=lambda u: _counts(s.update_weights()), read=lambda: (s.get_X(), s.get_weights()),
                     close=s.close)


def gnc_ra_session(ra, X0, r, robust=None, num_weight_updates=10, inner_iters=30, rgrad_tol=0.1, max_final_iters=1000,
                   acceleration=True, restart_interval=30, params=None, fixed=None, device=0):
    """multi_robot_gnc_session's flow on a multi-robot range-aided problem (RADataset), in ONE RaRbcdSession: the
    reference's agents run the same robust outer loop on a RangeAidedSLAMGraph as on a pose graph (ref
    src/Agent.cpp:1280-1441), over the pose-pose loop closures only (:1349-1395).  X0 is r x k in the global RA ordering;
    weights, loop_closures and fixed are in pose-pose order.

    ra keeps the final weights (set_pose_pose_weights).  Returns X, weights, per-round records."""
    from . import RaRbcdSession
    from . import robust as rb
    lc = ra.loop_closures()
    if fixed is not None:
        lc &= ~np.asarray(fixed, bool)
    s = RaRbcdSession(ra, r, acceleration=acceleration, restart_interval=restart_interval, params=params, device=device,
                      robust=robust or rb.RobustCostParameters("GNC_TLS"), fixed_weight=fixed)
    return _gnc_loop(ra, lc, X0, num_weight_updates, inner_iters, max_final_iters, set_X=s.set_X,
                     run=lambda iters: s.run(max_iters=iters, rgrad_tol=rgrad_tol),
                     reweight=lambda u: _counts(s.update_weights()), read=lambda: (s.get_X(), s.get_weights()),
                     close=s.close, store=ra.set_pose_pose_weights)


def multi_robot_team_session(ds, X0, num_robots=5, r=5, robust=None, team=None, acceleration=True, params=None,
                             fixed=None, device=0):
    """multi_robot_gnc_session's robust flow driven by the agents' own rules instead of fixed counts (ref
    src/Agent.cpp:558-586, 1123-1156, 1280-1441): RbcdSession.run_team re-weights when every agent has converged since
    the last update (or the inner iterations run out) and stops when all agents are ready after the required number of
    updates, or at max_num_iters.  team: a capi.TeamParams (default: the reference's, team_params()).

    ds.vals[:, -1] (the weights) is updated in place.  Returns X, weights, the run's record and the final statuses."""
    from . import robust as rb
    from . import team_params
    s = RbcdSession(ds, num_robots=num_robots, r=r, acceleration=acceleration, params=params, device=device,
                    robust=robust or rb.RobustCostParameters("GNC_TLS"), fixed_weight=fixed)
    try:
        s.enable_team(team if team is not None else team_params())
        s.set_X(np.asarray(X0, dtype=np.float64))
        out = s.run_team()
        X, w = s.get_X(), s.get_weights()
        statuses = [s.agent_status(q) for q in range(num_robots)]
        stats = [s.loop_closure_stats(q) for q in range(num_robots)]
    finally:
        s.close()
    ds.vals[:, -1] = w
    return {"X": X, "weights": w.copy(), "loop_closures": _gnc_mask(ds, num_robots, fixed), "run": out,
            "statuses": statuses, "loop_closure_stats": stats,
            "final": {"iterations": int(out["iters"]), "cost_2f": float(out["cost"][-1]) if out["iters"] else None,
                      "gradnorm": float(out["gradnorm"][-1]) if out["iters"] else None,
                      "weight_updates": int(out["weight_updates"]), "stop_reason": out["stop_reason"]}}


def ra_team_session(ra, X0, r, robust=None, team=None, acceleration=True, restart_interval=30, params=None,
                    fixed=None, device=0):
    """multi_robot_team_session's flow on a multi-robot range-aided problem (RADataset), in ONE RaRbcdSession: the
    reference's agents run the same status block, termination and weight-update rules on a RangeAidedSLAMGraph as on a
    pose graph (ref src/Agent.cpp:558-586, 1123-1156, 1280-1441), re-weighting the pose-pose loop closures only.  X0 is
    r x k in the global RA ordering; weights, loop_closures and fixed are in pose-pose order, statuses and
    loop_closure_stats by agent (position in the sorted robot list).

    ra keeps the final weights (set_pose_pose_weights).  Returns the record of multi_robot_team_session."""
    from . import RaRbcdSession, team_params
    from . import robust as rb
    lc = ra.loop_closures()
    if fixed is not None:
        lc &= ~np.asarray(fixed, bool)
    s = RaRbcdSession(ra, r, acceleration=acceleration, restart_interval=restart_interval, params=params, device=device,
                      robust=robust or rb.RobustCostParameters("GNC_TLS"), fixed_weight=fixed)
    try:
        s.enable_team(team if team is not None else team_params())
        s.set_X(np.asarray(X0, dtype=np.float64))
        out = s.run_team()
        X, w = s.get_X(), s.get_weights()
        statuses = [s.agent_status(q) for q in range(s.R)]
        stats = [s.loop_closure_stats(q) for q in range(s.R)]
    finally:
        s.close()
    ra.set_pose_pose_weights(w)
    return {"X": X, "weights": w.copy(), "loop_closures": lc, "run": out,
            "statuses": statuses, "loop_closure_stats": stats,
            "final": {"iterations": int(out["iters"]), "cost_2f": float(out["cost"][-1]) if out["iters"] else None,
                      "gradnorm": float(out["gradnorm"][-1]) if out["iters"] else None,
                      "weight_updates": int(out["weight_updates"]), "stop_reason": out["stop_reason"]}}


def exchange_run(ex, max_iters=1000, rgrad_tol=0.1):
    """RbcdSession.run across the ranks: greedy passes through Exchange.iterate until |rgrad| < rgrad_tol, at most
    max_iters (the loop of dcora_rbcd_run, ref examples/MultiRobotExample.cpp:223-307)"""
    cost, gn, sel = [], [], []
    selected = 0
    for _ in range(max_iters):
        c2, g, _, nxt = ex.iterate(selected)
        cost.append(c2)
        gn.append(g)
        sel.append(selected)
        if g < rgrad_tol:
            break
        selected = nxt
    return dict(iters=len(cost), cost=np.asarray(cost, float), gradnorm=np.asarray(gn, float),
                selected=np.asarray(sel, np.int32))


def multi_robot_gnc_ranks(ds, X0, num_robots=5, r=5, robust=None, num_weight_updates=10, inner_iters=30,
                          rgrad_tol=0.1, max_final_iters=1000, acceleration=True, params=None, fixed=None, device=0,
                          rank=0, world_size=1, job_name="gnc"):
    """multi_robot_gnc_session on one rank of a multi-rank job (SPMD: every rank calls it with the same arguments but
    rank): the ranks' robust sessions and their exchange (robust_ranked_session), the inner loops through
    Exchange.iterate, every updateMeasurementWeights collective.  The same outputs on every rank: X gathered, the
    job's weights.

    ds.vals[:, -1] (the weights) is updated in place.  Returns X, weights, per-round records."""
    from . import robust as rb
    from . import robust_ranked_session
    s, ex = robust_ranked_session(ds, job_name, num_robots=num_robots, r=r,
                                  robust=robust or rb.RobustCostParameters("GNC_TLS"), fixed_weight=fixed, rank=rank,
                                  world_size=world_size, device=device, acceleration=acceleration, params=params)
    return _gnc_loop(ds, _gnc_mask(ds, num_robots, fixed), X0, num_weight_updates, inner_iters, max_final_iters,
                     set_X=ex.set_X, run=lambda iters: exchange_run(ex, max_iters=iters, rgrad_tol=rgrad_tol),
                     reweight=lambda u: _counts(ex.update_weights()), read=lambda: (ex.gather_X(), ex.get_weights()),
                     close=lambda: (ex.close(), s.close()))


def gnc_ra_ranks(ra, X0, r, robust=None, num_weight_updates=10, inner_iters=30, rgrad_tol=0.1, max_final_iters=1000,
                 acceleration=True, restart_interval=30, params=None, fixed=None, device=0, rank=0, world_size=1,
                 job_name="ra_gnc"):
    """gnc_ra_session on one rank of a multi-rank job (SPMD: every rank calls it with the same arguments but rank): the
    ranks' robust range-aided sessions and their exchange (ra_robust_ranked_session), the inner loops through
    Exchange.iterate, every updateMeasurementWeights collective.  The same outputs on every rank: X gathered, the
    job's pose-pose weights.

    ra keeps the final weights (set_pose_pose_weights).  Returns X, weights, per-round records."""
    from . import ra_robust_ranked_session
    from . import robust as rb
    lc = ra.loop_closures()
    if fixed is not None:
        lc &= ~np.asarray(fixed, bool)
    s, ex = ra_robust_ranked_session(ra, job_name, r, robust=robust or rb.RobustCostParameters("GNC_TLS"),
                                     fixed_weight=fixed, rank=rank, world_size=world_size, device=device,
                                     acceleration=acceleration, restart_interval=restart_interval, params=params)
    return _gnc_loop(ra, lc, X0, num_weight_updates, inner_iters, max_final_iters, set_X=ex.set_X,
                     run=lambda iters: exchange_run(ex, max_iters=iters, rgrad_tol=rgrad_tol),
                     reweight=lambda u: _counts(ex.update_weights()), read=lambda: (ex.gather_X(), ex.get_weights()),
                     close=lambda: (ex.close(), s.close()), store=ra.set_pose_pose_weights)


def _check_certificate(certificate):
    if certificate not in ("host", "live"):
        raise ValueError('certificate must be "host" or "live"')
    return certificate == "live"


class _RanksJob:
    """one rank's (session, exchange) of a job behind the calls _staircase_session makes on a session: run /
    run_coloured across the ranks, Exchange.certify with the global Q on rank 0 (q_now(): the job's current matrix,
    called on every rank because reading a robust job's weights is collective) and Exchange.lift.  certificate="live":
    Exchange.certify_live instead -- the certificate of the matrices the ranks hold; q_now is never called and no Q is
    built on the host"""

    def __init__(self, s, ex, k, rank, q_now, certificate="host"):
        self.s, self.ex, self.k, self.rank, self.q_now, self.certificate = s, ex, k, rank, q_now, certificate

    @property
    def r(self):
        return self.s.r

    def set_X(self, X):
        self.ex.set_X(X)

    def get_X(self):
        return self.ex.gather_X()

    def run(self, max_iters, rgrad_tol):
        return exchange_run(self.ex, max_iters=max_iters, rgrad_tol=rgrad_tol)

    def run_coloured(self, max_sweeps, rgrad_tol):
        return self.ex.run_coloured(max_sweeps=max_sweeps, rgrad_tol=rgrad_tol)

    def certify(self, eta):
        if self.certificate == "live":
            cert, theta, lmin, v, mv, dist, info = self.ex.certify_live(eta)
            return cert, theta, v, lmin, {"matvecs": mv, "distributed": dist, "rounds": info["rounds"]}
        Q = self.q_now()
        cert, theta, lmin, v, mv, dist = self.ex.certify(Q if self.rank == 0 else None, eta, self.k)
        return cert, theta, v, lmin, {"matvecs": mv, "distributed": dist}

    def lift(self, theta, v, gradient_tolerance, preconditioned_gradient_tolerance):
        return self.ex.lift(theta, v, gradient_tolerance, preconditioned_gradient_tolerance)

    def round(self, cost=False):
        return self.ex.round()  # (no rounded cost across ranks: no rank holds the whole problem)

    def project(self):
        return self.ex.project()

    def evaluate(self):
        return self.ex.evaluate()

    def close(self):
        # (reached from a `finally`: after an error of the exchange the barrier raises as well -- the exchange and the
        # session are closed all the same, and the first error stays the one the caller sees)
        try:
            if sys.exc_info()[0] is None:
                self.ex.barrier()
        finally:
            self.ex.close()
            self.s.close()


def multi_robot_staircase_ranks(ds, X0, num_robots=5, r_min=5, r_max=100, max_iters=1000, rgrad_tol=0.1,
                                min_eig_tol=1e-3, gradient_tolerance=1e-6, preconditioned_gradient_tolerance=1e-6,
                                acceleration=True, params=None, device=0, mode="rbcd++", robust=None, fixed=None, rank=0,
                                world_size=1, job_name="staircase", certificate="host", round_on_device=False):
    """multi_robot_staircase_session on one rank of a multi-rank job (SPMD: every rank calls it with the same arguments
    but rank; ref examples/MultiRobotExample.cpp:223-370): per level exchange_run (or the coloured sweeps),
    Exchange.certify and Exchange.lift, robust or plain -- the job never leaves the library between its levels.  The
    sessions reserve min(r_max, 16) rows before their exchange is created.  The same outputs on every rank.
    With robust=..., ds.vals[:, -1] (the weights) is updated in place before every certificate, as
    multi_robot_gnc_ranks leaves them.
    certificate: "host" -- Exchange.certify on the global Q, rebuilt on the host from the job's weights before every
    certificate; "live" -- Exchange.certify_live, the certificate of the matrices the ranks hold on the device: no Q is
    built on the host and ds is not written.
    round_on_device: Exchange.round ends the solve -- every rank rounds its own agents' states against pose 0 and every
    rank's result carries the whole trajectory (rounded_cost_2f and rounded_gradnorm are None: no rank holds the whole
    problem).  multi_robot_staircase_ranks_projected ends a certified solve with the projection to rank d as well."""
    return _multi_robot_staircase_ranks(False, **locals())


def multi_robot_staircase_ranks_projected(ds, X0, round_on_device=True, **kw):
    """multi_robot_staircase_ranks (its arguments, SPMD) ended as CORA ends a certified solve (ref
    examples/SingleRobotExample_RASLAM.cpp:220-234), what project_on_device=True is to multi_robot_staircase_session:
    after a certified level Exchange.project takes the whole job to rank d in place, the level's own run parameters
    refine it there and (round_on_device) Exchange.round rounds the refined point.  Every key of
    multi_robot_staircase_ranks is what it is there; the result also carries sigma, projected_cost_2f,
    refined_cost_2f and refine_iters (None where no level was certified), the same on every rank."""
    return _multi_robot_staircase_ranks(True, ds=ds, X0=X0, round_on_device=round_on_device, **kw)


def _multi_robot_staircase_ranks(project_on_device, ds, X0, num_robots=5, r_min=5, r_max=100, max_iters=1000,
                                 rgrad_tol=0.1, min_eig_tol=1e-3, gradient_tolerance=1e-6,
                                 preconditioned_gradient_tolerance=1e-6, acceleration=True, params=None, device=0,
                                 mode="rbcd++", robust=None, fixed=None, rank=0, world_size=1, job_name="staircase",
                                 certificate="host", round_on_device=False):
    from . import Exchange, robust_ranked_session
    _check_mode(mode)
    live = _check_certificate(certificate)
    d, n = ds.d, ds.n
    r_top = max(min(r_max, 16), r_min)
    ts = time.perf_counter()
    accel = acceleration and mode == "rbcd++"
    if robust is None:
        s = RbcdSession(ds, num_robots=num_robots, r=r_min, acceleration=accel, params=params, device=device, rank=rank,
                        world_size=world_size)
        s.reserve_rank(r_top)
        ex = Exchange(s, job_name)
        Q = build_Q_pgo(ds) if rank == 0 and not live else None
        q_now = lambda: Q
    else:
        s, ex = robust_ranked_session(ds, job_name, num_robots=num_robots, r=r_min, robust=robust, fixed_weight=fixed,
                                      rank=rank, world_size=world_size, device=device, acceleration=accel, params=params,
                                      r_reserve=r_top)

        def q_now():
            ds.vals[:, -1] = ex.get_weights()
            return build_Q_pgo(ds) if rank == 0 else None
    return _staircase_session(
        _RanksJob(s, ex, (d + 1) * n, rank, q_now, certificate), X0, (d + 1) * n, r_min, r_top, max_iters, rgrad_tol, min_eig_tol,
        gradient_tolerance, preconditioned_gradient_tolerance, mode, ts,
        gap=lambda X, psd, lmin: suboptimality_gap(X.shape[0], d, n, X, psd, min_eig_tol, lmin),
        round_on_device=round_on_device, project_on_device=project_on_device)


def raslam_staircase_ranks(ra, X0, r_min=None, r_max=100, max_iters=1000, rgrad_tol=0.1, min_eig_tol=1e-3,
                           gradient_tolerance=1e-4, preconditioned_gradient_tolerance=1e-4, acceleration=True,
                           params=None, device=0, mode="rbcd++", robust=None, fixed=None, rank=0, world_size=1,
                           job_name="ra_staircase", certificate="host", round_on_device=False):
    """raslam_staircase_session on one rank of a multi-rank range-aided job (SPMD, as multi_robot_staircase_ranks; ref
    examples/MultiRobotExample_RASLAM.cpp): exchange_run, Exchange.certify and Exchange.lift per level.  With
    robust=..., ra keeps the job's current pose-pose weights (set_pose_pose_weights before every certificate), as
    gnc_ra_ranks leaves them.  certificate: as multi_robot_staircase_ranks ("live": ra is not written).
    round_on_device: as multi_robot_staircase_ranks, with unit_spheres and landmarks.
    raslam_staircase_ranks_projected ends a certified solve with the projection to rank d as well."""
    return _raslam_staircase_ranks(False, **locals())


def raslam_staircase_ranks_projected(ra, X0, round_on_device=True, **kw):
    """raslam_staircase_ranks (its arguments, SPMD) ended with Exchange.project, the refinement at rank d and
    (round_on_device) Exchange.round: multi_robot_staircase_ranks_projected for a range-aided job"""
    return _raslam_staircase_ranks(True, ra=ra, X0=X0, round_on_device=round_on_device, **kw)


def _raslam_staircase_ranks(project_on_device, ra, X0, r_min=None, r_max=100, max_iters=1000, rgrad_tol=0.1,
                            min_eig_tol=1e-3, gradient_tolerance=1e-4, preconditioned_gradient_tolerance=1e-4,
                            acceleration=True, params=None, device=0, mode="rbcd++", robust=None, fixed=None, rank=0,
                            world_size=1, job_name="ra_staircase", certificate="host", round_on_device=False):
    from . import Exchange, RaRbcdSession, ROptParameters, ra_robust_ranked_session
    _check_mode(mode)
    _check_certificate(certificate)
    r_min = ra.d if r_min is None else r_min
    r_top = max(min(r_max, 16), r_min)
    if params is None:
        params = ROptParameters(RTR_iterations=200, RTR_tCG_iterations=200, gradnorm_tol=1e-4)
    ts = time.perf_counter()
    accel = acceleration and mode == "rbcd++"
    if robust is None:
        s = RaRbcdSession(ra, r_min, acceleration=accel, params=params, device=device, rank=rank, world_size=world_size)
        s.reserve_rank(r_top)
        ex = Exchange(s, job_name)
        q_now = lambda: ra.Q
    else:
        s, ex = ra_robust_ranked_session(ra, job_name, r_min, robust=robust, fixed_weight=fixed, rank=rank,
                                         world_size=world_size, device=device, acceleration=accel, params=params,
                                         r_reserve=r_top)

        def q_now():
            ra.set_pose_pose_weights(ex.get_weights())
            return ra.Q
    return _staircase_session(_RanksJob(s, ex, ra.k, rank, q_now, certificate), X0, ra.k, r_min, r_top, max_iters, rgrad_tol,
                              min_eig_tol, gradient_tolerance, preconditioned_gradient_tolerance, mode, ts,
                              round_on_device=round_on_device, project_on_device=project_on_device)


def multi_robot_team_ranks(ds, X0, num_robots=5, r=5, robust=None, team=None, acceleration=True, params=None,
                           fixed=None, device=0, rank=0, world_size=1, job_name="team"):
    """multi_robot_team_session on one rank of a multi-rank job (SPMD: every rank calls it with the same arguments but
    rank): the ranks' robust sessions and their exchange (robust_ranked_session), the team enabled through the exchange
    so that every rank holds every agent's status, Exchange.run_team re-weighting and stopping by the agents' rules.
    The same outputs on every rank: X gathered, the job's weights, the statuses.

    ds.vals[:, -1] (the weights) is updated in place.  Returns X, weights, the run's record and the final statuses."""
    from . import robust as rb
    from . import robust_ranked_session, team_params
    s, ex = robust_ranked_session(ds, job_name, num_robots=num_robots, r=r,
                                  robust=robust or rb.RobustCostParameters("GNC_TLS"), fixed_weight=fixed, rank=rank,
                                  world_size=world_size, device=device, acceleration=acceleration, params=params)
    try:
        ex.enable_team(team if team is not None else team_params())
        ex.set_X(np.asarray(X0, dtype=np.float64))
        out = ex.run_team()
        X, w = ex.gather_X(), ex.get_weights()
        statuses = [ex.agent_status(q) for q in range(num_robots)]
        stats = [ex.loop_closure_stats(q) for q in range(num_robots)]
        ex.barrier()
    finally:
        ex.close()
        s.close()
    ds.vals[:, -1] = w
    return {"X": X, "weights": w.copy(), "loop_closures": _gnc_mask(ds, num_robots, fixed), "run": out,
            "statuses": statuses, "loop_closure_stats": stats,
            "final": {"iterations": int(out["iters"]), "cost_2f": float(out["cost"][-1]) if out["iters"] else None,
                      "gradnorm": float(out["gradnorm"][-1]) if out["iters"] else None,
                      "weight_updates": int(out["weight_updates"]), "stop_reason": out["stop_reason"]}}


def ra_team_ranks(ra, X0, r, robust=None, team=None, acceleration=True, restart_interval=30, params=None, fixed=None,
                  device=0, rank=0, world_size=1, job_name="ra_team"):
    """ra_team_session on one rank of a multi-rank job (SPMD: every rank calls it with the same arguments but rank): the
    ranks' robust range-aided sessions and their exchange (ra_robust_ranked_session), the team enabled through the
    exchange so that every rank holds every agent's status, Exchange.run_team re-weighting and stopping by the agents'
    rules.  The same outputs on every rank: X gathered, the job's pose-pose weights, the statuses.

    ra keeps the final weights (set_pose_pose_weights).  Returns the record of multi_robot_team_ranks."""
    from . import ra_robust_ranked_session, team_params
    from . import robust as rb
    lc = ra.loop_closures()
    if fixed is not None:
        lc &= ~np.asarray(fixed, bool)
    s, ex = ra_robust_ranked_session(ra, job_name, r, robust=robust or rb.RobustCostParameters("GNC_TLS"),
                                     fixed_weight=fixed, rank=rank, world_size=world_size, device=device,
                                     acceleration=acceleration, restart_interval=restart_interval, params=params)
    try:
        ex.enable_team_ra(team if team is not None else team_params())
        ex.set_X(np.asarray(X0, dtype=np.float64))
        out = ex.run_team()
        X, w = ex.gather_X(), ex.get_weights()
        statuses = [ex.agent_status(q) for q in range(s.R)]
        stats = [ex.loop_closure_stats(q) for q in range(s.R)]
        ex.barrier()
    finally:
        ex.close()
        s.close()
    ra.set_pose_pose_weights(w)
    return {"X": X, "weights": w.copy(), "loop_closures": lc, "run": out,
            "statuses": statuses, "loop_closure_stats": stats,
            "final": {"iterations": int(out["iters"]), "cost_2f": float(out["cost"][-1]) if out["iters"] else None,
                      "gradnorm": float(out["gradnorm"][-1]) if out["iters"] else None,
                      "weight_updates": int(out["weight_updates"]), "stop_reason": out["stop_reason"]}}


def multi_robot_raslam_example(ra, X0, r_min=None, r_max=100, max_iters=1000, rgrad_tol=0.1, min_eig_tol=1e-3,
                               gradient_tolerance=1e-4, preconditioned_gradient_tolerance=1e-4, acceleration=True,
                               params=None, device=0, mode="rbcd++"):
    """The multi-robot range-aided SLAM driver (ref examples/MultiRobotExample_RASLAM.cpp) over the C ABI: per level
    the agents' RBCD++ (dcora_ra_rbcd_*), the merged problem's dual certificate and fastVerification, escapeSaddle of
    the central problem into the next rank.  Defaults of the example: r_min = d, local RTR 200 x 200 at 1e-4,
    |rgrad| < 0.1, eigenvalue tolerance 1e-3.  X0: r_min x k (RA ordering).  mode: as multi_robot_example."""
    from . import RaRbcdSession, ROptParameters, precond_regularization
    _check_mode(mode)
    d, n, l, b, k = ra.d, ra.n, ra.l, ra.b, ra.k
    r_min = d if r_min is None else r_min
    if params is None:
        params = ROptParameters(RTR_iterations=200, RTR_tCG_iterations=200, gradnorm_tol=1e-4)
    X = np.asarray(X0, dtype=np.float64)
    if X.shape != (r_min, k):
        raise ValueError("X0 must be r_min x k")
    reg = None
    levels, certified, theta, total = [], False, 0.0, 0
    r = r_min
    while r < r_max:
        ts = time.perf_counter()
        s = RaRbcdSession(ra, r, acceleration=acceleration and mode == "rbcd++", params=params, device=device)
        s.set_X(X)
        t0 = time.perf_counter()
        out = _run_level(s, mode, max_iters, rgrad_tol)
        t1 = time.perf_counter()
        Xopt = s.get_X()
        s.close()
        total += out["iters"]
        S = dual_certificate(r, d, n, Xopt, ra.Q, l=l, b=b, device=device)
        psd, theta, v, lmin = fast_verification(S, min_eig_tol, block=1, device=device)
        t2 = time.perf_counter()
        lev = {"rank": r, "iterations": int(out["iters"]), "cost_2f": float(out["cost"][-1]),
               "gradnorm": float(out["gradnorm"][-1]), "setup_s": t0 - ts, "rbcd_s": t1 - t0,
               "certification_s": t2 - t1,
               "certified": bool(psd), "theta": float(theta), "mode": mode}
        levels.append(lev)
        X = Xopt
        if psd:
            certified = True
            break
        if theta >= -min_eig_tol / 2:
            raise RuntimeError("escape direction computation did not converge to the desired precision")
        if reg is None:
            reg = precond_regularization(ra.Q, device=device)
        Pn = QuadraticProblem(r + 1, d, n, ra.Q, reg=reg, l=l, b=b, device=device)
        Xn = Pn.escapeSaddle(Xopt, theta, v, gradient_tolerance, preconditioned_gradient_tolerance)
        Pn.close()
        lev["escape_s"] = time.perf_counter() - t2
        lev["escaped"] = Xn is not None
        if Xn is None:
            break
        X = Xn
        r += 1
    return {"X": X, "rank": X.shape[0], "certified": certified, "theta": float(theta), "total_iters": int(total),
            "levels": levels}
