"""What the staircase's step costs in place (RbcdSession.lift / RaRbcdSession.lift) against the path the drivers that
re-create their sessions take for the same step (driver.multi_robot_example, driver.multi_robot_raslam_example):
get_X, close, a whole-graph QuadraticProblem at r + 1 for escapeSaddle, a new session at r + 1, set_X -- and
set_weights on a robust session.

Workloads: sphere2500 / 5 agents from rank 5 at the seed-4 random point (plain and robust), tiers.pyfg (four robots)
from rank 3 at a random point.  (theta, v) comes from the host certificate, outside the clock, the same for both paths.
Two cache states, five alternated rounds each, in one process:
  cold  precond_cache_clear, then the session at r is created (not timed): the step pays the whole-graph preconditioner
        on either path (and, range-aided, its regularisation);
  warm  the second level: the step r + 1 -> r + 2 from the point the first step reached; the whole-graph preconditioner
        is in the cache (re-creating path) or attached to the session's central problem (lift).
Times are host clocks around calls that end in a device synchronise.  Every round checks that both paths reach the same
point.  The launch count of a session that never lifts -- creation, set_X and 100 iterations of sphere2500 / 5 agents,
dcora_debug_launch_count -- is taken in a child process, and with --parent-lib also with another build of the library.

    python tools/lift_cost.py [--rounds K] [--parent-lib PATH] [--out profiles/lift_cost.txt]

Prints one JSON line per case and writes the table."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def launch_count(lib):
    from dcora_amd import capi
    if lib:  # (another build may lack entry points this one has: bind what it exports)
        import ctypes
        capi.LIB_PATH = lib
        other = ctypes.CDLL(lib)
        capi.SIGNATURES = {k: q for k, q in capi.SIGNATURES.items() if hasattr(other, k)}
    import common
    import dcora_amd as da
    ds = common.product_dataset("sphere2500")
    X = common.random_point(5, ds.d, ds.n, 4, da.manifold_project)
    n0 = da.debug_launch_count()
    s = da.RbcdSession(ds, num_robots=5, r=5)
    s.set_X(X)
    out = s.run(max_iters=100, rgrad_tol=0.0)
    n1 = da.debug_launch_count()
    s.close()
    print(json.dumps({"launches": n1 - n0, "iterations": int(out["iters"]), "cost_2f": float(out["cost"][-1])}))


def stats(ms):
    ms = np.asarray(ms)
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max()), "rounds": int(ms.size)}


class Case:
    """one workload: make(r) -> a session at rank r, whole_graph(r) -> the QuadraticProblem of the re-creating path,
    direction(r, X) -> (theta, v) of the host certificate"""

    def __init__(self, da, name, kind, robust):
        import common
        from dcora_amd import robust as rb
        self.da, self.name, self.kind, self.robust = da, name, kind, robust
        self.params = rb.RobustCostParameters("GNC_TLS", GNCBarc=10.0, GNCMuStep=2.0) if robust else None
        self.w = None
        if kind == "pgo":
            self.ds = common.product_dataset("sphere2500")
            self.d, self.n, self.kw, self.block, self.r = self.ds.d, self.ds.n, {}, self.ds.d + 1, 5
            self.k = (self.d + 1) * self.n
            self.tol = (1e-6, 1e-6)
            if robust:
                self.w = np.random.default_rng(7).uniform(0.05, 1.0, self.ds.m)
                wds = da.Dataset(self.ds.d, self.ds.n, self.ds.ids.copy(), self.ds.vals.copy())
                wds.vals[:, -1] = self.w
                self.Q = da.build_Q_pgo(wds)
            else:
                self.Q = da.build_Q_pgo(self.ds)
            self.reg = 0.1
            self.X = common.random_point(self.r, self.d, self.n, 4, da.manifold_project)
        else:
            from test_raslam import ra_path
            self.ra = da.RADataset(ra_path("tiers"))
            ra = self.ra
            self.d, self.n, self.k, self.kw, self.block, self.r = ra.d, ra.n, ra.k, dict(l=ra.l, b=ra.b), 1, 3
            self.tol = (1e-4, 1e-4)
            self.Q, self.reg = ra.Q, None
            M = np.random.default_rng(4).uniform(-1, 1, (self.r, self.k))
            self.X = da.manifold_project(self.r, self.d, self.n, M, **self.kw)

    def make(self, r, weights=True):
        da = self.da
        if self.kind == "pgo":
            s = da.RbcdSession(self.ds, num_robots=5, r=r, robust=self.params)
        else:
            s = da.RaRbcdSession(self.ra, r, params=da.ROptParameters(RTR_iterations=200, RTR_tCG_iterations=200,
                                                                      gradnorm_tol=1e-4))
        if self.robust and weights:
            s.set_weights(self.w)
        return s

    def whole_graph(self, r):
        da = self.da
        if self.reg is None:  # the range-aided driver computes it before its first escape
            self.reg = da.precond_regularization(self.Q)
        return da.QuadraticProblem(r, self.d, self.n, self.Q, reg=self.reg, **self.kw)

    def direction(self, r, X):
        da = self.da
        S = da.dual_certificate(r, self.d, self.n, X, self.Q, **self.kw)
        psd, theta, v, lmin = da.fast_verification(S, 1e-3, block=self.block)
        if psd:
            raise RuntimeError("%s: the certificate accepts the point, nothing to time" % self.name)
        return theta, v

    def recreate(self, s, r, theta, v):
        """the re-creating drivers' step; -> (ms, the new session)"""
        t0 = time.perf_counter()
        X = s.get_X()
        w = s.get_weights() if self.robust else None
        s.close()
        P = self.whole_graph(r + 1)
        Xn = P.escapeSaddle(X, theta, v, *self.tol)
        P.close()
        n = self.make(r + 1, weights=False)
        if self.robust:
            n.set_weights(w)
        n.set_X(Xn)
        return 1e3 * (time.perf_counter() - t0), n

    def lift(self, s, theta, v):
        t0 = time.perf_counter()
        escaped, info = s.lift(theta, v, *self.tol)
        ms = 1e3 * (time.perf_counter() - t0)
        if not escaped:
            raise RuntimeError("%s: no escape" % self.name)
        return ms, info


def run_case(da, case, rounds):
    r, X = case.r, case.X
    theta, v = case.direction(r, X)
    res = {"case": case.name, "k": case.k, "from_rank": r}
    # the first step once, outside the clock: the point and the direction of the second level
    s = case.make(r)
    s.set_X(X)
    case.lift(s, theta, v)
    X1 = s.get_X()
    s.close()
    theta1, v1 = case.direction(r + 1, X1)
    for state in ("cold", "warm"):
        rec, lif, split, same = [], [], [], True
        if state == "warm":  # the re-creating driver has made its first escape: regularisation known, image cached
            case.whole_graph(r + 1).close()
        for i in range(rounds):
            for path in (("recreate", "lift") if i % 2 == 0 else ("lift", "recreate")):
                if state == "cold":
                    da.precond_cache_clear()
                    case.reg = None if case.kind == "ra" else case.reg
                    s = case.make(r)
                    s.set_X(X)
                    args = (r, theta, v)
                elif path == "lift":  # the session that made the first step itself
                    s = case.make(r)
                    s.set_X(X)
                    case.lift(s, theta, v)
                    args = (r + 1, theta1, v1)
                else:
                    s = case.make(r + 1)
                    s.set_X(X1)
                    args = (r + 1, theta1, v1)
                if path == "recreate":
                    ms, n = case.recreate(s, *args)
                    rec.append(ms)
                    Xa = n.get_X()
                    n.close()
                else:
                    ms, info = case.lift(s, args[1], args[2])
                    lif.append(ms)
                    split.append(info)
                    Xb = s.get_X()
                    s.close()
            same = same and bool(np.abs(Xa - Xb).max() <= 1e-12 * np.abs(Xa).max())
        res[state] = {"recreate_ms": stats(rec), "lift_ms": stats(lif), "same_point": same,
                      "lift_precond_ms": float(np.median([q["precond_ms"] for q in split])),
                      "lift_redimension_ms": float(np.median([q["redimension_ms"] for q in split])),
                      "lift_inside_ms": float(np.median([q["total_ms"] for q in split])),
                      "lift_trials": int(split[0]["trials"])}
    w = res["warm"]
    spread = w["recreate_ms"]["max"] - w["recreate_ms"]["min"]
    w["lift_below_recreate_by_more_than_its_spread"] = bool(
        w["recreate_ms"]["median"] - w["lift_ms"]["median"] > spread)
    return res


def child_count(lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--launch-count"] + (["--lib", lib] if lib else [])
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="another build of libdcora_hip.so to count launches with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_cost.txt"))
    ap.add_argument("--launch-count", action="store_true", help="(child) print the launch count and leave")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.launch_count:
        launch_count(a.lib)
        return
    import dcora_amd as da
    if da.device_count() < 1:
        raise SystemExit("lift_cost needs a GPU")
    lines = ["lift against re-creating the session for one staircase step (tools/lift_cost.py), ms, %d alternated "
             "rounds: median (min .. max)" % a.rounds, ""]
    fmt = lambda q: "%9.2f (%8.2f .. %8.2f)" % (q["median"], q["min"], q["max"])
    for name, kind, robust in (("sphere2500 / 5 agents, 5 -> 6 (warm: 6 -> 7)", "pgo", False),
                               ("sphere2500 / 5 agents, robust, 5 -> 6 (warm: 6 -> 7)", "pgo", True),
                               ("tiers.pyfg / 4 robots, 3 -> 4 (warm: 4 -> 5)", "ra", False)):
        res = run_case(da, Case(da, name, kind, robust), a.rounds)
        print(json.dumps(res), flush=True)
        lines.append("%s, k = %d" % (name, res["k"]))
        for state in ("cold", "warm"):
            q = res[state]
            lines.append("  %s  re-create %s   lift %s   same point: %s" %
                         (state, fmt(q["recreate_ms"]), fmt(q["lift_ms"]), q["same_point"]))
            lines.append("        inside lift (medians): central preconditioner %.2f, re-dimensioning %.2f, total %.2f; "
                         "%d trial(s)" % (q["lift_precond_ms"], q["lift_redimension_ms"], q["lift_inside_ms"],
                                          q["lift_trials"]))
        lines.append("  warm: lift below re-creating by more than the re-creating rounds' spread: %s" %
                     res["warm"]["lift_below_recreate_by_more_than_its_spread"])
        lines.append("")
    here = child_count(None)
    lines.append("a session that never lifts (sphere2500 / 5 agents: creation, set_X, 100 iterations): %d launches, "
                 "final 2f %.9f" % (here["launches"], here["cost_2f"]))
    print(json.dumps({"launch_count": here}), flush=True)
    if a.parent_lib:
        parent = child_count(a.parent_lib)
        print(json.dumps({"launch_count_parent_build": parent}), flush=True)
        lines.append("the same with the parent commit's build of the library: %d launches, final 2f %.9f -> %s" %
                     (parent["launches"], parent["cost_2f"],
                      "the same" if parent == here else "DIFFERENT"))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
