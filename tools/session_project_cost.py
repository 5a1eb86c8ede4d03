"""What the projection of a live session to rank d costs in place (RbcdSession.project / RaRbcdSession.project) against
the detour a user of a session had to take before: get_X, the host-fed project_solution_raslam (which uploads X again),
close, a new session at rank d, set_X.

Workloads: sphere2500 / 5 agents / r = 5, tiers.pyfg / 4 robots / r = 4, the 100k-pose lattice / 8 agents / r = 5, each
at a random point of its manifold after three iterations.  Ten alternated rounds per path and cache state, in one
process:
  warm  the detour's new session finds its preconditioners in the cache;
  cold  precond_cache_clear before the detour's new session is created (the in-place path builds nothing either way).
Times are host clocks around calls that end in a device synchronise; the parts of the in-place call are its own
(info8[4..6]: events around the kernels, host clock around the re-dimensioning).  Every round checks that both paths
reach the same point up to a global rotation (Gram matrices of the rotation columns within 1e-9).

The Gram kernel alone (k_gram_mfma + k_gram_finish) against the host-fed path's k_gram on the same X is a kernel trace of
its own: run  rocprofv3 --kernel-trace --stats -- python tools/session_project_cost.py --gram-only  and read the two
kernels' rows; without a trace, --gram-only prints host-clock times of the two whole calls, which are dominated by
their copies and say nothing about the kernels.

    python tools/session_project_cost.py [--rounds K] [--skip-lattice] [--out profiles/session_project.txt]

Prints one JSON line per case and writes the table."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def stats(ms):
    ms = np.asarray(ms)
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max()), "rounds": int(ms.size)}


class Case:
    def __init__(self, da, kind):
        import common
        self.da, self.kind = da, kind
        if kind == "tiers":
            from test_raslam import ra_path
            self.ra = da.RADataset(ra_path("tiers"))
            ra = self.ra
            self.name, self.r, self.d, self.n, self.l, self.b, self.k = "tiers.pyfg / 4 robots / r = 4", 4, ra.d, ra.n, ra.l, ra.b, ra.k
            M = np.random.default_rng(4).uniform(-1, 1, (self.r, self.k))
            self.X0 = da.manifold_project(self.r, self.d, self.n, M, l=ra.l, b=ra.b)
        else:
            if kind == "sphere":
                self.ds, self.R, self.name = common.product_dataset("sphere2500"), 5, "sphere2500 / 5 agents / r = 5"
            else:
                from dcora_amd import synth
                self.ds, self.R, self.name = synth.lattice_se3(), 8, "100k-pose lattice / 8 agents / r = 5"
            self.r, self.d, self.n, self.l, self.b = 5, self.ds.d, self.ds.n, 0, 0
            self.k = (self.d + 1) * self.n
            self.X0 = common.random_point(self.r, self.d, self.n, 4, da.manifold_project)

    def make(self, r):
        da = self.da
        if self.kind == "tiers":
            return da.RaRbcdSession(self.ra, r, params=da.ROptParameters(RTR_iterations=200, RTR_tCG_iterations=200,
                                                                          gradnorm_tol=1e-4))
        return da.RbcdSession(self.ds, num_robots=self.R, r=r)

    def start(self):
        s = self.make(self.r)
        s.set_X(self.X0)
        s.run(max_iters=3, rgrad_tol=0.0)
        return s

    def to_ra(self, X):
        if self.kind == "tiers":
            return X
        rows, d, n = X.shape[0], self.d, self.n
        out = np.zeros_like(X)
        out[:, :d * n] = X.reshape(rows, n, d + 1)[:, :, :d].reshape(rows, d * n)
        out[:, d * n:] = X[:, d::d + 1]
        return out

    def from_ra(self, P):
        if self.kind == "tiers":
            return P
        rows, d, n = P.shape[0], self.d, self.n
        out = np.zeros_like(P)
        out.reshape(rows, n, d + 1)[:, :, :d] = P[:, :d * n].reshape(rows, n, d)
        out[:, d::d + 1] = P[:, d * n:]
        return out

    def in_place(self, s):
        t0 = time.perf_counter()
        out = s.project()
        return 1e3 * (time.perf_counter() - t0), out

    def detour(self, s, cold):
        da = self.da
        t0 = time.perf_counter()
        X = s.get_X()
        P = self.from_ra(da.project_solution_raslam(self.to_ra(X), self.r, self.d, self.n, self.l, self.b))
        s.close()
        if cold:
            da.precond_cache_clear()
        n = self.make(self.d)
        n.set_X(P)
        return 1e3 * (time.perf_counter() - t0), n

    def rotation_gram(self, P):
        cols = min(self.d * self.n, 600)
        R = self.to_ra(P)[:, :cols]
        return R.T @ R


def run_case(case, rounds):
    res = {"case": case.name, "k": case.k, "from_rank": case.r, "to_rank": case.d}
    for state in ("warm", "cold"):
        inp, det, parts, same = [], [], [], True
        for i in range(rounds):
            for path in (("detour", "project") if i % 2 == 0 else ("project", "detour")):
                s = case.start()
                if path == "project":
                    ms, out = case.in_place(s)
                    inp.append(ms)
                    parts.append(out)
                    Pa = s.get_X()
                    s.close()
                else:
                    ms, n = case.detour(s, state == "cold")
                    det.append(ms)
                    Pb = n.get_X()
                    n.close()
            same = same and bool(np.abs(case.rotation_gram(Pa) - case.rotation_gram(Pb)).max() <= 1e-9)
        res[state] = {"project_ms": stats(inp), "detour_ms": stats(det), "same_point": same,
                      "kernels_ms": float(np.median([q["ms_kernels"] for q in parts])),
                      "redimension_ms": float(np.median([q["ms_redimension"] for q in parts])),
                      "inside_ms": float(np.median([q["ms_total"] for q in parts])),
                      "sigma_ratio": float(parts[0]["sigma"][case.d] / parts[0]["sigma"][case.d - 1])}
        q = res[state]
        q["project_below_detour_by_more_than_its_spread"] = bool(
            q["detour_ms"]["median"] - q["project_ms"]["median"] > q["detour_ms"]["max"] - q["detour_ms"]["min"])
    return res


def gram_only(da, rounds):
    """the two Gram paths on one X per workload size, for a kernel trace"""
    import ctypes as C
    from dcora_amd import capi
    for r, k in ((5, 10000), (4, 37094), (5, 400000)):
        X = np.random.default_rng(k).standard_normal((r, k))
        G = np.zeros(r * r)
        t_new, t_old = [], []
        for _ in range(rounds):
            t0 = time.perf_counter()
            capi.check(capi.lib().dcora_debug_project_gram(r, k, capi.F(X), G, None))
            t_new.append(1e3 * (time.perf_counter() - t0))
            n = k // 4
            t0 = time.perf_counter()
            da.project_solution_raslam(X[:, :4 * n], r, 3, n, 0, 0)  # (its first kernel is k_gram on the same X)
            t_old.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps({"r": r, "k": k, "one_pass_call_ms": stats(t_new), "host_fed_call_ms": stats(t_old)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--skip-lattice", action="store_true")
    ap.add_argument("--gram-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_project.txt"))
    a = ap.parse_args()
    import dcora_amd as da
    if da.device_count() < 1:
        raise SystemExit("session_project_cost needs a GPU")
    if a.gram_only:
        gram_only(da, a.rounds)
        return
    lines = ["project() in place against the detour through the host (tools/session_project_cost.py), ms, %d alternated "
             "rounds: median (min .. max)" % a.rounds, ""]
    fmt = lambda q: "%9.2f (%8.2f .. %8.2f)" % (q["median"], q["min"], q["max"])
    for kind in ("sphere", "tiers") + (() if a.skip_lattice else ("lattice",)):
        res = run_case(Case(da, kind), a.rounds)
        print(json.dumps(res), flush=True)
        lines.append("%s, %d -> %d, k = %d, sigma_%d / sigma_%d = %.3g" %
                     (res["case"], res["from_rank"], res["to_rank"], res["k"], res["to_rank"] + 1, res["to_rank"],
                      res["warm"]["sigma_ratio"]))
        for state in ("warm", "cold"):
            q = res[state]
            lines.append("  %s  detour %s   project %s   same point: %s" %
                         (state, fmt(q["detour_ms"]), fmt(q["project_ms"]), q["same_point"]))
            lines.append("        inside project (medians): kernels %.3f, re-dimensioning %.2f, total %.2f" %
                         (q["kernels_ms"], q["redimension_ms"], q["inside_ms"]))
            lines.append("        project below the detour by more than the detour rounds' spread: %s" %
                         q["project_below_detour_by_more_than_its_spread"])
        lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
