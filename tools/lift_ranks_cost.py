"""What the staircase's step costs a multi-rank job collectively (Exchange.lift) against the path a job had to take
before there was one: gather_X, every exchange and session destroyed, escapeSaddle of one host-fed whole-graph problem
at r + 1, sessions and exchanges created again at r + 1 (the shared segment, the IPC handles and the link check with
them), Exchange.set_X.

Workloads: sphere2500 / 5 agents from rank 5 at the seed-4 random point, tiers.pyfg (four robots) from rank 3 at a random
point; TWO ranks sharing ONE GPU (one GPU per rank is not measured).  (theta, v) comes from the host certificate,
outside the clock, the same for both paths and both ranks.  Two cache states, five alternated rounds each:
  cold  precond_cache_clear, then the job at r is created (not timed): the re-creating path pays the whole-graph
        preconditioner of its escapeSaddle, the collective lift has none to pay (it tests with the agents' own);
  warm  the second level, r + 1 -> r + 2 from the point the first step reached.
Times are rank 0's host clocks between two barriers of the job, around calls that end in a device synchronise.  Every
round checks that both paths reach the same point.

    python tools/lift_ranks_cost.py [--rounds K] [--out profiles/lift_ranks_cost.txt]

The parent starts one child per rank; rank 0 prints one JSON line per case and the parent writes the table."""
import argparse
import json
import os
import subprocess
import sys
import time
import uuid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

WORLD = 2


def stats(ms):
    ms = np.asarray(ms)
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max()), "rounds": int(ms.size)}


class Case:
    def __init__(self, da, kind, rank, job):
        import common
        self.da, self.kind, self.rank, self.job, self.serial = da, kind, rank, job, 0
        if kind == "pgo":
            self.name = "sphere2500 / 5 agents"
            self.ds = common.product_dataset("sphere2500")
            self.d, self.n, self.kw, self.block, self.r = self.ds.d, self.ds.n, {}, self.ds.d + 1, 5
            self.k = (self.d + 1) * self.n
            self.tol, self.Q, self.reg = (1e-6, 1e-6), da.build_Q_pgo(self.ds), 0.1
            self.X = common.random_point(self.r, self.d, self.n, 4, da.manifold_project)
        else:
            from test_raslam import ra_path
            self.name = "tiers.pyfg / 4 robots"
            self.ra = da.RADataset(ra_path("tiers"))
            ra = self.ra
            self.d, self.n, self.k, self.kw, self.block, self.r = ra.d, ra.n, ra.k, dict(l=ra.l, b=ra.b), 1, 3
            self.tol, self.Q, self.reg = (1e-4, 1e-4), ra.Q, None
            M = np.random.default_rng(4).uniform(-1, 1, (self.r, self.k))
            self.X = da.manifold_project(self.r, self.d, self.n, M, **self.kw)

    def make(self, r, reserve):
        """(session, exchange) of this rank at rank r; every call of every rank takes the next job name"""
        da = self.da
        self.serial += 1
        if self.kind == "pgo":
            s = da.RbcdSession(self.ds, num_robots=5, r=r, rank=self.rank, world_size=WORLD)
        else:
            s = da.RaRbcdSession(self.ra, r, rank=self.rank, world_size=WORLD,
                                 params=da.ROptParameters(RTR_iterations=200, RTR_tCG_iterations=200, gradnorm_tol=1e-4))
        if reserve:
            s.reserve_rank(reserve)
        return s, da.Exchange(s, "%s_%d" % (self.job, self.serial))

    def direction(self, r, X):
        da = self.da
        S = da.dual_certificate(r, self.d, self.n, X, self.Q, **self.kw)
        psd, theta, v, lmin = da.fast_verification(S, 1e-3, block=self.block)
        if psd:
            raise RuntimeError("%s: the certificate accepts the point, nothing to time" % self.name)
        return theta, v

    def recreate(self, s, ex, r, theta, v):
        """the path of a job without a collective lift; -> (ms, the new session and exchange)"""
        da = self.da
        ex.barrier()
        t0 = time.perf_counter()
        X = ex.gather_X()
        ex.close()
        s.close()
        if self.reg is None:
            self.reg = da.precond_regularization(self.Q)
        P = da.QuadraticProblem(r + 1, self.d, self.n, self.Q, reg=self.reg, **self.kw)
        Xn = P.escapeSaddle(X, theta, v, *self.tol)
        P.close()
        s, ex = self.make(r + 1, 0)
        ex.set_X(Xn)
        ex.barrier()
        return 1e3 * (time.perf_counter() - t0), s, ex

    def lift(self, ex, theta, v):
        ex.barrier()
        t0 = time.perf_counter()
        escaped, info = ex.lift(theta, v, *self.tol)
        ex.barrier()
        ms = 1e3 * (time.perf_counter() - t0)
        if not escaped:
            raise RuntimeError("%s: no escape" % self.name)
        return ms, info


def run_case(da, case, rounds):
    r, X = case.r, case.X
    theta, v = case.direction(r, X)
    res = {"case": case.name, "k": case.k, "from_rank": r, "ranks": WORLD}
    s, ex = case.make(r, r + 2)
    ex.set_X(X)
    case.lift(ex, theta, v)
    X1 = ex.gather_X()
    ex.close()
    s.close()
    theta1, v1 = case.direction(r + 1, X1)
    for state in ("cold", "warm"):
        rec, lif, split, same = [], [], [], True
        for i in range(rounds):
            for path in (("recreate", "lift") if i % 2 == 0 else ("lift", "recreate")):
                if state == "cold":
                    da.precond_cache_clear()
                    case.reg = None if case.kind == "ra" else case.reg
                    s, ex = case.make(r, r + 2 if path == "lift" else 0)
                    ex.set_X(X)
                    args = (r, theta, v)
                elif path == "lift":  # the job that made the first step itself
                    s, ex = case.make(r, r + 2)
                    ex.set_X(X)
                    case.lift(ex, theta, v)
                    args = (r + 1, theta1, v1)
                else:
                    s, ex = case.make(r + 1, 0)
                    ex.set_X(X1)
                    args = (r + 1, theta1, v1)
                if path == "recreate":
                    ms, s, ex = case.recreate(s, ex, *args)
                    rec.append(ms)
                    Xa = ex.gather_X()
                else:
                    ms, info = case.lift(ex, args[1], args[2])
                    lif.append(ms)
                    split.append(info)
                    Xb = ex.gather_X()
                ex.close()
                s.close()
            same = same and bool(np.abs(Xa - Xb).max() <= 1e-12 * np.abs(Xa).max())
        res[state] = {"recreate_ms": stats(rec), "lift_ms": stats(lif), "same_point": same,
                      "lift_redimension_ms": float(np.median([q["redimension_ms"] for q in split])),
                      "lift_inside_ms": float(np.median([q["total_ms"] for q in split])),
                      "lift_trials": int(split[0]["trials"])}
    return res


def fmt(q):
    return "%.1f (%.1f .. %.1f)" % (q["median"], q["min"], q["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_ranks_cost.txt"))
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--job", default="")
    a = ap.parse_args()
    if a.rank >= 0:  # one rank of the measurement
        import dcora_amd as da
        for kind in ("pgo", "ra"):
            res = run_case(da, Case(da, kind, a.rank, "%s%s" % (a.job, kind)), a.rounds)
            if a.rank == 0:
                print(json.dumps(res), flush=True)
        return
    job = "c%s" % uuid.uuid4().hex[:10]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(k), "--job", job, "--rounds",
                               str(a.rounds)], stdout=subprocess.PIPE if k == 0 else subprocess.DEVNULL, text=True)
             for k in range(WORLD)]
    try:  # (a rank that fails or never ends takes the others with it: none stays behind with the GPU open)
        out, _ = procs[0].communicate(timeout=1100)
        for p in procs[1:]:
            p.wait(timeout=120)
    except BaseException:
        for p in procs:
            p.kill()
        raise
    if any(p.returncode for p in procs):
        for p in procs:
            p.kill()
        raise SystemExit("a rank failed: %s" % [p.returncode for p in procs])
    results = [json.loads(line) for line in out.splitlines() if line.startswith("{")]
    lines = ["# tools/lift_ranks_cost.py: the collective lift against gather_X + destroy + host escapeSaddle + create at r + 1",
             "# + set_X; %d ranks sharing ONE MI355X (one GPU per rank is not measured), %d alternated rounds, ms on rank 0"
             % (WORLD, a.rounds),
             "# as median (min .. max) between two barriers of the job", ""]
    for res in results:
        print(json.dumps(res))
        for state in ("cold", "warm"):
            q = res[state]
            lines.append("%-24s %d -> %d  %-4s  re-create %-22s  lift %-20s  inside the lift %.1f, re-dimensioning %.1f,"
                         " trials %d, same point %s" %
                         (res["case"], res["from_rank"] + (state == "warm"), res["from_rank"] + 1 + (state == "warm"),
                          state, fmt(q["recreate_ms"]), fmt(q["lift_ms"]), q["lift_inside_ms"],
                          q["lift_redimension_ms"], q["lift_trials"], q["same_point"]))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
