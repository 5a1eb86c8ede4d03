"""What the projection to rank d costs a multi-rank job collectively (Exchange.project) against the path a job had to
take before there was one: gather_X, the host-fed projection (dcora_round_project_solution_raslam), every exchange and
session destroyed, sessions and exchanges created again at rank d (the shared segment, the IPC handles and the link
check with them), Exchange.set_X.

Workloads: sphere2500 / 5 agents at rank 5 at the seed-4 random point, tiers.pyfg (four robots) at rank 3 at a random
point; TWO ranks sharing ONE GPU (one GPU per rank is not measured).  Two cache states, alternated rounds each:
  cold  precond_cache_clear before the job at r is created (not timed): the re-creating path builds the agents'
        preconditioners again at rank d;
  warm  the cache holds them.
Times are rank 0's host clocks between two barriers of the job.  Also:
  transports  the per-agent Gram matrices through the segment's X area against allreduce_sum pieces (the debug hook),
              the whole of Exchange.project on smallGrid3D with R in {5, 8} agents at r in {5, 16};
  gram        the block-list launch pair against a loop of the single-block pair over the same blocks, in event time
              (one process): sphere2500 / 5 agents and a 100k-pose lattice / 8 agents.

    python tools/project_ranks_cost.py [--rounds K] [--out profiles/project_ranks_cost.txt]

The parent starts one child per rank; rank 0 prints one JSON line per case and the parent writes the table."""
import argparse
import ctypes as C
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
    def __init__(self, da, kind, rank, job, R=5, r=None):
        import common
        self.da, self.kind, self.rank, self.job, self.serial, self.R = da, kind, rank, job, 0, R
        if kind in ("pgo", "small"):
            name = "sphere2500" if kind == "pgo" else "smallGrid3D"
            self.name = "%s / %d agents" % (name, R)
            self.ds = common.product_dataset(name)
            self.d, self.n, self.l, self.b, self.r = self.ds.d, self.ds.n, 0, 0, r or 5
            self.k = (self.d + 1) * self.n
            self.X = common.random_point(self.r, self.d, self.n, 4, da.manifold_project)
        else:
            from test_raslam import ra_path
            self.name = "tiers.pyfg / 4 robots"
            self.ra = da.RADataset(ra_path("tiers"))
            ra = self.ra
            self.d, self.n, self.l, self.b, self.k, self.r = ra.d, ra.n, ra.l, ra.b, ra.k, r or 3
            M = np.random.default_rng(4).uniform(-1, 1, (self.r, self.k))
            self.X = da.manifold_project(self.r, self.d, self.n, M, l=ra.l, b=ra.b)

    def make(self, r):
        da = self.da
        self.serial += 1
        if self.kind == "ra":
            s = da.RaRbcdSession(self.ra, r, rank=self.rank, world_size=WORLD,
                                 params=da.ROptParameters(RTR_iterations=200, RTR_tCG_iterations=200, gradnorm_tol=1e-4))
        else:
            s = da.RbcdSession(self.ds, num_robots=self.R, r=r, rank=self.rank, world_size=WORLD)
        return s, da.Exchange(s, "%s_%d" % (self.job, self.serial))

    def host_project(self, X):
        import session_project_inputs as spi
        import session_round_inputs as sri
        da = self.da
        if self.kind == "ra":
            return da.project_solution_raslam(X, X.shape[0], self.d, self.n, self.l, self.b)
        P = da.project_solution_raslam(spi.ra_from_se(X, self.d, self.n), X.shape[0], self.d, self.n, 0, 0)
        return sri.se_from_ra(P, self.d, self.n, 0)

    def recreate(self, s, ex):
        """the path of a job without a collective projection; -> (ms, the new session and exchange)"""
        ex.barrier()
        t0 = time.perf_counter()
        X = ex.gather_X()
        P = self.host_project(X)
        ex.close()
        s.close()
        s, ex = self.make(self.d)
        ex.set_X(P)
        ex.barrier()
        return 1e3 * (time.perf_counter() - t0), s, ex

    def project(self, ex):
        ex.barrier()
        t0 = time.perf_counter()
        out = ex.project()
        ex.barrier()
        return 1e3 * (time.perf_counter() - t0), out


def run_case(da, case, rounds):
    res = {"case": case.name, "k": case.k, "from_rank": case.r, "ranks": WORLD}
    for state in ("cold", "warm"):
        rec, pro, inside, same = [], [], [], True
        for i in range(rounds):
            for path in (("recreate", "project") if i % 2 == 0 else ("project", "recreate")):
                if state == "cold":
                    da.precond_cache_clear()
                s, ex = case.make(case.r)
                ex.set_X(case.X)
                if path == "recreate":
                    ms, s, ex = case.recreate(s, ex)
                    rec.append(ms)
                    Xa = ex.gather_X()
                else:
                    ms, out = case.project(ex)
                    pro.append(ms)
                    inside.append(out)
                    Xb = ex.gather_X()
                ex.close()
                s.close()
            same = same and bool(np.abs(Xa.T @ Xa - Xb.T @ Xb).max() <= 1e-10)  # (the gauge may differ)
        res[state] = {"recreate_ms": stats(rec), "project_ms": stats(pro), "same_point": same,
                      "kernels_ms": float(np.median([q["ms_kernels"] for q in inside])),
                      "redimension_ms": float(np.median([q["ms_redimension"] for q in inside])),
                      "inside_ms": float(np.median([q["ms_total"] for q in inside]))}
    return res


def run_transports(da, rank, job, rounds):
    from dcora_amd import capi
    out = []
    for R in (5, 8):
        for r in (5, 16):
            case = Case(da, "small", rank, "%st%d_%d" % (job, R, r), R=R, r=r)
            ms = {0: [], 1: []}
            for i in range(rounds):
                for sums in ((0, 1) if i % 2 == 0 else (1, 0)):
                    capi.check(capi.lib().dcora_debug_exchange_project_sums(sums))
                    s, ex = case.make(r)
                    ex.set_X(case.X)
                    ms[sums].append(case.project(ex)[0])
                    ex.close()
                    s.close()
            capi.check(capi.lib().dcora_debug_exchange_project_sums(0))
            out.append({"transport": "smallGrid3D", "R": R, "r": r, "area_ms": stats(ms[0]), "sums_ms": stats(ms[1])})
    return out


def run_gram(da, reps):
    from dcora_amd import capi
    out = []
    for name, r, ks in (("sphere2500 / 5 agents", 5, [2000] * 5), ("100k-pose lattice / 8 agents", 5, [50000] * 8)):
        k = np.array(ks, np.int64)
        loop, pair = np.zeros(reps), np.zeros(reps)
        capi.check(capi.lib().dcora_debug_project_gram_time(r, len(ks), k.ctypes.data_as(C.c_void_p), reps, loop, pair))
        out.append({"gram": name, "r": r, "loop_us": stats(loop), "pair_us": stats(pair)})
    return out


def fmt(q, f="%.1f"):
    return (f + " (" + f + " .. " + f + ")") % (q["median"], q["min"], q["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_ranks_cost.txt"))
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--job", default="")
    a = ap.parse_args()
    if a.rank >= 0:  # one rank of the measurement
        import dcora_amd as da
        results = [run_case(da, Case(da, kind, a.rank, "%s%s" % (a.job, kind)), a.rounds) for kind in ("pgo", "ra")]
        results += run_transports(da, a.rank, a.job, a.rounds)
        if a.rank == 0:
            for res in results:
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
    import dcora_amd as da
    results = [json.loads(line) for line in out.splitlines() if line.startswith("{")] + run_gram(da, 10)
    lines = ["# tools/project_ranks_cost.py: the collective projection against gather_X + host-fed projection + destroy +",
             "# create at rank d + set_X; %d ranks sharing ONE MI355X (one GPU per rank is not measured), %d alternated"
             % (WORLD, a.rounds),
             "# rounds, ms on rank 0 as median (min .. max) between two barriers of the job", ""]
    for res in results:
        print(json.dumps(res))
        if "case" in res:
            for state in ("cold", "warm"):
                q = res[state]
                lines.append("%-24s %d -> d  %-4s  re-create %-22s  project %-20s  inside %.2f: kernels %.3f, "
                             "re-dimensioning %.2f; same point %s" %
                             (res["case"], res["from_rank"], state, fmt(q["recreate_ms"]), fmt(q["project_ms"], "%.2f"),
                              q["inside_ms"], q["kernels_ms"], q["redimension_ms"], q["same_point"]))
        elif "transport" in res:
            lines.append("per-agent Gram matrices, %s R = %d r = %-2d  Exchange.project: X area %-22s  allreduce_sum pieces %s"
                         % (res["transport"], res["R"], res["r"], fmt(res["area_ms"], "%.2f"), fmt(res["sums_ms"], "%.2f")))
        else:
            lines.append("Gram launch pair, %-28s r = %d, us from events: loop of launch_gram %-22s  block list %s" %
                         (res["gram"], res["r"], fmt(res["loop_us"]), fmt(res["pair_us"])))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
