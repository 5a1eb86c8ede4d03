"""What the last step of a solve costs, two ways, at the same iterate:
  (a) the host-fed calls: get_X + align_lifted_trajectory_to_frame (dcora_round_align_trajectory: X down, X up again,
      the frame on the host, k_align_poses with one thread per pose, a device-wide synchronise, the result down);
  (b) RbcdSession.round (dcora_rbcd_round: k_round_states on the session's stream from the mirror, the result down),
      without the rounded cost and with it.
Workloads: sphere2500 / 5 agents / r = 5 three RBCD iterations from the chordal start, and the synthetic 100k-pose SE(3)
lattice / 8 agents / r = 5 three iterations from the seed-20250310 random point (bench.py's config 5).  Across ranks:
Exchange.round against gather_X + the host-fed rounding, sphere2500 on TWO ranks sharing ONE GPU (one GPU per rank is
not measured).  Per workload and way: 3 warm-up calls, then 20 timed calls, the ways alternating call by call; host clock
around calls that end in a synchronise (across ranks: rank 0's, between two barriers of the job); median (min .. max) ms.

    python tools/session_round_cost.py [--out profiles/session_round.txt] [--resource-usage FILE] [--no-lattice]
    python tools/session_round_cost.py --kernels      (the lattice alone, 5 calls each way: for a
                                                       rocprofv3 --kernel-trace --stats run of its own)

--resource-usage: the remarks of hipcc -Rpass-analysis=kernel-resource-usage on csrc/session_round.hip, condensed into
the head of the file.  The parent starts one child per rank for the ranks' part."""
import argparse
import json
import os
import re
import subprocess
import sys
import time
import uuid

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, REPS, WORLD = 3, 20, 2


def fmt(ms):
    ms = np.asarray(ms)
    return "%8.3f (%.3f .. %.3f)" % (np.median(ms), ms.min(), ms.max())


def alternate(ways, before=None):
    times = {name: [] for name, _ in ways}
    for rep in range(WARM + REPS):
        for name, fn in ways:
            if before:
                before()
            t0 = time.perf_counter()
            fn()
            if rep >= WARM:
                times[name].append(1e3 * (time.perf_counter() - t0))
    return times


def sphere_session(da, **kw):
    import common
    ds = common.product_dataset("sphere2500")
    X0 = np.zeros((5, 4 * ds.n)); X0[:3] = da.chordal_initialization(ds)
    return ds, da.RbcdSession(ds, num_robots=5, r=5, **kw), X0


def lattice_session(da):
    from dcora_amd import synth
    ds = synth.lattice_se3()
    X0 = da.manifold_project(5, ds.d, ds.n, np.random.default_rng(20250310).uniform(-1, 1, (5, (ds.d + 1) * ds.n)))
    return ds, da.RbcdSession(ds, num_robots=8, r=5), X0


def host_fed(da, X, d, n):
    return da.align_lifted_trajectory_to_frame(X, X[:, :d + 1], d, n, True)


def measure(da, tag, ds, s, X0, out):
    d, n = ds.d, ds.n
    s.set_X(X0)
    s.run(max_iters=3, rgrad_tol=0.0)
    ways = (("host-fed", lambda: host_fed(da, s.get_X(), d, n)), ("round", lambda: s.round()),
            ("round+cost", lambda: s.round(cost=True)))
    t = alternate(ways)
    a, b = s.round(cost=True), host_fed(da, s.get_X(), d, n)
    out.append("%-28s (a) get_X + host-fed %s   (b) round %s   (b) with the cost %s   ms" %
               (tag, fmt(t["host-fed"]), fmt(t["round"]), fmt(t["round+cost"])))
    out.append("%-28s inside round+cost: kernels %.3f ms, evaluation %.3f ms, total %.3f ms; rounded 2f %.6f, |rgrad| "
               "%.3g; max |trajectory - host-fed| %.2e" % ("", a["info"]["kernel_ms"], a["info"]["eval_ms"],
                                                          a["info"]["ms"], a["cost_2f"], a["gradnorm"],
                                                          np.abs(a["trajectory"] - b).max()))
    spread = max(t["host-fed"]) - min(t["host-fed"])
    out.append("%-28s (b) below (a) by %.3f ms; (a)'s own spread %.3f ms: %s" %
               ("", np.median(t["host-fed"]) - np.median(t["round"]), spread,
                "below by more than the spread" if np.median(t["host-fed"]) - np.median(t["round"]) > spread
                else "NOT below by more than the spread"))
    for line in out[-3:]:
        print(line, flush=True)


def rank_main(rank, job):
    import dcora_amd as da
    from dcora_amd import driver
    ds, s, X0 = sphere_session(da, rank=rank, world_size=WORLD)
    ex = da.Exchange(s, job)
    ex.set_X(X0)
    driver.exchange_run(ex, max_iters=3, rgrad_tol=0.0)
    ways = (("gather", lambda: host_fed(da, ex.gather_X(), ds.d, ds.n)), ("round", lambda: ex.round()))
    t = alternate(ways, before=ex.barrier)
    same = float(np.abs(ex.round()["trajectory"] - host_fed(da, ex.gather_X(), ds.d, ds.n)).max())
    ex.barrier()
    ex.close()
    s.close()
    if rank == 0:
        print("JSON " + json.dumps({"gather": t["gather"], "round": t["round"], "same": same}), flush=True)


def resource_table(path):
    rows, name = [], None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
            name = re.sub(r"\(.*", "", name.replace("dcora::(anonymous namespace)::", "").replace("void ", ""))
            rows.append([name, {}])
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and rows:
            rows[-1][1][m.group(1).split(" [")[0]] = int(m.group(2))
    return ["  %-52s VGPRs %3d  SGPRs %3d  scratch %d B/lane  LDS %4d B/block  occupancy %d waves/SIMD" %
            (n, u["VGPRs"], u["TotalSGPRs"], u["ScratchSize"], u["LDS Size"], u["Occupancy"]) for n, u in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--resource-usage", default=None)
    ap.add_argument("--no-lattice", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rank", type=int, default=None)
    ap.add_argument("--job", default=None)
    a = ap.parse_args()
    if a.rank is not None:
        return rank_main(a.rank, a.job)
    import dcora_amd as da
    if da.device_count() < 1:
        raise SystemExit("needs a GPU")
    if a.kernels:
        ds, s, X0 = lattice_session(da)
        s.set_X(X0)
        s.run(max_iters=3, rgrad_tol=0.0)
        for _ in range(5):
            s.round()
            host_fed(da, s.get_X(), ds.d, ds.n)
        s.close()
        return
    out = ["# tools/session_round_cost.py: the last step of a solve, (a) get_X + dcora_round_align_trajectory against (b)",
           "# dcora_rbcd_round on the live session; one MI355X, %d calls after %d warm-up, the ways alternating call by "
           "call," % (REPS, WARM), "# host clock around calls that end in a synchronise; ms as median (min .. max)", ""]
    if a.resource_usage:
        out += ["hipcc -Rpass-analysis=kernel-resource-usage, gfx950 (k_round_states / k_round_points, csrc/session_round.hip):"]
        out += resource_table(a.resource_usage) + [""]
    ds, s, X0 = sphere_session(da)
    measure(da, "sphere2500 / 5 agents / r=5", ds, s, X0, out)
    s.close()
    if not a.no_lattice:
        ds, s, X0 = lattice_session(da)
        measure(da, "lattice 100k / 8 agents / r=5", ds, s, X0, out)
        s.close()
    job = "rc%s" % uuid.uuid4().hex[:10]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", DCORA_EXCHANGE_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(k), "--job", job], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for k in range(WORLD)]
    texts = [p.communicate(timeout=600)[0] for p in procs]
    if any(p.returncode for p in procs):
        raise SystemExit("a rank failed:\n" + "\n".join(t[-2000:] for t in texts))
    rec = json.loads([ln for ln in texts[0].splitlines() if ln.startswith("JSON ")][0][5:])
    out += ["", "across ranks, sphere2500 / 5 agents / r=5, %d ranks sharing ONE GPU (one GPU per rank is not measured), rank "
            "0's clock between two barriers:" % WORLD,
            "%-28s gather_X + host-fed %s   Exchange.round %s   ms; max |difference| %.2e" %
            ("", fmt(rec["gather"]), fmt(rec["round"]), rec["same"])]
    print("\n".join(out[-2:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
