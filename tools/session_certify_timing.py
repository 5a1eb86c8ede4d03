"""What certifying a live session costs, two ways, at the same iterate and with the symbolic analysis cached on both sides:
  (a) the host-fed calls: get_X + dual_certificate + fast_verification with a host Q;
  (b) RbcdSession.certify (dcora_rbcd_certify): X Q, Lambda, the values of S + eta I and the factorisation on the device.
Workloads: sphere2500 (5 agents, r = 5) at the converged iterate of the chordal start, and the planar lattice of 9216 poses
(1 agent, r = 3: the block-CSR central problem) after a few RBCD rounds from a random point.  Per workload and way: 3
warm-up calls, then 20 timed calls (wall clock around the call, which ends in a device synchronise); median, minimum and
maximum in ms.  Twice: the two ways alternating call by call, and each way in a block of its own calls.
python tools/session_certify_timing.py [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import common  # noqa: E402
import dcora_amd as da  # noqa: E402
from dcora_amd import synth  # noqa: E402

ETA, WARM, REPS = 1e-3, 3, 20


def host_fed(s, ds, r, Q):
    X = s.get_X()
    S = da.dual_certificate(r, ds.d, ds.n, X, Q)
    return da.fast_verification(S, ETA, block=ds.d + 1)[0]


def measure(tag, s, ds, r, Q, out):
    ways = (("host-fed", lambda: host_fed(s, ds, r, Q)), ("session", lambda: s.certify(ETA)[0]))
    verdict = {}

    def timed(name, fn, into):
        t0 = time.perf_counter()
        verdict[name] = bool(fn())
        into.append(1e3 * (time.perf_counter() - t0))

    alternating = {name: [] for name, _ in ways}
    for rep in range(WARM + REPS):
        for name, fn in ways:
            timed(name, fn, alternating[name] if rep >= WARM else [])
    blocks = {name: [] for name, _ in ways}
    for name, fn in ways:
        for rep in range(WARM + REPS):
            timed(name, fn, blocks[name] if rep >= WARM else [])
    info = s.certify(ETA)[4]
    for order, times in (("alternating", alternating), ("in blocks", blocks)):
        for name, _ in ways:
            t = np.array(times[name])
            out.append("%s %-11s %-8s psd %-5s median %8.3f ms  min %8.3f  max %8.3f  (%d calls after %d warm-up)" % (
                tag, order, name, verdict[name], np.median(t), t.min(), t.max(), REPS, WARM))
            print(out[-1], flush=True)
    out.append("%s session info: symbolic %.3f ms, numeric %.3f ms, look-up %.3f ms, arena %.1f MB, %d launches" % (
        tag, info["symbolic_ms"], info["numeric_ms"], info["lookup_ms"], info["arena_bytes"] / 1e6, info["launches"]))
    print(out[-1], flush=True)
    for order, times in (("alternating", alternating), ("in blocks", blocks)):
        for name, _ in ways:
            out.append("%s raw %s %s ms: %s" % (tag, order, name, " ".join("%.3f" % x for x in times[name])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if da.device_count() < 1:
        raise SystemExit("needs a GPU")
    out = []
    ds = common.product_dataset("sphere2500")
    r = 5
    X0 = np.zeros((r, 4 * ds.n)); X0[:3] = da.chordal_initialization(ds)
    s = da.RbcdSession(ds, num_robots=5, r=r)
    s.set_X(X0)
    run = s.run(max_iters=1000, rgrad_tol=0.1)
    out.append("sphere2500: %d RBCD iterations, |rgrad| %.3g, 2f %.4f" % (run["iters"], run["gradnorm"][-1], run["cost"][-1]))
    print(out[-1], flush=True)
    measure("sphere2500 k=%d" % (4 * ds.n), s, ds, r, da.build_Q_pgo(ds), out)
    s.close()
    ds = synth.lattice_se2()
    r = 3
    X0 = da.manifold_project(r, 2, ds.n, np.random.default_rng(3).uniform(-1, 1, (r, 3 * ds.n)))
    s = da.RbcdSession(ds, num_robots=1, r=r)
    s.set_X(X0)
    run = s.run(max_iters=3, rgrad_tol=0.0)
    out.append("lattice_se2 (%d poses): %d RBCD iterations, |rgrad| %.3g (not converged: the certificate is refused, "
               "both ways run the Lanczos stage)" % (ds.n, run["iters"], run["gradnorm"][-1]))
    print(out[-1], flush=True)
    measure("lattice9216 k=%d" % (3 * ds.n), s, ds, r, da.build_Q_pgo(ds), out)
    s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
