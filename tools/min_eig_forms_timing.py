"""Milliseconds per call of the three clients of the certificate's eigensolver, for ONE build of the library or for two
builds in alternated processes (a process loads one libdcora_hip.so):

    python tools/min_eig_forms_timing.py [--lib PATH/libdcora_hip.so]            one build -> one JSON line
    python tools/min_eig_forms_timing.py --against PATH/libdcora_hip.so [--rounds 2] [--out FILE]
                                          that build and the tree's, alternated `rounds` times each -> a table

  min_eig   dcora_cert_min_eig (tol 1e-6) on the indefinite certificate of sphere2500 at a seeded random point, r = 5
  reg       dcora_graph_precond_regularization on the first robot's Q of tiers.pyfg
  live      a refused dcora_exchange_certify_live (eta 1e-3) on two ranks sharing the GPU, smallGrid3D / 5 agents, r = 3,
            after 4 iterations from a seeded random point; rank 0's clock
Each: CALLS calls after WARM warm-ups per process.  The table gives median and min - max over all of a build's calls."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import uuid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

WARM, CALLS, WORLD = 3, 10, 2
LIVE = dict(kind="pgo", name="smallGrid3D", R=5, tol=1e-6)


def timed(fn):
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms


def rank_main(rank, job, out_dir, lib):
    import record_session_blocks as rec
    if lib:
        rec.use_library(lib)
    import dcora_amd as da
    from dcora_amd import driver
    w = rec.Workload(da, LIVE)
    s = w.session(da, rank=rank, world_size=WORLD)
    ex = da.Exchange(s, job)
    ex.set_X(w.X0)
    driver.exchange_run(ex, max_iters=4, rgrad_tol=0.0)
    assert not ex.certify_live(1e-3)[0]
    ms = timed(lambda: ex.certify_live(1e-3))
    ex.barrier()
    ex.close()
    s.close()
    json.dump(ms, open(os.path.join(out_dir, "rank%d.json" % rank), "w"))


def one_build(lib):
    import record_session_blocks as rec
    if lib:
        rec.use_library(lib)
    import common
    import dcora_amd as da
    from test_raslam import ra_path
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the device")
    out = {"lib": lib or "tree"}
    ds = common.product_dataset("sphere2500")
    X = da.manifold_project(5, ds.d, ds.n, np.random.default_rng(4).standard_normal((5, 4 * ds.n)))
    S = da.dual_certificate(5, ds.d, ds.n, X, da.build_Q_pgo(ds))
    out["min_eig"] = timed(lambda: da.min_eig(S, tol=1e-6))
    ra = da.RADataset(ra_path("tiers"))
    Qa = ra.agent_blocks(ra.robots[0])[2]
    out["reg"] = timed(lambda: da.precond_regularization(Qa))
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", DCORA_EXCHANGE_TIMEOUT_S="60")
        job = "t%s" % uuid.uuid4().hex[:12]
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(k), "--job", job, "--dir", d] +
                                  (["--lib", lib] if lib else []), env=env) for k in range(WORLD)]
        codes = [p.wait(timeout=300) for p in procs]
        if any(codes):
            raise SystemExit("a rank failed: %s" % codes)
        out["live"] = json.load(open(os.path.join(d, "rank0.json")))
    return out


def against(parent, rounds, out_path):
    runs = {"parent": [], "tree": []}
    for _ in range(rounds):
        for tag, lib in (("parent", parent), ("tree", None)):
            cmd = [sys.executable, os.path.abspath(__file__)] + (["--lib", lib] if lib else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise SystemExit(res.stdout[-2000:] + res.stderr[-2000:])
            runs[tag].append(json.loads(res.stdout.strip().splitlines()[-1]))
    lines = ["ms per call, %d alternated processes per build, %d calls after %d warm-ups in each" % (rounds, CALLS, WARM),
             "%-8s %-7s %9s %9s %9s   verdict" % ("what", "build", "median", "min", "max")]
    for what in ("min_eig", "reg", "live"):
        spread = {}
        for tag in ("parent", "tree"):
            ms = np.concatenate([r[what] for r in runs[tag]])
            spread[tag] = (float(np.median(ms)), float(ms.min()), float(ms.max()))
        for tag in ("parent", "tree"):
            inside = spread["parent"][1] <= spread["tree"][0] <= spread["parent"][2]
            lines.append("%-8s %-7s %9.3f %9.3f %9.3f   %s" % ((what, tag) + spread[tag] + (
                "" if tag == "parent" else "median %s the parent's spread" % ("inside" if inside else "OUTSIDE"),)))
    text = "\n".join(lines)
    print(text)
    if out_path:
        open(out_path, "w").write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--against", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rank", type=int, default=None)
    ap.add_argument("--job", default=None)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    lib = os.path.abspath(a.lib) if a.lib else None
    if a.rank is not None:
        rank_main(a.rank, a.job, a.dir, lib)
    elif a.against:
        against(os.path.abspath(a.against), a.rounds, a.out)
    else:
        print(json.dumps(one_build(lib)), flush=True)


if __name__ == "__main__":
    main()
