"""What a session and a job compute through the places where a hosted agent's block is read or written and where a
session changes rank -- gather_X, round, certify, lift, the rounds after it, project -- recorded as one .npz:

    python tools/record_session_blocks.py --lib PATH/libdcora_hip.so --out FILE    record what that build computes
    python tools/record_session_blocks.py [--lib PATH/libdcora_hip.so] --check FILE  recompute and compare bit for bit

tests/golden/session_blocks_parent.npz is the record of the commit BEFORE the agent's block, the rank change and the
drain were stated once in the session core, written with --lib pointing at a library built from that commit's sources;
tests/test_session_blocks_gpu.py recomputes the cases with the tree's library and wants every array equal.

The workloads are the smallest on which both orderings and both block placements occur: tinyGrid3D over 3 agents
(contiguous blocks of the mirror, SE ordering) and range_aided_slam_test_2d with its 2 robots (listed columns,
[rotations | unit spheres | translations | landmarks]), both at r = 3 from the usual seed-4 start.  Each runs
  single   one process: 4 iterations, get_X, round (anchor read on the device at poses 0 and n - 1, anchor from the
           host), certify, lift along its direction, X, 3 iterations, project, X
  ranks    a two-rank job, one process per rank: the same through the exchange (certify and certify_live; no project)
  robust   a two-rank robust job: 4 iterations, a collective weight update, certify_live on the weights it left, lift,
           3 iterations
Times in the info arrays are left out by index; everything else in them is kept.  A process loads ONE library, so the
choice is made before the package is used; the rank workers (tests/session_blocks_worker.py) are told the same one."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import uuid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

ETA = 1e-3
R0, PRE, POST, WORLD = 3, 4, 3, 2
GNC = dict(GNCBarc=10.0, GNCMuStep=2.0)
WORKLOADS = {"pgo": dict(kind="pgo", name="tinyGrid3D", R=3, tol=1e-6),
             "ra": dict(kind="ra", name="range_aided_slam_test_2d", tol=1e-4)}
MODES = ("single", "ranks", "robust")
CASES = ["%s/%s" % (w, m) for w in WORKLOADS for m in MODES]
WORKER = os.path.join(ROOT, "tests", "session_blocks_worker.py")
# info arrays without their times: certify's info8 and certify_live's info10 keep arena bytes, flops, levels, launches,
# logdet (certify_live: and the rounds)
CERT_KEPT, LIVE_KEPT = (2, 3, 4, 5, 6), (2, 3, 4, 5, 6, 8)


def use_library(path):
    import lib_window  # (the one way the tools choose a build)
    lib_window.use_library(path)


class Workload:
    def __init__(self, da, cfg):
        import common
        self.cfg, self.ra = cfg, cfg["kind"] == "ra"
        if self.ra:
            from test_raslam import ra_path
            self.ds = da.RADataset(ra_path(cfg["name"]))
            ds = self.ds
            self.d, self.n, self.l, self.b, self.k = ds.d, ds.n, ds.l, ds.b, ds.k
            M = np.random.default_rng(4).uniform(-1, 1, (R0, self.k))
            self.X0 = da.manifold_project(R0, self.d, self.n, M, l=self.l, b=self.b)
        else:
            self.ds = common.product_dataset(cfg["name"])
            self.d, self.n, self.l, self.b = self.ds.d, self.ds.n, 0, 0
            self.k = (self.d + 1) * self.n
            self.X0 = common.random_point(R0, self.d, self.n, 4, da.manifold_project)
        self.tol = dict(gradient_tolerance=cfg["tol"], preconditioned_gradient_tolerance=cfg["tol"])

    def host_Q(self, da):
        return self.ds.Q if self.ra else da.build_Q_pgo(self.ds)

    def anchor_of(self, X, pose):
        """the lifted pose `pose` of X, r x (d + 1): what round takes as an anchor from the host"""
        d, n, l = self.d, self.n, self.l
        if self.ra:
            cols = list(range(d * pose, d * pose + d)) + [d * n + l + pose]
        else:
            cols = list(range((d + 1) * pose, (d + 1) * (pose + 1)))
        return np.ascontiguousarray(X[:, cols])

    def session(self, da, robust=None, **kw):
        if self.ra:
            return da.RaRbcdSession(self.ds, R0, robust=robust, **kw)
        return da.RbcdSession(self.ds, num_robots=self.cfg["R"], r=R0, robust=robust, **kw)


def _put_round(out, tag, res):
    for key in ("trajectory", "unit_spheres", "landmarks"):
        if key in res:
            out[tag + "/" + key] = np.ascontiguousarray(res[key], dtype=np.float64)
    if "cost_2f" in res:
        out[tag + "/cost"] = np.array([res["cost_2f"], res["gradnorm"]])


def _put_lift(out, tag, escaped, info, r):
    out[tag] = np.array([float(escaped), float(info["trials"]), info["alpha"], info["f_before"], info["f_after"],
                         float(info.get("precond_built", 0)), float(r)])


def single(da, w):
    """one process -> dict of arrays"""
    out = {}
    s = w.session(da)
    s.set_X(w.X0)
    run = s.run(max_iters=PRE, rgrad_tol=0.0)
    out["pre/trace"] = np.array([run["cost"], run["gradnorm"], run["selected"].astype(np.float64)])
    X = s.get_X()
    out["X"] = X
    _put_round(out, "round/pose0", s.round(anchor_pose=0, cost=True))
    _put_round(out, "round/last", s.round(anchor_pose=w.n - 1))
    _put_round(out, "round/host", s.round(anchor=w.anchor_of(X, 1), cost=True))
    psd, theta, v, lmin, info = s.certify(ETA)
    assert not psd, "the certificate accepts the point: nothing to lift along"
    i8 = np.array([info[k] for k in ("symbolic_ms", "numeric_ms", "arena_bytes", "flops", "levels", "launches",
                                     "logdet", "lookup_ms")], dtype=np.float64)
    out["certify/scalars"] = np.array([float(psd), theta, lmin, float(info["matvecs"])])
    out["certify/info"] = i8[list(CERT_KEPT)]
    out["certify/v"] = v
    escaped, linfo = s.lift(theta, v, **w.tol)
    _put_lift(out, "lift/scalars", escaped, linfo, s.r)
    out["lift/X"] = s.get_X()
    run = s.run(max_iters=POST, rgrad_tol=0.0)
    out["post/trace"] = np.array([run["cost"], run["gradnorm"], run["selected"].astype(np.float64)])
    out["post/X"] = s.get_X()
    p = s.project()
    out["project/scalars"] = np.array([float(p["projected"]), float(p["reflected"]), float(p["positive_dets"]),
                                       p["gradnorm"], p["cost_2f"], float(p["gram_chunk"]), float(s.r)])
    out["project/sigma"], out["project/gram"] = p["sigma"], np.ascontiguousarray(p["gram"])
    out["project/basis"] = np.ascontiguousarray(p["basis"]) if p["projected"] else np.zeros(0)
    out["project/X"] = s.get_X()
    if not w.ra:
        out["launches"] = np.array([float(s.debug_launches())])
    s.close()
    return out


def ranked(da, w, rank, world, job, robust):
    """one rank of a job -> dict of arrays (what every rank returns is the same but where it says so)"""
    from dcora_amd import driver
    from dcora_amd import robust as rb
    out = {}
    kw = dict(rank=rank, world_size=world)
    if robust:
        prm = rb.RobustCostParameters("GNC_TLS", **GNC)
        if w.ra:
            s, ex = da.ra_robust_ranked_session(w.ds, job, R0, robust=prm, r_reserve=R0 + 1, **kw)
        else:
            s, ex = da.robust_ranked_session(w.ds, job, num_robots=w.cfg["R"], r=R0, robust=prm, r_reserve=R0 + 1, **kw)
    else:
        s = w.session(da, **kw)
        s.reserve_rank(R0 + 1)
        ex = da.Exchange(s, job)
    ex.set_X(w.X0)
    run = driver.exchange_run(ex, max_iters=PRE, rgrad_tol=0.0)
    out["pre/trace"] = np.array([run["cost"], run["gradnorm"], np.asarray(run["selected"], dtype=np.float64)])
    if robust:
        c = ex.update_weights()
        out["weights/counts"] = np.array([c["accepted"], c["rejected"], c["undecided"]], dtype=np.float64)
        out["weights/w"] = ex.get_weights()
    X = ex.gather_X()
    out["X"] = X
    _put_round(out, "round/pose0", ex.round(anchor_pose=0))
    _put_round(out, "round/last", ex.round(anchor_pose=w.n - 1))
    _put_round(out, "round/host", ex.round(anchor=w.anchor_of(X, 1)))
    if not robust:  # (the host certificate takes the job's Q: the creation weights)
        cert, theta, lmin, v, mv, dist = ex.certify(w.host_Q(da) if rank == 0 else None, ETA, w.k)
        out["certify/scalars"] = np.array([float(cert), theta, lmin, float(mv), float(dist)])
        out["certify/v"] = v
    cert, theta, lmin, v, mv, dist, info = ex.certify_live(ETA)
    assert not cert, "the certificate accepts the point: nothing to lift along"
    out["certify_live/scalars"] = np.array([float(cert), theta, lmin, float(mv), float(dist)])
    out["certify_live/info"] = np.asarray(info["info10"], dtype=np.float64)[list(LIVE_KEPT)]
    out["certify_live/v"] = v
    escaped, linfo = ex.lift(theta, v, **w.tol)
    _put_lift(out, "lift/scalars", escaped, linfo, s.r)
    out["lift/X"] = ex.gather_X()
    run = driver.exchange_run(ex, max_iters=POST, rgrad_tol=0.0)
    out["post/trace"] = np.array([run["cost"], run["gradnorm"], np.asarray(run["selected"], dtype=np.float64)])
    out["post/X"] = ex.gather_X()
    if not w.ra:
        out["launches/rank%d" % rank] = np.array([float(s.debug_launches())])
    ex.barrier()
    ex.close()
    s.close()
    return out


def run_ranks(workload, robust, lib=None, timeout=240):
    """the two-rank job, one process per rank -> the ranks' dicts"""
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "job.json"), "w") as f:
            json.dump(dict(workload=workload, robust=bool(robust), lib=lib), f)
        job = "b%s" % uuid.uuid4().hex[:12]
        env = dict(os.environ)
        env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
        env["DCORA_EXCHANGE_TIMEOUT_S"] = "60"
        env.pop("DCORA_EXCHANGE_WAIT", None)
        env.pop("DCORA_EXCHANGE", None)
        procs = [subprocess.Popen([sys.executable, WORKER, str(k), str(WORLD), job, d], env=env, stdout=subprocess.PIPE,
                                  stderr=subprocess.STDOUT) for k in range(WORLD)]
        outs = []
        for p in procs:
            try:
                o, _ = p.communicate(timeout=timeout)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            outs.append(o.decode(errors="replace"))
        for k, p in enumerate(procs):
            if p.returncode != 0:
                raise RuntimeError("rank %d failed (%d):\n%s" % (k, p.returncode, outs[k][-3000:]))
        return [dict(np.load(os.path.join(d, "rank%d.npz" % k))) for k in range(WORLD)]


def compute_case(case, lib=None):
    """one of CASES -> {case/name: array}; a two-rank case keeps rank 0's arrays and, under rank1/, those of rank 1
    that are its own (every other one must equal rank 0's, which is asserted here)"""
    workload, mode = case.split("/")
    if mode == "single":
        import dcora_amd as da
        if da.device_count() < 1:
            raise SystemExit("no GPU visible: these cases run on the device")
        got = single(da, Workload(da, WORKLOADS[workload]))
    else:
        r0, r1 = run_ranks(workload, mode == "robust", lib)
        got = dict(r0)
        for k, v in r1.items():
            if k not in r0:
                got[k] = v
            elif not (v.shape == r0[k].shape and np.array_equal(v.view(np.uint64), r0[k].view(np.uint64))):
                raise RuntimeError("%s: the ranks disagree on %s" % (case, k))
    return {case + "/" + k: np.ascontiguousarray(v, dtype=np.float64) for k, v in got.items()}


def compute(lib=None, cases=CASES):
    out = {}
    for case in cases:
        out.update(compute_case(case, lib))
    return out


def differing(got, want):
    """names of the arrays that are not equal bit for bit (or are missing on one side)"""
    bad = sorted(set(got) ^ set(want))
    for k in sorted(set(got) & set(want)):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape or not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
            bad.append(k)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--check", default=None)
    a = ap.parse_args()
    lib = os.path.abspath(a.lib) if a.lib else None
    if lib:
        use_library(lib)
    got = compute(lib)
    for k in sorted(got):
        if k.endswith("/scalars") or k.endswith("/trace") or "launches" in k:
            print(k, got[k].tolist())
    if a.out:
        np.savez_compressed(a.out, **got)
        print("wrote", a.out, os.path.getsize(a.out), "bytes,", len(got), "arrays")
    if a.check:
        bad = differing(got, dict(np.load(a.check)))
        print("arrays that differ from %s: %s" % (a.check, bad if bad else "none of %d" % len(got)))
        if bad:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
