"""What the certificate's eigensolver computes -- the Lanczos runs and the plan of computeMinimumEigenPair around them --
recorded as one .npz:

    python tools/record_min_eig.py --lib PATH/libdcora_hip.so --out FILE      record what that build computes
    python tools/record_min_eig.py [--lib PATH/libdcora_hip.so] --check FILE  recompute and compare bit for bit

tests/golden/min_eig_parent.npz is the record of the commit BEFORE the thick-restart recurrence (lanczos_restart.h) and
the plan (min_eig_plan.h) were stated once, written with --lib pointing at a library built from that commit's sources;
tests/test_min_eig_forms_gpu.py recomputes the cases with the tree's library and wants every array equal.

  single/device, single/sync   one process each (the cycle kept on the device; DCORA_LANCZOS=sync, the per-step form),
      dcora_cert_min_eig on
        grid      the indefinite certificate of smallGrid3D at a seeded random point, r = 3 (with the launches of the
                  call), tol 1e-3: lambda_lm = 1166, the spectrum-shifted run delivers
        zero, two_i, diag   the matrices of test_kernel_forms_gpu.py's Lanczos test: a norm that vanishes at step 0
                  (done_zero), a remainder that is rounding noise (the shifted run), three distinct eigenvalues (at its
                  tol of 1e-8 the shortcut, the first shift converges)
        neg_diag  the negated diagonal: the first run ends negative
        huge      lambda_min = -50 under lambda_lm = 4e6 (test_gpu_parity.py): the shortcut, then the ladder OUTWARD
                  (-10 refused, -100 factors and converges)
        drone     single_drone.pyfg.gz minus 1e-3 I, lambda_lm = 2e4 at tol 1e-4: the shortcut, then 3150 solves of the
                  inverse run at the first shift, which converges
        drone_inward   0.05 Q of single_drone minus 1e-3 I, lambda_lm = 999: the shifted run spends its 1000 restarts
                  (10 020 matvecs), so do the inverse runs at -10, -5 and -2.5: the ladder moves INWARD to -1.25, which
                  converges after 7260 solves (3 s; the count returned, 17 300, leaves the three
                  inverse runs that did not deliver out)
      and dcora_graph_precond_regularization on the agents' Q of range_aided_slam_test_2d
  ranks/pgo, ranks/ra   a two-rank job, one process per rank (tests/min_eig_forms_worker.py), on tinyGrid3D / 3 agents
      and range_aided_slam_test_2d (scattered rows: row_map): certify and certify_live at eta = 1e-3 (the collective
      runs deliver: distributed = 1) and certify_live at eta = 1e-7 (eta / lambda_lm < 1e-8: the collective shortcut to
      rank 0's fallback, distributed = 0)
Per case: ok, lambda, matvecs (the rank cases: certified, theta, lambda, matvecs, distributed) and v.  A process loads
ONE library, so the choice is made before the package is used; the children are told the same one."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import record_session_blocks as rec  # noqa: E402  (the workloads of the rank cases, use_library, differing)

ETA, ETA_SMALL = 1e-3, 1e-7
PRE, WORLD = 4, 2
FORMS = {"device": {}, "sync": {"DCORA_LANCZOS": "sync"}}
MATRICES = ("grid", "zero", "two_i", "diag", "neg_diag", "huge", "drone", "drone_inward")
CASES = ["single/%s" % f for f in FORMS] + ["ranks/%s" % w for w in rec.WORKLOADS]
WORKER = os.path.join(ROOT, "tests", "min_eig_forms_worker.py")


def matrices(da):
    """name -> (Csr, tol)"""
    import common
    import scipy.sparse as sp
    out = {}
    ds = common.product_dataset("smallGrid3D")
    X = da.manifold_project(3, ds.d, ds.n, np.random.default_rng(4).standard_normal((3, 4 * ds.n)))
    out["grid"] = (da.dual_certificate(3, ds.d, ds.n, X, da.build_Q_pgo(ds)), 1e-3)  # (1e-6 / 1166 would be hopeless)
    n = 400
    out["zero"] = (da.Csr.from_scipy(sp.csr_matrix((np.zeros(n), (np.arange(n), np.arange(n))), shape=(n, n))), 1e-6)
    out["two_i"] = (da.Csr.from_scipy((2.0 * sp.identity(n)).tocsr()), 1e-6)
    three = np.r_[-2.0, np.ones(200), 3.0 * np.ones(199)]
    out["diag"] = (da.Csr.from_scipy(sp.diags(three).tocsr()), 1e-8)
    out["neg_diag"] = (da.Csr.from_scipy(sp.diags(-three).tocsr()), 1e-8)
    d = np.concatenate(([-50.0], np.random.default_rng(5).uniform(1.0, 30.0, n - 2), [4e6]))
    A = sp.diags(d).tocsr()
    for off in (0, 1):  # an orthogonal similarity that keeps the matrix sparse: plane rotations on neighbouring pairs
        c, s_ = np.cos(0.7), np.sin(0.7)
        blocks = [np.array([[c, -s_], [s_, c]])] * ((n - off) // 2)
        G = sp.block_diag(([np.eye(1)] if off else []) + blocks + ([np.eye(1)] if (n - off) % 2 else []), format="csr")
        A = (G @ A @ G.T).tocsr()
    A = ((A + A.T) * 0.5).tocsr()
    A.sort_indices()
    out["huge"] = (da.Csr.from_scipy(A), 1e-3)
    Q = da.RADataset(os.path.join(common.DATA, "single_drone.pyfg.gz")).Q.to_scipy()
    out["drone"] = (da.Csr.from_scipy((Q - 1e-3 * sp.identity(Q.shape[0])).tocsr()), 1e-4)
    out["drone_inward"] = (da.Csr.from_scipy((0.05 * Q - 1e-3 * sp.identity(Q.shape[0])).tocsr()), 1e-4)
    return out


def single(da):
    """one process, one form of the Lanczos cycle -> dict of arrays"""
    from test_raslam import ra_path
    out = {}
    for name, (S, tol) in matrices(da).items():
        n0 = da.debug_launch_count()
        ok, lam, v, mv = da.min_eig(S, tol=tol)
        if name == "grid":
            out["grid/launches"] = np.array([float(da.debug_launch_count() - n0)])
        out[name + "/scalars"] = np.array([float(ok), lam, float(mv)])
        out[name + "/v"] = v
    ra = da.RADataset(ra_path("range_aided_slam_test_2d"))
    out["reg"] = np.array([da.precond_regularization(ra.agent_blocks(robot)[2]) for robot in ra.robots])
    return out


def ranked(da, w, rank, world, job):
    """one rank of a job -> dict of arrays (the same on every rank)"""
    from dcora_amd import driver
    out = {}
    s = w.session(da, rank=rank, world_size=world)
    ex = da.Exchange(s, job)
    ex.set_X(w.X0)
    driver.exchange_run(ex, max_iters=PRE, rgrad_tol=0.0)
    cert, theta, lmin, v, mv, dist = ex.certify(w.host_Q(da) if rank == 0 else None, ETA, w.k)
    out["certify/scalars"], out["certify/v"] = np.array([float(cert), theta, lmin, float(mv), float(dist)]), v
    for tag, eta in (("certify_live", ETA), ("certify_live_small", ETA_SMALL)):
        cert, theta, lmin, v, mv, dist, _ = ex.certify_live(eta)
        out[tag + "/scalars"], out[tag + "/v"] = np.array([float(cert), theta, lmin, float(mv), float(dist)]), v
    ex.barrier()
    ex.close()
    s.close()
    return out


def _children(argvs, env, timeout):
    procs = [subprocess.Popen([sys.executable, WORKER] + a, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for a in argvs]
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
            raise RuntimeError("child %d failed (%d):\n%s" % (k, p.returncode, outs[k][-3000:]))


def compute_case(case, lib=None, timeout=240):
    """one of CASES -> {case/name: array}, computed by child processes"""
    kind, which = case.split("/")
    env = dict(os.environ)
    env.pop("DCORA_LANCZOS", None)
    with tempfile.TemporaryDirectory() as d:
        if kind == "single":
            env.update(FORMS[which])
            with open(os.path.join(d, "job.json"), "w") as f:
                json.dump(dict(lib=lib), f)
            _children([["single", d]], env, timeout)
            got = dict(np.load(os.path.join(d, "single.npz")))
        else:
            env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
            env["DCORA_EXCHANGE_TIMEOUT_S"] = "60"
            env.pop("DCORA_EXCHANGE_WAIT", None)
            env.pop("DCORA_EXCHANGE", None)
            with open(os.path.join(d, "job.json"), "w") as f:
                json.dump(dict(lib=lib, workload=which), f)
            job = "m%s" % uuid.uuid4().hex[:12]
            _children([["rank", d, str(k), str(WORLD), job] for k in range(WORLD)], env, timeout)
            r0, r1 = [dict(np.load(os.path.join(d, "rank%d.npz" % k))) for k in range(WORLD)]
            if rec.differing(r0, r1):
                raise RuntimeError("%s: the ranks disagree on %s" % (case, rec.differing(r0, r1)))
            got = r0
    return {case + "/" + k: np.ascontiguousarray(v, dtype=np.float64) for k, v in got.items()}


def compute(lib=None, cases=CASES):
    out = {}
    for case in cases:
        out.update(compute_case(case, lib))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--check", default=None)
    a = ap.parse_args()
    lib = os.path.abspath(a.lib) if a.lib else None
    got = compute(lib)
    for k in sorted(got):
        if not k.endswith("/v"):
            print(k, got[k].tolist())
    if a.out:
        np.savez_compressed(a.out, **got)
        print("wrote", a.out, os.path.getsize(a.out), "bytes,", len(got), "arrays")
    if a.check:
        bad = rec.differing(got, dict(np.load(a.check)))
        print("arrays that differ from %s: %s" % (a.check, bad if bad else "none of %d" % len(got)))
        if bad:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
