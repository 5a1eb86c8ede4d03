"""One build of the library on the generic (thread-per-variable) solver path, for A/B against another build: a process
loads ONE libdcora_hip.so, so the caller alternates processes.

    python tools/generic_window.py [--lib PATH/libdcora_hip.so] [--replays 5]

The cases are the ones that reach every CSR SpMM kernel of spmm_csr.hip:
  tiers_r3       tiers.pyfg at r = 3 from the odometry start (RA layout, a long landmark row: k_spmm_dir_fix<2>)
  long150_r5     the two hub shapes of tests/test_dense_forms_oracle_gpu.py (long rotation rows: k_spmm_dir +
  long150_r16    k_hessfix), from their warm starts
  sphere2500_r16 sphere2500 at r = 16 (no long row: k_spmm_dir_fix<3>)

Prints one JSON line: per case the milliseconds of every replayed solve and a sha256 digest of f, EucGrad, HessVec and
of the iterate and result of the solve: two builds that compute the same thing print the same digests.

Untimed, under "manifold": digests of what the thread-per-variable manifold kernels (manifold.hip) compute where the
cases above do not reach them:
  d<d>_l<l>_b<b>_r<r>  the layouts of test_range_aided_layout_in_its_four_presence_cases at r = d, d + 3 and 9 (all three
                       register widths): every operator, the dual certificate, the iterate and result of a solve
  rbcd_generic_r5      smallGrid3D, 5 agents, accelerated, 70 iterations under DCORA_SOLVER=generic (k_nesterov in its
  rbcd_r9              four modes, two restarts), and 20 iterations at r = 9 (generic by rank, the widest block)
  ra3d_r4, tiers_r3    RaRbcdSession on range_aided_slam_test_3d (14 iterations, restart interval 5) and on tiers
                       (6 iterations, interval 4): k_polar with three operands, k_tangent with the hub fold"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

KEYS = ("fInit", "gradNormInit", "fOpt", "gradNormOpt", "tCGStatus", "outer_iterations", "inner_iterations",
        "accepted_steps")


def measure(da, P, X, V, kw, replays):
    h = hashlib.sha256(np.float64(P.f(X)).tobytes())
    for a in (P.EucGrad(X), P.HessVec(X, V)):
        h.update(np.ascontiguousarray(a).tobytes())
    ms = []
    for i in range(replays + 1):   # (the first solve is the warm-up)
        opt = da.QuadraticOptimizer(P, da.ROptParameters(**kw))
        t0 = time.perf_counter()
        Xs = opt.optimize(X)
        ms.append(1e3 * (time.perf_counter() - t0))
        res = opt.getOptResult()
        if i == 0:
            h.update(np.ascontiguousarray(Xs).tobytes())
            h.update(np.array([res[k] for k in KEYS], dtype=np.float64).tobytes())
            inner = res["inner_iterations"]
    return {"ms_per_solve": [round(t, 3) for t in ms[1:]], "tcg_iterations": inner, "digest": h.hexdigest()[:16]}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def manifold_digests(da, datasets):
    import scipy.sparse as sp
    import common
    out = {}
    n = 12
    for d in (2, 3):
        for l, b in ((0, 0), (7, 0), (0, 5), (7, 5)):
            k = d * n + l + n + b
            rng = np.random.default_rng(100 * d + 10 * l + b)
            A = sp.random(3 * k, k, density=4.0 / k, random_state=np.random.RandomState(d + l + b), format="csr")
            Q = sp.csr_matrix(A.T @ A + 1e-3 * sp.identity(k))
            Q.sort_indices()
            for r in (d, d + 3, 9):
                X = da.manifold_project(r, d, n, rng.standard_normal((r, k)), l=l, b=b)
                V = rng.standard_normal((r, k))
                P = da.QuadraticProblem(r, d, n, da.Csr.from_scipy(Q), reg=0.05, l=l, b=b)
                Vt = P.projectToTangentSpace(X, V)
                S = da.dual_certificate(r, d, n, X, da.Csr.from_scipy(Q), l=l, b=b).to_scipy()
                S.sort_indices()
                opt = da.QuadraticOptimizer(P)
                Xs = opt.optimize(X)
                res = opt.getOptResult()
                out["d%d_l%d_b%d_r%d" % (d, l, b, r)] = sha(
                    X, P.RieGrad(X), Vt, P.HessVec(X, Vt), P.Retract(X, 0.2 * Vt), P.PreCondition(X, Vt),
                    da.manifold_project(r, d, n, X + 0.3 * V, l=l, b=b), S.indptr, S.indices, S.data, Xs,
                    np.array([res[key] for key in KEYS], dtype=np.float64))
                P.close()

    ds = common.product_dataset("smallGrid3D")
    for tag, r, iters, solver in (("rbcd_generic_r5", 5, 70, "generic"), ("rbcd_r9", 9, 20, None)):
        X0 = common.random_point(r, ds.d, ds.n, 1, da.manifold_project)
        before = os.environ.get("DCORA_SOLVER")
        if solver:
            os.environ["DCORA_SOLVER"] = solver   # (the session reads it at every call)
        try:
            s = da.RbcdSession(ds, num_robots=5, r=r)
            s.set_X(X0)
            res = s.run(max_iters=iters, rgrad_tol=1e-12)
            out[tag] = sha(res["selected"], res["cost"], res["gradnorm"], s.get_X())
            s.close()
        finally:
            if before is None:
                os.environ.pop("DCORA_SOLVER", None)
            else:
                os.environ["DCORA_SOLVER"] = before

    for tag, name, r, iters, interval in (("ra3d_r4", "range_aided_slam_test_3d", 4, 14, 5), ("tiers_r3", "tiers", 3, 6, 4)):
        ra = da.RADataset(os.path.join(datasets.DATA, name + ".pyfg.gz"))
        if name == "tiers":
            X0 = np.vstack([ra.X_odom, np.zeros((r - ra.d, ra.k))])
        else:
            rng = np.random.default_rng(5)
            lift = np.linalg.qr(rng.standard_normal((r, ra.d)))[0]
            X0 = da.manifold_project(r, ra.d, ra.n, lift @ ra.gt + 0.05 * rng.standard_normal((r, ra.k)), l=ra.l, b=ra.b)
        s = da.RaRbcdSession(ra, r, acceleration=True, restart_interval=interval)
        s.set_X(X0)
        res = s.run(max_iters=iters, rgrad_tol=0.0)
        out[tag] = sha(res["selected"], res["cost"], res["gradnorm"], s.get_X())
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--replays", type=int, default=5)
    a = ap.parse_args()
    from dcora_amd import capi
    if a.lib:
        import ctypes
        capi.LIB_PATH = os.path.abspath(a.lib)
        L = ctypes.CDLL(capi.LIB_PATH)
        for name in [n for n in capi.SIGNATURES if not hasattr(L, n)]:  # (an older build lacks the newer entries)
            del capi.SIGNATURES[name]
    import common
    import dcora_amd as da
    import test_dense_forms_oracle_gpu as forms
    from dcora_amd import cora_flow, datasets
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: this tool measures the device")
    out = {"lib": capi.LIB_PATH}
    out["manifold"] = manifold_digests(da, datasets)

    ra = da.RADataset(os.path.join(datasets.DATA, "tiers.pyfg.gz"))
    P = cora_flow.ProductBackend(ra).problem(3)
    X = np.vstack([ra.X_odom, np.zeros((3 - ra.d, ra.k))])
    V = np.random.default_rng(5).standard_normal(X.shape)
    out["tiers_r3"] = measure(da, P, X, V, dict(cora_flow.PARAMS, RTR_iterations=20), a.replays)
    P.close()

    for sid, m, r, solver in forms.LONG_ROWS:
        n, Q, _, G, _, V, Xw = forms.case(("long", 300, 150, m), r)
        P = forms.make_problem(da, r, n, Q, G, None, solver)
        out[sid] = measure(da, P, Xw, V, dict(RTR_iterations=6, RTR_tCG_iterations=50), a.replays)
        P.close()

    ds = common.product_dataset("sphere2500")
    P = da.QuadraticProblem(16, ds.d, ds.n, da.build_Q_pgo(ds))
    X = common.random_point(16, ds.d, ds.n, 3, da.manifold_project)
    V = np.random.default_rng(5).standard_normal(X.shape)
    out["sphere2500_r16"] = measure(da, P, X, V, dict(RTR_iterations=10, RTR_tCG_iterations=50), a.replays)
    P.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
