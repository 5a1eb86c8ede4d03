"""One build of the library on the generic (thread-per-variable) solver path, for A/B against another build: a process
loads ONE libdcora_hip.so, so the caller alternates processes.

    python tools/generic_window.py [--lib PATH/libdcora_hip.so] [--replays 5]

The cases are the ones that reach every CSR SpMM kernel of spmm_csr.hip:
  tiers_r3       tiers.pyfg at r = 3 from the odometry start (RA layout, a long landmark row: k_spmm_dir_fix<2>)
  long150_r5     the two hub shapes of tests/test_dense_forms_oracle_gpu.py (long rotation rows: k_spmm_dir +
  long150_r16    k_hessfix), from their warm starts
  sphere2500_r16 sphere2500 at r = 16 (no long row: k_spmm_dir_fix<3>)

Prints one JSON line: per case the milliseconds of every replayed solve and a sha256 digest of f, EucGrad, HessVec and
of the iterate and result of the solve: two builds that compute the same thing print the same digests."""
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
