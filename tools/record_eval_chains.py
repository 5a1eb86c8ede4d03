"""The evaluation and bookkeeping kernels of an RTR solve and of an RBCD round (k_fused_grad, k_rtr_init, k_rtr_decide,
k_eval_finish, k_g_nesterov) on the smallest cases where they can go wrong, recorded as one .npz of results:

    python tools/record_eval_chains.py --lib PATH/libdcora_hip.so --out FILE    record what that build computes
    python tools/record_eval_chains.py [--lib PATH/libdcora_hip.so] --check FILE  recompute and compare bit for bit

tests/golden/eval_chains_parent.npz is the record of the commit BEFORE k_fused_grad requested its loads early, written
with --lib pointing at a library built from that commit's sources (profiles/eval_chains.txt, section 3);
tests/test_eval_chains_gpu.py recomputes the cases (compute() below) with the tree's library and wants every array equal.
A process loads ONE library, so the choice is made before the package is used."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

RESULT_KEYS = ("fInit", "fOpt", "gradNormInit", "gradNormOpt", "outer_iterations", "inner_iterations", "accepted_steps",
               "tCGStatus")


def kernel_constant(name):
    """a `constexpr int NAME = <integer>;` of the kernels' headers, so that the shapes below follow the C++"""
    import re
    for header in ("kernels.h", "pose_group.h"):
        with open(os.path.join(ROOT, "dcora_amd", "csrc", header)) as f:
            m = re.search(r"constexpr int %s = (\d+);" % name, f.read())
        if m:
            return int(m.group(1))
    raise KeyError(name)


def use_library(path):
    import lib_window  # (the one way the tools choose a build)
    lib_window.use_library(path)


def _put(out, name, X, res):
    out[name + "/X"] = np.ascontiguousarray(X, dtype=np.float64)
    out[name + "/result"] = np.array([float(res[k]) for k in RESULT_KEYS])


def _solve(da, P, prm, X0, out, name, want_tcg):
    assert P.solver_info()["tcg"] in want_tcg, (name, P.solver_info())
    opt = da.QuadraticOptimizer(P, prm)
    X = opt.optimize(X0)
    res = opt.getOptResult()
    assert P.solver_info()["tcg"] in want_tcg, (name, P.solver_info())  # (the run form did not give up)
    _put(out, name, X, res)
    return X, res


def group_entries(Q, r, d):
    """entries of Q the workgroups of k_fused_grad stage (fused_pb poses each), and the longest row"""
    rp = np.asarray(Q.rp)
    dh = d + 1
    block, gw = kernel_constant("kBlock"), kernel_constant("GW")
    pb = min(block // gw, block // (r * dh))  # fused_pb (pose_group.h)
    n = (len(rp) - 1) // dh
    per = [int(rp[min(n, p0 + pb) * dh] - rp[p0 * dh]) for p0 in range(0, n, pb)]
    return per, int(np.max(rp[1:] - rp[:-1]))


def chain_solves(da, out):
    """9-pose SE(3) chains (a last workgroup that is not full), with a hub (rows of 36 entries: more than the gather's
    first batch of 24) and without (no row above 12), r = 4 and 5, a random G: default parameters and long tCG runs;
    large initial radii (rejected steps); a solve from a converged iterate (k_rtr_init ends it: everything queued
    behind is gated off) followed by a solve of the SAME problem from a fresh point."""
    from test_run_sums_gpu import _chain_graph
    run = ("one launch per run",)
    n = 9
    for hub in (True, False):
        ds = _chain_graph(n, 4 if hub else -1, seed=11)
        Q = da.build_Q_pgo(ds)
        per, longest = group_entries(Q, 5, ds.d)
        assert (longest > 24) if hub else (longest <= 12), longest
        k = (ds.d + 1) * n
        for r in (4, 5):
            rng = np.random.default_rng(5 + r)
            G = 0.3 * rng.standard_normal((r, k))
            X0 = da.manifold_project(r, ds.d, n, rng.uniform(-1, 1, (r, k)))
            tag = "chain/%s/r%d" % ("hub" if hub else "plain", r)
            P = da.QuadraticProblem(r, ds.d, n, Q, G=G)
            Xs, rs = _solve(da, P, da.ROptParameters(), X0, out, tag + "/default", run)
            _solve(da, P, da.ROptParameters(RTR_tCG_iterations=60, gradnorm_tol=1e-9), X0, out, tag + "/long", run)
            if r == 5:
                for radius in (1e2, 1e4, 1e6):
                    _solve(da, P, da.ROptParameters(RTR_iterations=10, RTR_initial_radius=radius, gradnorm_tol=1e-6), X0,
                           out, tag + "/radius%g" % radius, run)
                if hub:
                    # converged already: gradnorm_tol above the gradient norm the first solve ended with
                    prm = da.ROptParameters(gradnorm_tol=4.0 * rs["gradNormOpt"] + 1e-300)
                    _solve(da, P, prm, Xs, out, tag + "/converged", run)
                    X1 = da.manifold_project(r, ds.d, n, rng.uniform(-1, 1, (r, k)))
                    _solve(da, P, da.ROptParameters(), X1, out, tag + "/after_converged", run)
            P.close()


def two_pass_solve(da, out):
    """a chain of 100 poses whose pose 5 sees every other one, r = 5: the first k_fused_grad workgroup stages more than
    kHessTile entries (a second tile pass) and no row is a long row, so the evaluation stays on the fused path (its tCG
    form is not the one-launch run: the hub's rows are too many for it)"""
    from test_run_sums_gpu import _chain_graph
    n, r = 100, 5
    ds = _chain_graph(n, 5, seed=13)
    Q = da.build_Q_pgo(ds)
    per, longest = group_entries(Q, r, ds.d)
    assert per[0] > kernel_constant("kHessTile") and longest <= kernel_constant("kLongRow"), (per[0], longest)
    rng = np.random.default_rng(17)
    k = (ds.d + 1) * n
    G = 0.3 * rng.standard_normal((r, k))
    X0 = da.manifold_project(r, ds.d, n, rng.uniform(-1, 1, (r, k)))
    P = da.QuadraticProblem(r, ds.d, n, Q, G=G)
    _solve(da, P, da.ROptParameters(), X0, out, "two_pass/r5/default", ("two launches", "one launch per run"))
    P.close()


def _session(da, ds, R, r, chain, **kw):
    if chain is not None:
        os.environ["DCORA_CHAIN"] = chain
    try:
        return da.RbcdSession(ds, num_robots=R, r=r, **kw)
    finally:
        os.environ.pop("DCORA_CHAIN", None)


def session_trace(da, out, tag, name, R, r, iters, chain, **kw):
    """per iteration 2 f, |grad|, the block norms, the next agent, the launches the round enqueued and the RTR
    iterations of its (last) local solve; at the end X"""
    import common
    ds = common.product_dataset(name)
    X0 = common.random_point(r, ds.d, ds.n, 3, da.manifold_project)
    s = _session(da, ds, R, r, chain, **kw)
    s.set_X(X0)
    rows, bns, sel = [], [], 0
    for _ in range(iters):
        n0 = s.debug_launches()
        c2, gn, bn, nxt = s.iterate(sel)
        rows.append([c2, gn, float(nxt), float(s.debug_launches() - n0), float(s.last_result()["outer_iterations"])])
        bns.append(np.asarray(bn, dtype=np.float64).copy())
        sel = nxt
    out[tag + "/scalars"] = np.array(rows)
    out[tag + "/block_norms"] = np.array(bns)
    out[tag + "/X"] = np.ascontiguousarray(s.get_X(), dtype=np.float64)
    s.close()


def sessions(da, out):
    for chain in (None, "launches"):
        c = chain or "ride"
        for r in (5, 4):  # smallGrid3D over 2 agents: 62 and 63 poses; plain rounds, restart rounds, the round after
            session_trace(da, out, "session/smallGrid3D/r%d/%s" % (r, c), "smallGrid3D", 2, r, 12, chain,
                          restart_interval=4)
        # planar: the smallest d = 2 graph of tests/golden/data over 2 agents (3 poses each)
        session_trace(da, out, "session/planar/r3/%s" % c, "pose_graph_optimization_test_2d", 2, 3, 6, chain)


def compute():
    import dcora_amd as da
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: these cases run on the device")
    out = {}
    chain_solves(da, out)
    two_pass_solve(da, out)
    sessions(da, out)
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
    if a.lib:
        use_library(a.lib)
    got = compute()
    for k in sorted(got):
        if k.endswith("/result"):
            print(k, dict(zip(RESULT_KEYS, got[k].tolist())))
        elif k.endswith("/scalars"):
            print(k, "launches", got[k][:, 3].astype(int).tolist(), "outer", got[k][:, 4].astype(int).tolist())
    if a.out:
        np.savez_compressed(a.out, **got)
        print("wrote", a.out, os.path.getsize(a.out), "bytes")
    if a.check:
        bad = differing(got, dict(np.load(a.check)))
        print("arrays that differ from %s: %s" % (a.check, bad if bad else "none of %d" % len(got)))
        if bad:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
