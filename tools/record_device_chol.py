"""What the device Cholesky and the dense inverse kernels (dcora_amd/csrc/device_chol.hip, dense_inverse.hip) compute on
the smallest cases at which each of their forms can go wrong, recorded as one .npz of results:

    python tools/record_device_chol.py --lib PATH/libdcora_hip.so --out FILE    record what that build computes
    python tools/record_device_chol.py [--lib PATH/libdcora_hip.so] --check FILE  recompute and compare

tests/golden/device_chol_parent.npz is the record of the commit BEFORE the inverse kernels took one job-list form, written
with --lib pointing at a library built from that commit's sources; tests/test_device_chol_forms_gpu.py recomputes the
cases (compute() below) with the tree's library.  Every case runs twice in one process, with both caches cleared in
between; NAME/repeats says whether the two runs gave the same bits -- only then can another build be held to them.
A process loads ONE library, so the choice is made before the package is used."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

DENSE_NB = (10, 16, 17, 330)   # k = 40 (less than one panel), 64 (exactly one), 68 (one and four columns), 1320 (20 and 40)
BATCH_NB = (17, 330)           # per agent, two agents
CHAIN_N = (1, 2, 5, 63, 64, 65, 130, 200)
ORDER_FREE = ("logdet/",)      # sums by atomicAdd in the order the workgroups arrive: never held to bits, 1e-12 relative
LATTICE = (10, 10, 10)         # the smallest of synth.lattice_se3 with a piece in every class (see the test's docstring)


def use_library(path):
    import lib_window  # (the one way the tools choose a build)
    lib_window.use_library(path)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest(), dtype=np.uint8)


def _twice(da, out, name, run):
    """run() -> dict of arrays; both caches are cleared before each of the two runs"""
    got = []
    for _ in range(2):
        da.precond_cache_clear()
        da.chol_cache_clear()
        got.append(run())
    for key, a in got[0].items():
        out["%s/%s" % (name, key)] = np.asarray(a)
    out[name + "/repeats"] = np.array(all(np.array_equal(_bits(got[0][k]), _bits(got[1][k])) for k in got[0]))


def _sphere_block(da, nb):
    import common
    ds = common.product_dataset("sphere2500")
    Q = da.build_Q_pgo(ds).to_scipy()
    return da.Csr.from_scipy(Q[:4 * nb, :4 * nb].tocsr())


def _point(da, nb, seed=3):
    rng = np.random.default_rng(seed)
    X = da.manifold_project(5, 3, nb, rng.uniform(-1, 1, (5, 4 * nb)))
    return X, rng.standard_normal((5, 4 * nb))


def _precondition(da, nb, Q, kind):
    P = da.QuadraticProblem(5, 3, nb, Q, reg=0.1)
    assert P.precond_info()["kind"] == kind, P.precond_info()
    Z = P.PreCondition(*_point(da, nb))
    P.close()
    return Z


def dense_single(da, out):
    """device_dense_spd_inverse behind PreCondition on sphere2500's leading block"""
    for nb in DENSE_NB:
        Q = _sphere_block(da, nb)
        _twice(da, out, "dense/single/k%d" % (4 * nb), lambda: {"Z": _precondition(da, nb, Q, "dense")})


def dense_batch(da, out):
    """the leading 2 nb poses of sphere2500 over two agents: equal k, distinct matrices, so the session builds both
    inverses in one batch (precond_prebuild_dense); a problem on an agent's matrix then attaches to the batch's image.
    single_equal: the same matrix built alone (caches cleared) gives the batch's bits."""
    import bench
    import common
    full = common.product_dataset("sphere2500")
    for nb in BATCH_NB:
        n = 2 * nb
        keep = (full.ids[:, 1] < n) & (full.ids[:, 3] < n)
        ds = da.Dataset(full.d, n, full.ids[keep], full.vals[keep])
        Qs = []
        for b in range(2):
            nbb, ids, vals = bench.agent_block(ds, 2, b)
            assert nbb == nb
            Qs.append(da.build_Q_pgo(ds, n=nb, agent=b, ids=ids, vals=vals))
        assert not np.array_equal(Qs[0].v, Qs[1].v)

        def run():
            s = da.RbcdSession(ds, num_robots=2, r=5)
            c0 = da.precond_cache_info()
            assert c0["entries"] == 2, c0
            Zb = [_precondition(da, nb, Q, "dense") for Q in Qs]
            c1 = da.precond_cache_info()
            assert c1["hits"] == c0["hits"] + 2 and c1["misses"] == c0["misses"], (c0, c1)  # the batch's images
            s.close()
            same = []
            for b in range(2):
                da.precond_cache_clear()
                same.append(np.array_equal(_bits(_precondition(da, nb, Qs[b], "dense")), _bits(Zb[b])))
            return {"Z0": Zb[0], "Z1": Zb[1], "single_equal": np.array(same, dtype=np.float64)}
        _twice(da, out, "dense/batch/k%d" % (4 * nb), run)


def forced_sparse(da, out):
    """the nb = 330 block with the partitioned sparse inverse forced: narrow pieces only (k_small_inv, k_small_w)"""
    nb = DENSE_NB[-1]
    Q = _sphere_block(da, nb)

    def run():
        old = os.environ.get("DCORA_PRECOND")
        os.environ["DCORA_PRECOND"] = "sparse"
        try:
            return {"Z": _precondition(da, nb, Q, "sparse")}
        finally:
            if old is None:
                del os.environ["DCORA_PRECOND"]
            else:
                os.environ["DCORA_PRECOND"] = old
    _twice(da, out, "sparse/k%d" % (4 * nb), run)


def lattice_dataset(dims=LATTICE):
    from dcora_amd import synth
    return synth.lattice_se3(*dims)


def piece_classes(da, out, dims=LATTICE):
    """chordal initialisation with its two SPD systems solved on the device (device sources: every piece is inverted
    there and its M stays there).  T is 12 n doubles: its digest, and every 16th pose for a comparison by norm"""
    ds = lattice_dataset(dims)

    def run():
        T = da.chordal_initialization(ds, device=0)
        return {"digest": _digest(T).astype(np.float64), "sample": T[:, ::64].copy(), "norm": np.array(np.linalg.norm(T))}
    _twice(da, out, "pieces/lattice", run)


def _chain(n, diag=4.0):
    import scipy.sparse as sp
    A = sp.diags([np.full(n, diag)], [0]).tolil()
    for i in range(n - 1):
        A[i, i + 1] = A[i + 1, i] = -1.0
    return A.tocsr()


def verdicts(da, out):
    """verdict and log-determinant (a case of its own: ORDER_FREE) of the chain matrices of tests/test_device_chol.py
    and of smallGrid3D shifted"""
    import common
    import scipy.sparse as sp
    cases = [("chain%d" % n, _chain(n), 1) for n in CHAIN_N]
    ds = common.product_dataset("smallGrid3D")
    Q = da.build_Q_pgo(ds).to_scipy()
    for tag, sh in (("plus1", 1.0), ("minus0.5", -0.5)):
        cases.append(("smallGrid3D_" + tag, (Q + sh * sp.identity(Q.shape[0])).tocsr(), ds.d + 1))
    for tag, A, block in cases:
        S = da.Csr.from_scipy(A)
        logdets = []

        def run():
            pd, info = da.is_psd_device(S, block, info=True)
            logdets.append(info["logdet"] if pd else 0.0)
            return {"verdict": np.array(float(pd))}
        _twice(da, out, "verdict/" + tag, run)
        out["logdet/%s/value" % tag] = np.array(logdets[0])
        out["logdet/%s/repeats" % tag] = np.array(logdets[0] == logdets[1])


def compute(dense=True, dims=LATTICE):
    """dense = False leaves out the cases that need the library's own choice of preconditioner (DCORA_PRECOND set)"""
    import dcora_amd as da
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: these cases run on the device")
    out = {}
    if dense:
        dense_single(da, out)
        dense_batch(da, out)
    forced_sparse(da, out)
    piece_classes(da, out, dims)
    verdicts(da, out)
    return out


def cases(rec):
    return sorted(k[:-len("/repeats")] for k in rec if k.endswith("/repeats"))


def differing(got, want):
    """arrays of the cases the record repeated bit for bit that are not equal bit for bit (or are missing); the
    ORDER_FREE ones that are further than 1e-12 relative"""
    bad = []
    for c in cases(want):
        for k in sorted(k for k in want if k.startswith(c + "/") and not k.endswith("/repeats")):
            if k not in got or got[k].shape != want[k].shape:
                bad.append(k)
            elif c.startswith(ORDER_FREE):
                if not np.all(np.abs(got[k] - want[k]) <= 1e-12 * np.maximum(1.0, np.abs(want[k]))):
                    bad.append(k)
            elif bool(want[c + "/repeats"]) and not np.array_equal(_bits(got[k]), _bits(want[k])):
                bad.append(k)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--check", default=None)
    ap.add_argument("--lattice", default=None, help="nx,ny,nz of the piece-class case (default: the recorded one)")
    a = ap.parse_args()
    if os.environ.get("DCORA_PRECOND"):
        raise SystemExit("DCORA_PRECOND overrides the choice of preconditioner the dense cases are about")
    if a.lib:
        use_library(a.lib)
    dims = tuple(int(x) for x in a.lattice.split(",")) if a.lattice else LATTICE
    got = compute(dims=dims)
    for c in cases(got):
        print(c, "repeats its bits" if bool(got[c + "/repeats"]) else "DOES NOT repeat its bits",
              {k.rsplit("/", 1)[1]: got[k].tolist() for k in got if k.startswith(c + "/") and got[k].size <= 2
               and not k.endswith("/repeats")})
    if a.out:
        np.savez_compressed(a.out, **got)
        print("wrote", a.out, os.path.getsize(a.out), "bytes")
    if a.check:
        bad = differing(got, dict(np.load(a.check)))
        print("arrays that differ from %s: %s" % (a.check, bad if bad else "none"))
        if bad:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
