"""writes tests/golden/exact_factors_ref.npz: recorded numbers (never matrices) of the cases of tests/exact_factors.py

Per case and scale group a: kappa_2(A) (dense eigvalsh; 2 s at k = 4000), the error of LAPACK's cho_solve against the
exact W (relative, Frobenius, 16 columns), the error of LAPACK's log-determinant against ln 2 sum e_i with the
sum of |2 ln l_ii| over its pivots, the oracle's solve error (its scalar up-looking Cholesky, reg = 0), and a SHA-256 of
A's rp / ci / v bytes.  The matrices come out of integer arithmetic, so the hashes are reproduced bit for bit; the
floating-point figures depend on the LAPACK at hand and are recorded, not regenerated, by the tests.

    python tests/golden/make_exact_factors_ref.py        (needs the oracle built: python __graft_entry__.py)"""
import os
import sys

import numpy as np
import scipy.linalg as sl

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import exact_factors as ef  # noqa: E402


def hashes():
    """{(case, a): sha256 of A}: integer arithmetic only"""
    return {(cid, a): ef.case(cid).sha256(a) for cid in ef.CASES for a in ef.SCALES}


def oracle_solve_error(c, a):
    from oracle import orc
    W, V = c.WV(a, 5)
    P = orc.Problem(5, c.d, c.n, orc.CSR(c.k, c.rp, c.ci, c.values(a)), reg=0.0, l=c.l, b=c.b)
    Z = P.precon_solve(np.ascontiguousarray(V.T))
    return float(np.linalg.norm(Z - W.T) / np.linalg.norm(W))


def measure(cid, a):
    c = ef.case(cid)
    A = c.scipy(a).toarray()
    w = np.linalg.eigvalsh(A)
    W, V = c.WV(a, ef.W_COLS)
    cf = sl.cho_factor(A, lower=True)
    X = sl.cho_solve(cf, V)
    logs = 2.0 * np.log(np.diag(cf[0]))
    return dict(kappa=float(w[-1] / w[0]), lapack_solve=float(np.linalg.norm(X - W) / np.linalg.norm(W)),
                lapack_logdet=float(abs(logs.sum() - c.logdet(a))), sum_abs_log=float(np.abs(logs).sum()),
                oracle_solve=oracle_solve_error(c, a), sha256=c.sha256(a))


def main():
    rows = [(cid, a, measure(cid, a)) for cid in ef.CASES for a in ef.SCALES]
    out = {"case": np.array([r[0] for r in rows]), "a": np.array([r[1] for r in rows], np.int64),
           "sha256": np.array([r[2]["sha256"] for r in rows])}
    for key in ("kappa", "lapack_solve", "lapack_logdet", "sum_abs_log", "oracle_solve"):
        out[key] = np.array([r[2][key] for r in rows], np.float64)
    np.savez(ef.REF_PATH, **out)
    for cid, a, m in rows:
        print("%-6s a=%-2d kappa %.3e  LAPACK solve %.2e logdet %.2e (sum |2 ln l_ii| %.1f)  oracle solve %.2e" % (
            cid, a, m["kappa"], m["lapack_solve"], m["lapack_logdet"], m["sum_abs_log"], m["oracle_solve"]))


if __name__ == "__main__":
    main()
