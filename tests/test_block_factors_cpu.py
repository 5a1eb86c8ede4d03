"""tests/golden/block_factors.npz (make_block_factors.py: polar, QF and SO(d) factors of single blocks at 50 digits) is
consistent with itself and with LAPACK where LAPACK is accurate, the CPU oracle -- the algorithmic twin of the device
code -- reproduces it to the accuracy the generator measured, and the generator still writes the same bits."""
import importlib.util
import os

import numpy as np
import pytest

import block_factors as bf

EPS = np.finfo(np.float64).eps


def test_references_are_orthonormal_and_so_references_are_rotations():
    fx = bf.load()
    for g in bf.pq_groups(fx):
        for ref in (g.polar, g.qf):
            assert bf.orth_err(ref).max() <= 4 * EPS, g.name
    for g in bf.so_groups(fx):
        assert bf.orth_err(g.ref).max() <= 4 * EPS, g.name
        assert np.abs(np.linalg.det(g.ref) - 1.0).max() <= 4 * EPS, g.name


def test_well_conditioned_groups_agree_with_lapack():
    """entry by entry to 64 eps for kappa <= 1e2 (LAPACK's own error grows with kappa: 62 eps at kappa = 1e2 here)"""
    fx = bf.load()
    seen = 0
    for g in bf.pq_groups(fx):
        if g.cond > 1e2 * (1 + 1e-6) or g.kind >= len(bf.KAPPAS):
            continue
        seen += 1
        for A, P, Q in zip(g.inp, g.polar, g.qf):
            U, _, Vt = np.linalg.svd(A, full_matrices=False)
            assert np.abs(U @ Vt - P).max() <= 64 * EPS, g.name
            Qn, Rn = np.linalg.qr(A)
            assert np.abs(Qn * np.sign(np.diag(Rn)) - Q).max() <= 64 * EPS, g.name
    assert seen == 2 * len(bf.PQ_DR)
    for g in bf.so_groups(fx):
        if g.r != g.d or g.cond > 1e2:
            continue
        for M, R in zip(g.inp, g.ref):
            U, _, Vt = np.linalg.svd(M)
            D = np.eye(g.d)
            D[-1, -1] = np.sign(np.linalg.det(U @ Vt))
            assert np.abs(U @ D @ Vt - R).max() <= 64 * EPS, g.name


def test_every_case_of_the_fixture_is_present():
    fx = bf.load()
    pq = {(g.d, g.r, g.kind) for g in bf.pq_groups(fx)}
    assert pq == {(d, r, k) for d, r in bf.PQ_DR for k in range(len(bf.KAPPAS) + 3)}
    so = [(g.d, g.r, g.sign, g.tail) for g in bf.so_groups(fx)]
    want = [(d, r, s, t) for d, r in bf.SO_DR for s in (1, -1) for t in range(5)]
    assert sorted(so) == sorted(want + [(2, 2, 0, -1), (3, 3, 0, -1)])
    for g in bf.so_groups(fx):
        if g.sign == 0:  # exact rank d - 1, and the plain completion of the frame has either handedness
            assert all(np.linalg.matrix_rank(M) == g.d - 1 for M in g.inp)
            for M, R in zip(g.inp, g.ref):  # the nearest rotation of a rank d - 1 block: R^T M symmetric, >= 0
                S = R.T @ M
                assert np.array_equal(S, S.T) and np.linalg.eigvalsh(S).min() >= -4 * EPS
            assert len(g.inp) == 24
        else:
            assert all(np.sign(np.linalg.det(M)) == g.sign for M in bf.so_blocks(fx, g))
    assert os.path.getsize(bf.PATH) < 300 * 1024


def test_oracle_reproduces_the_fixture(built):
    """guards the twin itself: per group within 2 x max(what the generator measured, eps cond)"""
    fx = bf.load()
    orth = 0.0
    bad = []
    for d, r in bf.PQ_DR:
        groups = bf.pq_groups(fx, d, r)
        A = np.concatenate([g.inp for g in groups])
        Po, Qo = bf.oracle_polar(A), bf.oracle_qf(A)
        orth = max(orth, bf.orth_err(Po).max(), bf.orth_err(Qo).max())
        for what, out in (("polar", Po), ("qf", Qo)):
            for g, err in bf.pq_group_errors(groups, out, what):
                if not err <= 2 * g.tol(what):
                    bad.append("%s %s: %.3e > 2 x %.3e" % (what, g.name, err, g.tol(what)))
    for d, r in bf.SO_DR:
        groups = bf.so_groups(fx, d, r)
        Ro = bf.oracle_so(np.concatenate([g.inp for g in groups]), bf.so_anchor(fx, d, r))
        orth = max(orth, bf.orth_err(Ro).max())
        for g, err in bf.so_group_errors(groups, Ro):
            if not err <= 2 * g.tol():
                bad.append("so %s: %.3e > 2 x %.3e" % (g.name, err, g.tol()))
    assert not bad, "\n".join(bad)
    assert orth <= 2 * float(fx["oracle_orth"])


def test_generator_reproduces_two_groups_bitwise():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_block_factors",
                                                  os.path.join(os.path.dirname(bf.PATH), "make_block_factors.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = bf.load()
    g = [g for g in bf.pq_groups(fx, 3, 9) if g.kind == 5][0]  # kappa = 1e10, first rank past the 8-wide fit
    A, P, Q, cond = gen.make_pq_group(3, 9, 5)
    assert A.tobytes() == g.inp.tobytes() and P.tobytes() == g.polar.tobytes() and Q.tobytes() == g.qf.tobytes()
    assert cond == g.cond
    g = [g for g in bf.so_groups(fx, 3, 5) if g.sign == -1 and g.tail == 3][0]  # det < 0, sigma_min = 1e-9, under R0
    Y, R, cond = gen.make_so_group(3, 5, -1, 3)
    assert Y.tobytes() == g.inp.tobytes() and R.tobytes() == g.ref.tobytes() and cond == g.cond
    assert gen.so_frame(3).tobytes() == np.ascontiguousarray(fx["so_R0_3"]).tobytes()
