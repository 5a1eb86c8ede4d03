"""tests/golden/block_factors_near.npz against its own description (tests/golden/make_block_factors.py): the family of
near-orthonormal blocks that carries the 8-lanes-per-pose kernels through tests/test_group_factors_gpu.py.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import block_factors as bf

EPS = bf.EPS


def _gram_dist(A):
    G = np.einsum("bia,bic->bac", A, A)
    return bf.block_err(G, np.eye(A.shape[2])[None])


def test_groups_are_the_described_ones():
    fx = bf.load_near()
    got = [(g.d, g.r, g.delta, len(g.inp)) for g in bf.near_groups(fx)]
    assert got == [(d, r, delta, 4) for d, r in bf.NEAR_DR for delta in bf.NEAR_DELTAS]
    assert bf.NEAR_DR == [(2, 2), (2, 4), (2, 5), (2, 8), (3, 3), (3, 4), (3, 5), (3, 6), (3, 8)]
    assert bf.NEAR_DELTAS == [1e-6, 1e-3, 0.03, 0.1, 0.2, 0.245, 0.255, 0.4]


def test_entries_are_multiples_of_the_quantum():
    for g in bf.near_groups(bf.load_near()):
        q = g.inp / bf.NEAR_QUANTUM
        assert np.array_equal(q, np.round(q)) and np.abs(q).max() < 2.0 ** 41, g.name


def test_distance_from_orthonormal_is_delta_and_clear_of_the_radius():
    for g in bf.near_groups(bf.load_near()):
        dist = _gram_dist(g.inp)
        assert (np.abs(dist - g.delta) <= 1e-3 * g.delta).all(), (g.name, dist)
        assert (np.abs(dist - bf.GRAM_RADIUS) > 1e-3).all(), (g.name, dist)
        x = np.linalg.eigvalsh(np.einsum("bia,bic->bac", g.inp, g.inp)) - 1.0
        assert ((x.min(axis=1) < 0) & (x.max(axis=1) > 0)).all(), g.name  # mixed signs


def test_references_are_orthonormal():
    for g in bf.near_groups(bf.load_near()):
        for what in ("polar", "qf"):
            assert bf.orth_err(g.ref(what)).max() <= 4 * EPS, (g.name, what)


def test_combinations_reproduce_the_blocks_bit_for_bit():
    """what the GPU tests hand the kernels: X + V, X + V / 2, x / 2 + v / 2 and v + (Xloc - y) / 2"""
    for g in bf.near_groups(bf.load_near()):
        A, E = g.inp, bf.qf_point(len(g.inp), g.r, g.d)
        assert np.array_equal(E + (A - E), A), g.name
        assert np.array_equal(E + 0.5 * (2 * A - 2 * E), A), g.name
        assert np.array_equal(0.5 * E + 0.5 * (2 * A - E), A), g.name
        assert np.array_equal(E + 0.5 * ((2 * A - E) - E), A), g.name
        # every intermediate is a multiple of 2^-41 below 8: exact whatever the order or the contraction
        for M in (A - E, 2 * A - 2 * E, 2 * A - E, 0.5 * (2 * A - E)):
            q = M / (bf.NEAR_QUANTUM / 2)
            assert np.array_equal(q, np.round(q)) and np.abs(q).max() < 2.0 ** 44, g.name


def test_oracle_error_columns_reproduce(built):
    fx = bf.load_near()
    orth = 0.0
    for g in bf.near_groups(fx):
        for what, fn in (("polar", bf.oracle_polar), ("qf", bf.oracle_qf)):
            out = fn(g.inp)
            orth = max(orth, bf.orth_err(out).max())
            err = bf.block_err(out, g.ref(what)).max()
            assert g.oracle_err[what] / 2 <= err <= 2 * g.oracle_err[what], (g.name, what, err, g.oracle_err[what])
    assert float(fx["oracle_orth"]) / 2 <= orth <= 2 * float(fx["oracle_orth"])


def test_generator_still_writes_the_same_bits():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_block_factors",
                                                  os.path.join(os.path.dirname(bf.NEAR_PATH), "make_block_factors.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = bf.load_near()
    g = [g for g in bf.near_groups(fx, 3, 5) if g.delta == 0.245][0]
    A, P, Q, cond = gen.make_near_group(3, 5, bf.NEAR_DELTAS.index(0.245))
    assert A.tobytes() == g.inp.tobytes() and P.tobytes() == g.polar.tobytes() and Q.tobytes() == g.qf.tobytes()
    assert cond == g.cond
    (g,) = bf.nd_groups(fx, 2, 4, 2)
    a, b, c, ref, smin, dist, _, cond = gen.make_nd_group(2, 4, 2)
    for got, want in ((a, g.a), (b, g.b), (c, g.c), (ref, g.ref), (smin, g.smin), (dist, g.dist)):
        assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    assert cond == g.cond


@pytest.mark.parametrize("mode", [1, 2])
def test_non_dyadic_groups(built, mode):
    """the stored factor is orthonormal, is the factor of the float64 combination up to that combination's rounding,
    and the groups straddle the Gram radius; the oracle column reproduces on the rounded combination"""
    fx = bf.load_near()
    for d, r in bf.ND_DR:
        (g,) = bf.nd_groups(fx, d, r, mode)
        assert len(g.ref) == 15 and bf.orth_err(g.ref).max() <= 4 * EPS
        if mode == 1:
            M = (1.0 - bf.ND_ALPHA) * g.a + bf.ND_ALPHA * g.b
        else:
            M = g.a + bf.ND_GAMMA * (g.b - g.c)
        assert (np.abs(_gram_dist(M) - g.dist) <= 1e-12 * (1 + g.dist)).all()
        assert (g.dist < 0.2).any() and (g.dist > 0.3).any() and (np.abs(g.dist - bf.GRAM_RADIUS) > 1e-3).all(), g.dist
        s = np.linalg.svd(M, compute_uv=False)
        assert np.allclose(s[:, -1], g.smin, rtol=1e-12) and abs((s[:, 0] / s[:, -1]).max() - g.cond) <= 1e-12 * g.cond
        err = bf.block_err(bf.oracle_polar(M), g.ref)
        assert (err <= 2 * g.oracle_err + g.forward()).all(), (g.name, err)
