"""The dense inverse kernels take their operands in ONE form (a job list, dcora_amd/csrc/dense_tiles.h), every host
schedule of them is written once (enqueue_dense_potrf, enqueue_inverse_jobs), a wide piece is a batch of one job and
the single dense build is the batch of one matrix.  None of this may move a bit: tests/golden/device_chol_parent.npz
was written on an MI355X by tools/record_device_chol.py --lib <a library built from the commit before> --out ...; it
holds what that library computed on the cases below (computed twice there, with both caches cleared in between), and the
tree's library must compute every array the parent repeated BIT FOR BIT.

The cases (tools/record_device_chol.py, compute(); computed once per test session):
  dense/single/k40, k64, k68, k1320   PreCondition of QuadraticProblem(5, 3, nb, Q[:4 nb, :4 nb], reg = 0.1) on
                 sphere2500's leading block, nb = 10, 16, 17, 330: less than one 64-column panel, exactly one, one and
                 four columns, 20 and one of 40 columns
  dense/batch/k68, k1320   the leading 2 nb poses of sphere2500 over two agents (equal k, distinct matrices): the session
                 builds both inverses in one batch; PreCondition through a problem attached to each image, and
                 single_equal: the same matrix built alone gives the batch's bits
  sparse/k1320   the nb = 330 block with DCORA_PRECOND=sparse: narrow pieces only (k_small_inv, k_small_w)
  pieces/lattice chordal_initialization(lattice_se3(10, 10, 10), device = 0): its rotation system has 45 narrow
                 (c <= 64), 15 mid (64 < c < 384) and 1 wide (c >= 384) piece ([factor] pieces: of DCORA_INIT_TIMING;
                 the translation system 26, 5 and 0), every piece inverted on the device with device sources.  The
                 hand-over WITHOUT device sources (the wide pieces' M copied to the host) is not reachable from Python
                 without a new entry point: it is covered by reading only.
  verdict/...    the chain matrices of test_device_tiny_matrices (n = 1, 2, 5, 63, 64, 65, 130, 200) and smallGrid3D
                 shifted by +1 and -0.5

  logdet/...     the log-determinants of the same factorisations

Every case above was repeated bit for bit by the parent in the record's two runs, and all but the following are held to
its bits:
  logdet/*       the log-determinant is an atomicAdd per front in whatever order the workgroups arrive (two equal runs
                 prove nothing about a third: logdet/chain200, three fronts in one launch, differs in the last bit now and
                 then, with the parent's library as with this one): 1e-12 relative, as in test_device_tiny_matrices.
A case the record says the parent did NOT repeat would be compared at the tolerance of the existing test of its path
(1e-10 relative for the dense builds, as in test_dense_inverse_built_on_the_device; 1e-9 for the chordal start point);
there is none."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
RECORD = os.path.join(HERE, "golden", "device_chol_parent.npz")
FALLBACK = {"dense/": 1e-10, "sparse/": 1e-10, "pieces/": 1e-9}  # for a case the parent did not repeat


@pytest.fixture(scope="module")
def computed(built):
    import record_device_chol
    return record_device_chol.compute(dense=not os.environ.get("DCORA_PRECOND"))


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(RECORD))


def _equal_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check_family(computed, recorded, family):
    import record_device_chol
    names = [c for c in record_device_chol.cases(recorded) if c.startswith(family)]
    assert names and names == [c for c in record_device_chol.cases(computed) if c.startswith(family)]
    bitwise = 0
    for c in names:
        keys = sorted(k for k in recorded if k.startswith(c + "/") and not k.endswith("/repeats"))
        assert keys == sorted(k for k in computed if k.startswith(c + "/") and not k.endswith("/repeats"))
        if not c.startswith(record_device_chol.ORDER_FREE):
            assert bool(computed[c + "/repeats"]) or not bool(recorded[c + "/repeats"]), c + " no longer repeats its bits"
        for k in keys:
            got, want = computed[k], recorded[k]
            diff = float(np.max(np.abs(got - want))) if got.shape == want.shape else float("nan")
            print(k, "max |difference|", diff, "parent repeated its bits:", bool(recorded[c + "/repeats"]))
            if c.startswith(record_device_chol.ORDER_FREE):
                assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), k
            elif bool(recorded[c + "/repeats"]):
                assert _equal_bits(got, want), k
                bitwise += 1
            elif not k.endswith("/digest"):
                tol = next(t for p, t in FALLBACK.items() if c.startswith(p))
                assert np.linalg.norm(got - want) <= tol * np.linalg.norm(want), k
    return bitwise, names


def test_single_dense_builds_are_bitwise_the_parents(computed, recorded):
    if os.environ.get("DCORA_PRECOND"):
        pytest.skip("DCORA_PRECOND overrides the choice of preconditioner this test is about")
    bitwise, names = _check_family(computed, recorded, "dense/single/")
    assert len(names) == 4 and bitwise == 4  # the batch's comment claims identical bits: none may fall to a tolerance


def test_batched_dense_builds_are_bitwise_the_parents_and_the_single_builds(computed, recorded):
    if os.environ.get("DCORA_PRECOND"):
        pytest.skip("DCORA_PRECOND overrides the choice of preconditioner this test is about")
    bitwise, names = _check_family(computed, recorded, "dense/batch/")
    assert len(names) == 2 and bitwise == 6
    for c in names:
        assert computed[c + "/single_equal"].tolist() == [1.0, 1.0], c  # each matrix built alone: the batch's bits
        assert not _equal_bits(computed[c + "/Z0"], computed[c + "/Z1"])   # (distinct matrices)


def test_forced_sparse_narrow_pieces_are_bitwise_the_parents(computed, recorded):
    assert _check_family(computed, recorded, "sparse/")[0] == 1


def test_every_piece_class_is_bitwise_the_parents(computed, recorded):
    assert _check_family(computed, recorded, "pieces/")[0] == 3


def test_verdicts_and_log_determinants(computed, recorded):
    bitwise, names = _check_family(computed, recorded, "verdict/")
    assert len(names) == 10 and bitwise == 10  # the ten verdicts, exactly
    assert computed["verdict/smallGrid3D_minus0.5/verdict"] == 0.0 and computed["verdict/smallGrid3D_plus1/verdict"] == 1.0
    for n in (1, 2, 5, 63, 64, 65, 130, 200):
        assert computed["verdict/chain%d/verdict" % n] == 1.0
    assert _check_family(computed, recorded, "logdet/") == (0, [c.replace("verdict/", "logdet/") for c in names])


def test_the_bitwise_cases_are_the_majority(recorded):
    import record_device_chol
    names = record_device_chol.cases(recorded)
    bitwise = [c for c in names if bool(recorded[c + "/repeats"]) and not c.startswith(record_device_chol.ORDER_FREE)]
    assert len(names) == 28 and len(bitwise) == 18
