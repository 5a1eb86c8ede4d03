"""The inputs and numpy references of the session projection tests (tests/session_project_inputs.py), checked without a
GPU: every point the GPU tests project has the eigenvalue gap and the block conditioning that keep the reference inside
their bounds; the reference agrees with the CPU oracle's projectSolutionRASLAM through the Gram matrix P^T P (1e-10, the
bound of tests/test_block_factors_gpu.py section e; the two branches of the reflect decision differ by more than 1e-3);
the reference's basis reproduces its own point; the new entry points are declared, bound, exported and guarded."""
import numpy as np
import pytest

import session_project_inputs as spi
import session_round_inputs as sri

EPS = spi.EPS
CHUNK = 768  # columns per workgroup of the Gram kernel (dcora_amd/csrc/session_project.h); the GPU test reads it


@pytest.fixture(scope="module")
def orc(built):
    from oracle import orc
    return orc


def _points():
    for d, r, n, nu in spi.size_cases():
        yield d, r, n, nu, spi.lifted_point(d, r, n, spi.seed_of(d, r, n, nu), nu)


def test_every_point_has_the_gap_and_well_conditioned_blocks():
    worst_gap, worst_sig = np.inf, np.inf
    for d, r, n, nu, X in _points():
        gap, sig = spi.eig_gap(X, d), spi.block_sigma_min(X, d, n, 0, True)
        worst_gap, worst_sig = min(worst_gap, gap), min(worst_sig, sig)
        assert gap >= spi.GAP, (d, r, n, nu, gap)
        assert sig >= spi.BLOCK_SIGMA_MIN, (d, r, n, nu, sig)
    for d in spi.DIMS:
        for m in spi.REFLECT_KEEP + spi.REFLECT_FLIP:
            Xd, X = spi.reflect_case(d, m)
            n, l = spi.REFLECT_DIMS["n"], spi.REFLECT_DIMS["l"]
            gap, sig = spi.eig_gap(X, d), spi.block_sigma_min(X, d, n, l, False)
            worst_gap, worst_sig = min(worst_gap, gap), min(worst_sig, sig)
            assert gap >= spi.GAP, (d, m, gap)
            assert sig >= spi.BLOCK_SIGMA_MIN - 8 * EPS, (d, m, sig)  # (the family's least singular value IS 0.5)
    print("least gap %.3f (rule %.2f), least block sigma_min %.3f (rule %.2f)" %
          (worst_gap, spi.GAP, worst_sig, spi.BLOCK_SIGMA_MIN))


def test_chunk_sizes_reach_the_edges_of_the_gram_kernel():
    for d in spi.DIMS:
        ks = [(d + 1) * n for n in spi.chunk_sizes(d, CHUNK)]
        assert min(ks) < 4 or d == 3  # (one pose of SE(3) has four columns)
        assert any(k % 4 for k in ks) or d == 3
        assert any(CHUNK - (d + 1) <= k < CHUNK for k in ks) and CHUNK in ks and any(CHUNK < k <= CHUNK + d + 1 for k in ks)
        assert any(k > 2 * CHUNK and k % CHUNK for k in ks)


@pytest.mark.parametrize("d", spi.DIMS)
def test_reference_agrees_with_the_oracle_on_the_sizes(orc, d):
    worst = 0.0
    for r in spi.ranks_of(d):
        for n in spi.SIZES:
            for nu in spi.NUS:
                X = spi.lifted_point(d, r, n, spi.seed_of(d, r, n, nu), nu)
                ref = spi.project_reference(X, d, n, 0, True)
                Po = orc.project_solution_raslam(X, r, d, n, 0, 0)  # (the oracle reads l = b = 0 as the SE ordering)
                Pr = ref["P"]
                assert ref["npos"] in (0, n) and ref["reflect"] == (ref["npos"] < n // 2)
                if r == d:
                    # no truncation at r == d: the oracle projects X's blocks as they stand (a left-handed Ylift gives
                    # blocks of determinant -1, each flipped on its own), and project() leaves the session alone
                    continue
                if n // 2 == 0:
                    # one pose: npos < n / 2 never reflects, so a truncation that came out left-handed is projected as
                    # it stands and the outcome depends on the handedness the eigensolver happened to return -- the
                    # band tests/test_block_factors_gpu.py leaves out; the GPU tests compare such a point with
                    # Proj(basis^T X) under the returned basis only
                    continue
                err = float(np.abs(Pr.T @ Pr - Po.T @ Po).max())
                worst = max(worst, err)
                assert err <= 1e-10, (d, r, n, nu, err)
    print("reference vs oracle, sizes d=%d: |G - G_oracle|_max %.2e (bound 1e-10)" % (d, worst))


@pytest.mark.parametrize("d", spi.DIMS)
def test_reference_takes_the_expected_reflect_branch(orc, d):
    n, l, b, r = (spi.REFLECT_DIMS[key] for key in ("n", "l", "b", "r"))
    for m in spi.REFLECT_KEEP + spi.REFLECT_FLIP:
        Xd, X = spi.reflect_case(d, m)
        want, kept, flipped = spi.reflect_expected(Xd, d, m)
        ref = spi.project_reference(X, d, n, l, False)
        Po = orc.project_solution_raslam(X, r, d, n, l, b)
        G = ref["P"].T @ ref["P"]
        dist = {False: np.abs(G - kept.T @ kept).max(), True: np.abs(G - flipped.T @ flipped).max()}
        print("reflect d=%d m=%d: reference |G - G_kept| %.2e |G - G_reflected| %.2e; vs oracle %.2e; npos %d" %
              (d, m, dist[False], dist[True], np.abs(G - Po.T @ Po).max(), ref["npos"]))
        assert dist[want] <= 1e-10 and dist[not want] > 1e-3, (m, dist)
        assert np.abs(G - Po.T @ Po).max() <= 1e-10
        assert ref["npos"] in (m, n - m)  # either handedness of the truncation
        assert ref["reflect"] == (ref["npos"] < n // 2)


def test_reference_point_is_the_projection_under_its_own_basis():
    d, r, n = 3, 5, 17
    X = spi.lifted_point(d, r, n, spi.seed_of(d, r, n, 1e-3), 1e-3)
    ref = spi.project_reference(X, d, n, 0, True)
    P = spi.project_blocks(spi.truncate(X, ref["basis"]), d, n, 0, True, False)
    assert np.array_equal(P, ref["P"])
    R = spi.rotation_blocks(P, d, n, 0, True)
    assert (np.linalg.det(R) > 1 - 64 * EPS).all()
    assert np.abs(ref["basis"].T @ ref["basis"] - np.eye(d)).max() <= 8 * EPS
    assert np.allclose(ref["sigma"][:d] ** 2, np.linalg.eigvalsh(X @ X.T)[::-1][:d], rtol=1e-12)
    # the SE -> RA reordering keeps a pose's columns together
    assert np.array_equal(sri.se_from_ra(spi.ra_from_se(X, d, n), d, n, 0), X)


# ---- the interface, without a device ----------------------------------------------------------------------------------------
ENTRIES = ("dcora_rbcd_project", "dcora_ra_rbcd_project", "dcora_debug_project_gram")


def test_entry_points_are_declared_bound_and_exported(built):
    import ctypes as C
    import os
    import re
    from dcora_amd import capi
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "dcora_hip.h")).read()
    L = C.CDLL(capi.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SIGNATURES and capi.SIGNATURES[name][0] is C.c_int, name
        assert hasattr(L, name), name
    # the chunk the CPU checks above size their inputs by is the kernel's
    src = open(os.path.join(os.path.dirname(capi.__file__), "csrc", "session_project.h")).read()
    assert int(re.search(r"constexpr int kGramCols = (\d+);", src).group(1)) == CHUNK


def test_entry_points_refuse_bad_arguments_before_any_device_use(built):
    """a NULL session and a Gram call without a matrix or with a rank outside 1 .. 16 end in the guard and the argument
    check (host only, as tests/test_abi_guard_cpu.py: nothing is handed to a live device)"""
    import ctypes as C
    import dcora_amd as da
    from dcora_amd import capi
    if da.device_count() > 0:
        pytest.skip("a device is present: bad arguments are only handed to the library without one")
    L = C.CDLL(capi.LIB_PATH)
    L.dcora_last_error.restype = C.c_char_p
    for name in ENTRIES[:2]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * 6
        assert fn(None, None, None, None, None, None) == 1 and L.dcora_last_error() == b"null argument", name
    fn = L.dcora_debug_project_gram
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn(5, 10, None, None, None) == 1 and L.dcora_last_error() == b"null argument"
    X, G = np.ones(17 * 4), np.zeros(17 * 17)
    for r, k in ((0, 4), (17, 4), (5, 0)):
        assert fn(r, k, X.ctypes.data_as(C.c_void_p), G.ctypes.data_as(C.c_void_p), None) == 1, (r, k)
        assert b"dcora_debug_project_gram" in L.dcora_last_error()


def test_python_view_and_driver_options(built):
    import inspect
    import dcora_amd as da
    from dcora_amd import driver
    for cls in (da.RbcdSession, da.RaRbcdSession):
        assert callable(getattr(cls, "project", None)), cls
    for fn in (driver.multi_robot_staircase_session, driver.raslam_staircase_session):
        p = inspect.signature(fn).parameters
        assert p["project_on_device"].default is False and p["round_on_device"].default is False, fn
    # the multi-rank drivers have no projection: a job's ranks are refused by the entry
    for fn in (driver.multi_robot_staircase_ranks, driver.raslam_staircase_ranks):
        assert "project_on_device" not in inspect.signature(fn).parameters, fn
