"""The agent form of the lift's image kernel (k_lift_images through dcora_debug_lift_images, ref
src/QuadraticProblem.cpp:148-160): from one agent's block X_a (r x k_a) and the GLOBAL eigenvector v, read through the
agent's column map, Xplus = [X_a; 0] and dir = [0; v_a^T].  The kernel only copies, so numpy is matched bit for bit:
r = 2 .. 8 (odd and even r + 1: the pairwise walk crosses column boundaries), 1, 2, 3 and 257 columns (one pair, an odd
tail, more than one workgroup), a contiguous range that starts at an odd column, a scattered list in the range-aided
ordering, and an agent without landmarks."""
import ctypes as C

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    if dcora_amd.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return dcora_amd


def images(da, Xa, v, cols=None, col0=0):
    from dcora_amd import capi
    r, ka = Xa.shape
    P, D = np.full((r + 1) * ka, np.nan), np.full((r + 1) * ka, np.nan)
    cp = None if cols is None else np.ascontiguousarray(cols, np.int32)
    capi.check(capi.lib().dcora_debug_lift_images(r, ka, capi.F(Xa), v.size, np.ascontiguousarray(v, np.float64),
                                                  None if cp is None else cp.ctypes.data_as(C.c_void_p), int(col0), P, D))
    return capi.unF(P, r + 1, ka), capi.unF(D, r + 1, ka)


def expected(Xa, va):
    r, ka = Xa.shape
    P, D = np.zeros((r + 1, ka)), np.zeros((r + 1, ka))
    P[:r] = Xa
    D[r] = va
    return P, D


def ra_agent_columns(d, n, l, b, poses, spheres, landmarks):
    """an agent's columns in the global RA ordering [d n rotations | l spheres | n translations | b landmarks], listed in
    its own ordering: rotations of its poses, its spheres, translations of its poses, its landmarks"""
    rot = [p * d + c for p in poses for c in range(d)]
    sph = [d * n + s for s in spheres]
    tra = [d * n + l + p for p in poses]
    lmk = [d * n + l + n + q for q in landmarks]
    return np.array(rot + sph + tra + lmk, np.int32)


@pytest.mark.parametrize("r", range(2, 9))
@pytest.mark.parametrize("ka", [1, 2, 3, 257])
def test_contiguous_range_from_an_odd_column(da, r, ka):
    rng = np.random.default_rng(100 * r + ka)
    kg, col0 = ka + 12, 7
    Xa, v = rng.standard_normal((r, ka)), rng.standard_normal(kg)
    P, D = images(da, Xa, v, col0=col0)
    Pe, De = expected(Xa, v[col0:col0 + ka])
    assert np.array_equal(P, Pe) and np.array_equal(D, De)


@pytest.mark.parametrize("r", range(2, 9))
@pytest.mark.parametrize("landmarks", [True, False])
def test_scattered_list_in_range_aided_order(da, r, landmarks):
    """two robots' variables interleaved: the agent owns every other pose, every third sphere and, or not, landmarks"""
    d, n, l, b = 3, 43, 17, 9
    cols = ra_agent_columns(d, n, l, b, poses=range(1, n, 2), spheres=range(0, l, 3),
                            landmarks=range(1, b, 2) if landmarks else [])
    kg = (d + 1) * n + l + b
    assert len(set(cols.tolist())) == cols.size and cols.max() < kg and np.any(np.diff(cols) > 1)  # (with gaps)
    rng = np.random.default_rng(7 * r + int(landmarks))
    Xa, v = rng.standard_normal((r, cols.size)), rng.standard_normal(kg)
    P, D = images(da, Xa, v, cols=cols)
    Pe, De = expected(Xa, v[cols])
    assert np.array_equal(P, Pe) and np.array_equal(D, De)


def test_whole_graph_form_is_the_identity_map(da):
    """col0 = 0 over all k columns: what the single-process lift launches"""
    rng = np.random.default_rng(3)
    Xa, v = rng.standard_normal((5, 500)), rng.standard_normal(500)
    P, D = images(da, Xa, v)
    Pe, De = expected(Xa, v)
    assert np.array_equal(P, Pe) and np.array_equal(D, De)


def test_columns_outside_v_are_refused(da):
    from dcora_amd import capi
    Xa, v = np.zeros((3, 4)), np.zeros(6)
    for kw in (dict(col0=3), dict(cols=[0, 1, 2, 6]), dict(cols=[0, -1, 2, 3])):
        with pytest.raises(capi.DcoraError) as e:
            images(da, Xa, v, **kw)
        assert e.value.status == 1
