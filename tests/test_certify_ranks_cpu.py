"""The addressing of the job-wide certificate (dcora_exchange_certify_live) on a machine without a GPU, through the
host-only debug entry dcora_debug_cert_rows: the table of one agent's rows of M = (Q - Lambda) + eta I in the CSR order
of the job-wide pattern, a host loop in the kernel's place.  Over all ranks, agents and windows every stored entry of
the pattern is written exactly once, by the rank hosting its row, and the assembled array equals the host assembly --
csr_shift_diag(Q - blockdiag(Lambda), eta) on dcora_cert_dual_matrix's pattern -- bit for bit
(ref src/DCORA_utils.cpp:1898-1982)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import common
from test_raslam import ra_path

ETA = 1e-3


def cert_rows(dims, Q, adims, cols, lam, lo, hi, corrupt=-1, rounds_of=0):
    """-> (status, window values, written counts, nnz of the job-wide pattern); rounds_of > 0: [lo, hi) walked in rounds
    of that many entries, as the job walks the value array through the segment's X area"""
    from dcora_amd import capi
    cols = np.ascontiguousarray(cols, np.int32)
    lam = np.ascontiguousarray(lam, np.float64)
    win, wr, nnz = np.zeros(max(hi - lo, 1)), np.zeros(max(hi - lo, 1), np.uint8), C.c_longlong(-1)
    st = capi.lib().dcora_debug_cert_rows(C.byref(capi.Dims(*dims)), Q.rp, Q.ci, Q.v, C.byref(capi.Dims(*adims)), cols,
                                          lam, ETA, lo, hi, rounds_of, win.ctypes.data_as(C.c_void_p),
                                          wr.ctypes.data_as(C.c_void_p), C.byref(nnz), corrupt)
    return st, win[:hi - lo], wr[:hi - lo], int(nnz.value)


def lambda_coo(d, rot_cols, sphere_cols, lam):
    """(rows, cols, values) of blockdiag(Lambda) from the device's layout of its values: d x d blocks column-major on
    the rotation columns of every pose, then one scalar per unit sphere"""
    I, J, V = [], [], []
    q = 0
    for c in rot_cols:
        for b in range(d):
            for a in range(d):
                I.append(c + a)
                J.append(c + b)
                V.append(lam[q])
                q += 1
    for c in sphere_cols:
        I.append(c)
        J.append(c)
        V.append(lam[q])
        q += 1
    assert q == len(lam)
    return np.array(I), np.array(J), np.array(V)


def host_assembly(Q, LI, LJ, LV):
    """csr_shift_diag(Q - blockdiag(Lambda), eta) on the pattern Q's entries, Lambda's entries and every diagonal give:
    (rowptr, colidx, values), the values in the host assembly's order of operations, (Q - Lambda) + eta"""
    k = Q.n
    A = Q.to_scipy()
    rows = np.repeat(np.arange(k), np.diff(Q.rp))
    allI = np.concatenate([rows, LI, np.arange(k)])
    allJ = np.concatenate([Q.ci, LJ, np.arange(k)])
    P = sp.csr_matrix((np.ones(allI.size), (allI, allJ)), shape=(k, k))
    P.sum_duplicates()
    P.sort_indices()
    prow = np.repeat(np.arange(k), np.diff(P.indptr))
    key = lambda i, j: np.asarray(i, np.int64) * k + np.asarray(j, np.int64)
    pk = key(prow, P.indices)
    assert np.all(np.diff(pk) > 0)
    qv, lv = np.zeros(pk.size), np.zeros(pk.size)
    has_l = np.zeros(pk.size, bool)
    qv[np.searchsorted(pk, key(rows, Q.ci))] = Q.v
    at = np.searchsorted(pk, key(LI, LJ))
    lv[at] = LV
    has_l[at] = True
    vals = np.where(has_l, qv - lv, qv)
    vals = np.where(prow == P.indices, vals + ETA, vals)
    assert A.shape == (k, k)
    return P.indptr, P.indices, vals, Q.nnz


def check_job(dims, Q, agents, world, want_rp, want_vals, windows, memo=None):
    """agents: [(adims, cols, lambda values)] in agent order; consecutive agents share a rank, ceil(R / world) each.
    memo: what the entry returned for (agent, window), shared between the splits of one job -- an agent's call does
    not depend on who else its rank hosts"""
    memo = {} if memo is None else memo
    nnz = want_vals.size
    R = len(agents)
    per = (R + world - 1) // world
    row_rank = np.full(Q.n, -1)
    for a, (_, cols, _) in enumerate(agents):
        row_rank[np.asarray(cols)] = a // per
    assert np.all(row_rank >= 0)
    entry_rank = np.repeat(row_rank, np.diff(want_rp))  # the rank hosting the row of every stored entry
    for w in windows:
        got = np.full(nnz, np.nan)
        count = np.zeros(nnz, int)
        by_rank = np.full(nnz, -1)
        # small windows: the entry walks the rounds itself (one call per agent); larger ones: one call per window
        for lo in (range(0, nnz, w) if w >= 1000 else [0]):
            hi = min(nnz, lo + w) if w >= 1000 else nnz
            for rank in range(world):
                for a in range(rank * per, min(R, (rank + 1) * per)):  # (a rank past the last agent hosts none)
                    adims, cols, lam = agents[a]
                    if (a, lo, hi, w) not in memo:
                        memo[(a, lo, hi, w)] = cert_rows(dims, Q, adims, cols, lam, lo, hi, rounds_of=w if w < 1000 else 0)
                    st, win, wr, n = memo[(a, lo, hi, w)]
                    assert st == 0 and n == nnz
                    hit = np.flatnonzero(wr)
                    got[lo + hit] = win[hit]
                    count[lo + hit] += wr[hit]
                    by_rank[lo + hit] = rank
        assert np.all(count == 1), "window %d: entries written %s times" % (w, np.unique(count))
        assert np.array_equal(by_rank, entry_rank)
        assert np.array_equal(got, want_vals), "window %d: max difference %g" % (w, np.max(np.abs(got - want_vals)))


@pytest.fixture(scope="module")
def grid():
    import dcora_amd as da
    ds = common.product_dataset("smallGrid3D")
    Q = da.build_Q_pgo(ds)
    d, n, R = ds.d, ds.n, 5
    dh, per = d + 1, n // R
    rng = np.random.default_rng(17)
    agents = []
    for b in range(R):
        p0, p1 = b * per, (n if b == R - 1 else (b + 1) * per)
        agents.append(((5, d, p1 - p0, 0, 0, 0), np.arange(p0 * dh, p1 * dh), rng.standard_normal((p1 - p0) * d * d)))
    lam = np.concatenate([a[2] for a in agents])
    LI, LJ, LV = lambda_coo(d, [i * dh for i in range(n)], [], lam)
    return (5, d, n, 0, 0, 0), Q, agents, host_assembly(Q, LI, LJ, LV), {}


@pytest.mark.parametrize("world", [1, 2, 4])
def test_pose_graph_rows_assemble_the_host_matrix(grid, world):
    dims, Q, agents, (rp, ci, vals, _), memo = grid
    nnz = vals.size
    assert 3 * 2500 < nnz < 4 * 2500  # (the X area of this job at r = 5 is 2500 doubles: four rounds)
    if world == 4:
        assert (len(agents) + 3) // 4 * 3 >= len(agents)  # rank 3 hosts no agent
    check_job(dims, Q, agents, world, rp, vals, [1, 7, 2500, 8000, nnz], memo)


def test_pattern_grows_where_Q_lacks_an_entry():
    """an isolated pose (its only closure has weight 0 at creation, so Q holds nothing but its explicit diagonal) lacks
    the off-diagonal entries of its Lambda block: the job-wide pattern has more entries than Q's, and they carry
    -Lambda"""
    import dcora_amd as da
    d, n, dh = 3, 4, 4
    ids = np.array([[0, 0, 0, 1], [0, 1, 0, 2], [0, 0, 0, 3]], np.int32)  # pose 3 hangs on one closure
    vals = np.zeros((3, d * d + d + 3))
    vals[:, [0, 4, 8]] = 1.0
    vals[:, 9:12] = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    vals[:, 12], vals[:, 13], vals[:, 14] = 2.0, 3.0, 1.0
    vals[2, 14] = 0.0  # ... whose weight is zero
    ds = da.Dataset(d, n, ids, vals)
    Q = da.build_Q_pgo(ds)
    rng = np.random.default_rng(3)
    agents = [((3, d, 2, 0, 0, 0), np.arange(0, 2 * dh), rng.standard_normal(2 * d * d)),
              ((3, d, 2, 0, 0, 0), np.arange(2 * dh, 4 * dh), rng.standard_normal(2 * d * d))]
    LI, LJ, LV = lambda_coo(d, [i * dh for i in range(n)], [], np.concatenate([a[2] for a in agents]))
    rp, ci, want, nnzq = host_assembly(Q, LI, LJ, LV)
    assert want.size > nnzq, "Q stores every entry of Lambda: the case shows nothing"
    check_job((3, d, n, 0, 0, 0), Q, agents, 2, rp, want, [1, 5, want.size])


def test_range_aided_rows_are_scattered():
    """range_aided_slam_test_2d, two robots: an agent's rows are scattered over the global ordering [rotations | unit
    spheres | translations | landmarks], and Lambda has a scalar on every unit sphere"""
    import dcora_amd as da
    ra = da.RADataset(ra_path("range_aided_slam_test_2d"))
    assert len(ra.robots) == 2 and ra.l > 0
    d = ra.d
    rng = np.random.default_rng(23)
    agents, LI, LJ, LV = [], [], [], []
    for rb in ra.robots:
        (na, la, ba), own = ra.agent_columns[rb]
        lam = rng.standard_normal(na * d * d + la)
        agents.append(((3, d, na, la, ba, 2), own, lam))
        i, j, v = lambda_coo(d, [own[q * d] for q in range(na)], [], lam[:na * d * d])
        # (a rotation block's columns are consecutive in the global ordering as in the agent's)
        assert all(np.array_equal(own[q * d:(q + 1) * d], own[q * d] + np.arange(d)) for q in range(na))
        LI += [i, own[na * d:na * d + la]]
        LJ += [j, own[na * d:na * d + la]]
        LV += [v, lam[na * d * d:]]
    owned = np.sort(np.concatenate([a[1] for a in agents]))
    assert np.array_equal(owned, np.arange(ra.k)), "a variable without an agent: the case needs another fixture"
    assert np.any(np.diff(agents[0][1]) > 1), "the first agent's rows are contiguous: nothing is scattered"
    rp, ci, want, _ = host_assembly(ra.Q, np.concatenate(LI), np.concatenate(LJ), np.concatenate(LV))
    for world in (1, 2):
        check_job((3, d, ra.n, ra.l, ra.b, 2), ra.Q, agents, world, rp, want, [1, 7, 2500, want.size])


def test_table_with_an_index_out_of_range_is_refused(grid):
    from dcora_amd import capi
    dims, Q, agents, (rp, ci, vals, _), _ = grid
    adims, cols, lam = agents[1]
    for entry in (0, 57):
        st, win, wr, _ = cert_rows(dims, Q, adims, cols, lam, 0, vals.size, corrupt=entry)
        assert st == 1  # DCORA_ERR_BAD_ARG
        assert "source index" in capi.lib().dcora_last_error().decode()
        assert not wr.any(), "a table that failed its check was walked"
    # a window outside the value array is refused as well
    st, _, _, _ = cert_rows(dims, Q, adims, cols, lam, 0, vals.size + 1)
    assert st == 1
