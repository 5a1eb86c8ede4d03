"""The coloured run loop (dcora_rbcd_run_coloured / dcora_ra_rbcd_run_coloured / dcora_exchange_run_coloured: sweeps of
one tick per colour, each followed by an evaluation -- the agents that fire together of src/Agent.cpp:650-678 as a
schedule) against the loop a caller writes with iterate_set / tick and evaluate: the same calls, hence the same bits;
across ranks against the single-process session with the assertions of tests/test_exchange_gpu.py; and up in the drivers
(dcora_amd/driver.py mode="coloured", the C++ examples' --coloured), which must end where the RBCD++ drivers end:
certified."""
import gzip
import json
import os
import shutil
import subprocess
import sys
import uuid

import numpy as np
import pytest

import common
from ra_ring import write_ring_variant
from test_raslam import ra_path

pytestmark = pytest.mark.gpu

WORKER = os.path.join(common.HERE, "ra_tick_worker.py")
EXAMPLES = os.path.join(os.path.dirname(common.HERE), "dcora_amd", "examples", "_build")


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


def _case(da, tmp_path, case):
    """-> (make a fresh non-accelerated session, start point, worker arguments kind / dataset / R / r)"""
    if case == "ring":
        path = write_ring_variant(tmp_path)[0]
        ra = da.RADataset(path)
        r = 3
        X0 = np.zeros((r, ra.k))
        X0[:ra.d] = ra.X_odom
        return (lambda **kw: da.RaRbcdSession(ra, r, acceleration=False, **kw)), X0, ("ra", path, 4, r)
    name, R = case
    ds = common.product_dataset(name)
    r = 5
    X0 = common.random_point(r, ds.d, ds.n, 11, lambda r_, d_, n_, M: da.manifold_project(r_, d_, n_, M))
    return (lambda **kw: da.RbcdSession(ds, num_robots=R, r=r, acceleration=False, **kw)), X0, ("pgo", name, R, r)


def _hand_loop(s, sweeps):
    col, nc = s.colours()
    cost, gn = [], []
    for _ in range(sweeps):
        for c in range(nc):
            s.iterate_set(np.flatnonzero(col == c).astype(np.int32))
        c2, g, bn, nxt = s.evaluate()
        cost.append(c2)
        gn.append(g)
    return np.asarray(cost), np.asarray(gn)


@pytest.mark.parametrize("case", [("sphere2500", 5), ("torus3D", 8), "ring"], ids=["sphere2500", "torus3D", "ring"])
def test_run_coloured_equals_the_hand_written_loop(env, tmp_path, case):
    da, orc = env
    make, X0, _ = _case(da, tmp_path, case)
    lib, hand = make(), make()
    lib.set_X(X0)
    hand.set_X(X0)
    out = lib.run_coloured(max_sweeps=4, rgrad_tol=0.0)
    cost, gn = _hand_loop(hand, 4)
    assert out["iters"] == 4
    assert np.array_equal(out["cost"], cost) and np.array_equal(out["gradnorm"], gn), (out, cost, gn)
    assert np.array_equal(lib.get_X(), hand.get_X())
    # a tolerance above the second sweep's |rgrad| (and not above the first's): exactly two sweeps
    assert gn[1] < gn[0], gn
    lib.set_X(X0)
    two = lib.run_coloured(max_sweeps=4, rgrad_tol=0.5 * (gn[0] + gn[1]))
    assert two["iters"] == 2
    assert np.array_equal(two["cost"], cost[:2]) and np.array_equal(two["gradnorm"], gn[:2])


def _run_ranks(tmp_path, world, kind, dataset, R, r, sweeps, X0, how):
    np.save(os.path.join(tmp_path, "X0.npy"), X0)
    job = "ct%s" % uuid.uuid4().hex[:12]
    envv = dict(os.environ)
    envv["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    envv.pop("DCORA_EXCHANGE", None)
    procs = [subprocess.Popen([sys.executable, WORKER, str(k), str(world), job, kind, dataset, str(R), str(r), str(sweeps),
                               str(tmp_path), how], env=envv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for k in range(world)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode(errors="replace"))
    for k, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (k, outs[k][-3000:])
    return [np.load(os.path.join(tmp_path, "%s_rank%d.npz" % (how, k))) for k in range(world)]


@pytest.mark.parametrize("case,hows", [("ring", ("run", "loop")), (("torus3D", 8), ("run",))], ids=["ring", "torus3D"])
def test_coloured_ranks_reproduce_the_single_session(env, tmp_path, case, hows):
    """2 ranks on one node: Exchange.run_coloured, and a loop of Exchange.tick + Exchange.evaluate, each against the
    single-process session (the assertions of test_exchange_gpu.test_ranks_reproduce_single_session)"""
    da, orc = env
    make, X0, (kind, dataset, R, r) = _case(da, tmp_path, case)
    sweeps = 3
    s = make()
    s.set_X(X0)
    cost, gn = _hand_loop(s, sweeps)
    X = s.get_X()
    s.close()
    for how in hows:
        res = _run_ranks(str(tmp_path), 2, kind, dataset, R, r, sweeps, X0, how)
        for k, o in enumerate(res):
            assert np.allclose(o["cost"], cost, rtol=1e-11, atol=0), (how, k, o["cost"], cost)
            assert np.allclose(o["gradnorm"], gn, rtol=1e-9, atol=0), (how, k, o["gradnorm"], gn)
            assert np.array_equal(o["X"], X), "%s, rank %d: iterates differ from the single session (max %g)" % (
                how, k, np.max(np.abs(o["X"] - X)))
            assert np.array_equal(o["cost"], res[0]["cost"]) and np.array_equal(o["gradnorm"], res[0]["gradnorm"])
        assert sum(int(o["posts"]) for o in res) > 0


def test_coloured_driver_certifies_sphere2500_from_the_chordal_start(env):
    """multi_robot_example(mode="coloured"): chordal initialisation -> 5 agents, 2 colours, at r = 5 -> certificate.  The
    oracle (orc.run_coloured, the same sweeps on the CPU) first sees |rgrad| < 0.1 after 68 sweeps, at 2 f = 1687.0128."""
    da, orc = env
    from dcora_amd import driver
    ds, dso = common.product_dataset("sphere2500"), common.oracle_dataset("sphere2500")
    r = 5
    X0 = np.zeros((r, 4 * ds.n))
    X0[:3] = da.chordal_initialization(ds)
    out = driver.multi_robot_example(ds, X0, num_robots=5, r_min=r, max_iters=200, rgrad_tol=0.1, mode="coloured")
    want = orc.run_coloured(dso, X0, num_robots=5, r=r, sweeps=200, threads=5)
    below = np.flatnonzero(want["gradnorm"] < 0.1)
    oracle_sweeps = int(below[0]) + 1 if below.size else None
    lev = out["levels"][-1]
    msg = "product: %d sweeps (|rgrad| %.4f, 2f %.4f); oracle: %s sweeps" % (lev["iterations"], lev["gradnorm"],
                                                                              lev["cost_2f"], oracle_sweeps)
    print(msg)
    assert out["certified"] and out["rank"] == 5 and len(out["levels"]) == 1, msg
    assert lev["mode"] == "coloured" and lev["iterations"] < 200 and lev["gradnorm"] < 0.1, msg
    assert abs(lev["cost_2f"] - 1687.02) < 0.05, msg
    assert np.all(out["selected"] == -1) and out["total_iters"] == lev["iterations"]


@pytest.mark.parametrize("name", ["range_aided_slam_test_2d", "range_aided_slam_test_3d"])
def test_coloured_raslam_driver_reaches_the_certified_optimum(env, name):
    """multi_robot_raslam_example(mode="coloured") from the random start of
    test_ra_session.test_multi_robot_raslam_driver_reaches_the_certified_optimum.  A numpy loop over the oracle's local
    solver that alternates the two agents certifies 2d at rank 3 after 13 + 110 sweeps and 3d at rank 4 after 47 + 189."""
    da, orc = env
    from dcora_amd import driver
    ra = da.RADataset(ra_path(name))
    d = ra.d
    rng = np.random.default_rng(12)
    X0 = orc.project_to_manifold(d, d, ra.n, rng.standard_normal((d, ra.k)), l=ra.l, b=ra.b)
    out = driver.multi_robot_raslam_example(ra, X0, max_iters=600, rgrad_tol=1e-3, r_max=d + 5, mode="coloured")
    msg = "sweeps per level: %s" % [(lv["rank"], lv["iterations"], lv["cost_2f"], lv["certified"]) for lv in out["levels"]]
    print(msg)
    assert out["certified"], msg
    assert all(lv["mode"] == "coloured" for lv in out["levels"])
    assert out["levels"][-1]["cost_2f"] < 1e-3, msg


def test_cpp_drivers_run_coloured(env, tmp_path):
    """--coloured of the two C++ staircase drivers: exit 0, a certified level, and the Python driver's sweeps and cost"""
    da, orc = env
    from dcora_amd import driver
    out = subprocess.run([os.path.join(EXAMPLES, "multi-robot-example"), "5", common.plain_path("smallGrid3D"), "--rank", "5",
                          "--quiet", "--coloured"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["certified"] and "global minimizer" in out.stdout
    ds = common.product_dataset("smallGrid3D")
    X0 = np.zeros((5, (ds.d + 1) * ds.n))
    X0[:ds.d] = da.chordal_initialization(ds)
    ref = driver.multi_robot_example(ds, X0, num_robots=5, r_min=5, max_iters=1000, rgrad_tol=0.1, mode="coloured")
    assert ref["certified"] and res["rank"] == ref["rank"] and res["iterations"] == ref["total_iters"]
    assert abs(res["cost_2f"] - ref["cost"][-1]) <= 1e-9 * abs(ref["cost"][-1])

    plain = str(tmp_path / "ra3d.pyfg")
    with open(plain, "wb") as dst, gzip.open(ra_path("range_aided_slam_test_3d"), "rb") as src:
        shutil.copyfileobj(src, dst)
    out = subprocess.run([os.path.join(EXAMPLES, "multi-robot-example-raslam"), plain, "--quiet", "--iters", "600",
                          "--rgrad-tol", "1e-3", "--coloured"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["certified"] and "global minimizer" in out.stdout, out.stdout[-2000:]
    ra = da.RADataset(ra_path("range_aided_slam_test_3d"))
    ref = driver.multi_robot_raslam_example(ra, ra.X_odom, max_iters=600, rgrad_tol=1e-3, r_max=ra.d + 12, mode="coloured")
    assert ref["certified"] and res["rank"] == ref["rank"] and res["iterations"] == ref["total_iters"]
    assert abs(res["cost_2f"] - ref["levels"][-1]["cost_2f"]) <= 1e-9 + 1e-6 * abs(ref["levels"][-1]["cost_2f"])
