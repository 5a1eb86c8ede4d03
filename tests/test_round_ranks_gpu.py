"""Rounding across the ranks of a job (dcora_exchange_round; ref examples/MultiRobotExample.cpp:341-347,
examples/MultiRobotExample_RASLAM.cpp:488-495, src/Agent.cpp:1014-1033): every rank rounds the states of the agents it
hosts, from those agents' own blocks, against an anchor that travels from its hosting rank.

One process per rank, all on device 0.  After set_X the job runs 3 greedy iterations, so the ranks' mirrors differ away
from their hosted and the neighbours' public columns: a rank that rounded from its mirror would return other bits.
Every comparison is bit for bit: the kernel forms every element as one sum in index order, whoever hosts the pose, and
the anchor's words arrive unchanged (x + 0; a -0 as +0, which changes no sum)."""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import common
import session_round_inputs as sri
from test_raslam import ra_path

pytestmark = pytest.mark.gpu

WORKER = os.path.join(common.HERE, "round_ranks_worker.py")
UNSUPPORTED, BAD_ARG = 8, 1
RA_NAME = "range_aided_slam_test_2d"


@pytest.fixture(scope="module")
def env(built):
    import dcora_amd as da
    from oracle import orc
    if da.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return da, orc


def run_ranks(tmp_path, world, cfg, X0, transport=None):
    d = str(tmp_path)
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "X0.npy"), X0)
    with open(os.path.join(d, "job.json"), "w") as f:
        json.dump(cfg, f)
    job = "r%s" % uuid.uuid4().hex[:12]
    env_ = dict(os.environ)
    env_["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env_["DCORA_EXCHANGE_TIMEOUT_S"] = "60"
    env_.pop("DCORA_EXCHANGE_WAIT", None)
    if transport:
        env_["DCORA_EXCHANGE"] = transport
    else:
        env_.pop("DCORA_EXCHANGE", None)
    procs = [subprocess.Popen([sys.executable, WORKER, str(k), str(world), job, d], env=env_, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for k in range(world)]
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
    return [np.load(os.path.join(d, "rank%d.npz" % k)) for k in range(world)]


class Case:
    """a job's start point and what the single-process session returns after the same 3 iterations"""

    def __init__(self, da, orc, kind):
        self.kind = kind
        if kind == "pgo":
            ds = common.product_dataset("smallGrid3D")
            self.d, self.n, self.r = ds.d, ds.n, 5
            self.cfg = dict(kind="pgo", name="smallGrid3D", R=5, r=5, pre=3, greedy=5)
            self.X0 = common.random_point(5, ds.d, ds.n, 4, orc.project_to_manifold)
            s = da.RbcdSession(ds, num_robots=5, r=5)
            X0se = self.X0
        else:
            ra = da.RADataset(ra_path(RA_NAME))
            self.d, self.n, self.r = ra.d, ra.n, ra.d + 2
            self.cfg = dict(kind="ra", path=ra_path(RA_NAME), r=self.r, pre=3, greedy=5)
            rng = np.random.default_rng(4)
            self.X0 = orc.project_to_manifold(self.r, ra.d, ra.n, rng.uniform(-1, 1, (self.r, ra.k)), l=ra.l, b=ra.b)
            s = da.RaRbcdSession(ra, self.r)
            X0se = sri.se_from_ra(self.X0, ra.d, ra.n, ra.l)
        s.set_X(self.X0)
        s.run(max_iters=3, rgrad_tol=0.0)
        self.X = s.get_X()
        explicit = sri.anchor_of(X0se, self.d, 1)
        self.ref = dict(first=s.round(), last=s.round(anchor_pose=self.n - 1), explicit=s.round(anchor=explicit))
        g = s.run(max_iters=5, rgrad_tol=0.0)
        self.after = dict(g_cost=g["cost"], g_selected=g["selected"], X_greedy=s.get_X())
        s.close()
        self.keys = ["trajectory"] + (["unit_spheres", "landmarks"] if kind == "ra" else [])


@pytest.fixture(scope="module")
def cases(env):
    da, orc = env
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = Case(da, orc, kind)
        return made[kind]
    return get


@pytest.mark.parametrize("kind,world,transport", [("pgo", 2, None), ("pgo", 2, "staged"), ("pgo", 4, None),
                                                  ("pgo", 4, "staged"), ("ra", 2, None), ("ra", 2, "staged")])
def test_ranks_round_to_the_single_process_bits(env, cases, tmp_path, kind, world, transport):
    """anchors: pose 0, the last pose (hosted by the last rank that hosts anything: the anchor travels), an explicit
    host anchor; the refusals, identical on every rank; and the job goes on as the single-process session does"""
    case = cases(kind)
    res = run_ranks(tmp_path, world, case.cfg, case.X0, transport=transport)
    for k, o in enumerate(res):
        assert np.array_equal(o["X"], case.X), k  # the same iterate: the comparison below is of the rounding alone
        for label in ("first", "last", "explicit"):
            for key in case.keys:
                got, want = o["%s_%s" % (label, key)], case.ref[label][key]
                assert got.shape == want.shape and np.array_equal(got, want), (k, label, key, np.abs(got - want).max())
        for key in case.keys:
            assert np.array_equal(o["again_" + key], o["first_" + key]), (k, key)
        assert list(o["status"]) == [BAD_ARG] * 4 + [UNSUPPORTED], (k, o["status"])
        assert np.array_equal(o["g_selected"], case.after["g_selected"]), k
        assert np.array_equal(o["X_greedy"], case.after["X_greedy"]), k


@pytest.mark.parametrize("kind", ["pgo", "ra"])
def test_a_job_that_rounded_goes_on_as_its_twin_that_never_did(env, cases, tmp_path, kind):
    case = cases(kind)
    A = run_ranks(tmp_path / "rounded", 2, case.cfg, case.X0)
    B = run_ranks(tmp_path / "twin", 2, dict(case.cfg, round=False), case.X0)
    for k in range(2):
        a, b = A[k], B[k]
        for key in ("X", "X_greedy", "g_cost", "g_gradnorm", "g_selected"):
            assert np.array_equal(a[key], b[key]), (k, key)
        assert "first_trajectory" in a.files and "first_trajectory" not in b.files
        print("%s rank %d: launches with the roundings %d, without %d" % (kind, k, int(a["launches"]), int(b["launches"])))
