"""bench.py as the driver starts it: the line of the N = 1 run and of a 2-rank rehearsal (two processes on ONE GPU over
gloo -- not a scaling figure, a check that the SCALE path runs and prints a line the driver can parse)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def run_bench(extra, env_extra=None, timeout=900):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert lines, p.stderr[-2000:]
    last = lines[-1]
    assert len(last) <= 8000
    return json.loads(last, parse_constant=lambda t: pytest.fail("non-finite constant " + t))


def test_headline_line_of_the_one_gpu_run(tmp_path):
    line = run_bench(["--steps", "20", "--warmup", "5", "--dump-outputs", str(tmp_path)])
    assert line["n_gpus"] == 1 and line["steps"] == 20 and line["warmup"] == 5 and line["value"] > 100
    for key in ("sustained", "roofline", "cpu_baseline", "coloured_rbcd", "scaling_100k_lattice"):
        assert key not in line, key  # a plain run measures only its window; side measurements need --full
    assert abs(line["value"] * line["ms_per_step"] - 1e3) < 1.0
    assert line["config"]["workload"].startswith("sphere2500") and line["vs_baseline"] is None
    with open(os.path.join(ROOT, "gpurun_out", "bench_detail.json")) as fh:
        detail = json.load(fh)
    assert abs(detail["value"] - line["value"]) <= 1e-5 * line["value"]
    check_last_step_dump(tmp_path, detail)


def test_full_run_adds_the_side_measurements():
    line = run_bench(["--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline", "--no-config3", "--no-config4",
                      "--no-config5", "--no-coloured"])
    assert line["steps"] == 20 and line["value"] > 100
    assert line["sustained"]["steps"] == 300 and line["sustained"]["value"] > 100
    assert line["roofline"]["unit"] == "GB/s" and line["roofline"]["achieved"] > 0
    assert "value" in line["ms_to_certified_optimum"]


def check_last_step_dump(path, detail):
    """the dump holds the outputs of the last timed step: the evaluation the line reports, and the whole iterate X it
    was taken at (2f recomputed from the dumped X by the CPU oracle)"""
    import numpy as np
    import common
    from oracle import orc
    X = np.load(path / "X.npy")
    assert X.dtype == np.float64 and X.shape == (5, 4 * 2500) and np.isfinite(X).all()
    c2 = float(np.load(path / "cost_2f.npy"))
    assert c2 == detail["config"]["final_cost_2f"]
    assert float(np.load(path / "gradnorm.npy")) == detail["config"]["final_gradnorm"]
    dso = common.oracle_dataset("sphere2500")
    assert abs(2 * orc.Problem(5, dso.d, dso.n, orc.build_Q_pgo(dso)).f(X) - c2) <= 1e-9 * abs(c2)
    bn = np.load(path / "block_gradnorms.npy")
    assert bn.shape == (5,) and np.isfinite(bn).all() and 0 <= int(np.load(path / "next_selected.npy")) < 5
    return X


@pytest.mark.parametrize("transport", ["library exchange", "collectives"])
def test_two_rank_dump_is_the_whole_last_step(tmp_path, transport):
    env = {"DCORA_DIST_BACKEND": "gloo"}
    if transport == "collectives":
        env["DCORA_BENCH_COLLECTIVES"] = "1"
    line = run_bench(["--gpus", "2", "--steps", "6", "--warmup", "2", "--dump-outputs", str(tmp_path)], env)
    assert line["n_gpus"] == 2 and line["steps"] == 6
    fallback = line["process_group"]["transport"] == "torch.distributed collectives (fallback)"
    assert fallback == (transport == "collectives"), line["process_group"]
    import bench
    with open(bench.DETAIL_PATH) as fh:  # where bench.py leaves the whole line
        check_last_step_dump(tmp_path, json.load(fh))


def test_two_rank_rehearsal_prints_the_scaling_series():
    line = run_bench(["--gpus", "2", "--steps", "10", "--warmup", "3", "--full", "--scaling-only"],
                     {"DCORA_DIST_BACKEND": "gloo"})
    assert line["n_gpus"] == 2 and line["value"] > 50
    sc = line["scaling_100k_lattice"]
    assert sc["agents"] == 16 and sc["n_gpus"] == 2 and sc["sweeps_per_s"] > 1, sc
    assert line["scaling_value"] == sc["sweeps_per_s"]
    assert sc["secondary_R_2N"]["agents"] == 4 and sc["secondary_R_2N"]["sweeps_per_s"] > 1
    assert line["process_group"]["backend"] == "gloo" and line["process_group"]["ranks"] == 2
