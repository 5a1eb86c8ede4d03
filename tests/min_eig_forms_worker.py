"""one child process of tools/record_min_eig.py: `single dir` (every one-process case, in the form of the Lanczos cycle
that the environment chooses) or `rank dir k world job` (one rank of a two-rank job); started by that tool's
compute_case -- from tests/test_min_eig_forms_gpu.py or from the tool's command line -- and by nothing else.  dir holds
job.json (lib: another build's library or null; workload); the child writes single.npz or rank<k>.npz there."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))


def main():
    mode, out_dir = sys.argv[1], sys.argv[2]
    import record_min_eig as me
    cfg = json.load(open(os.path.join(out_dir, "job.json")))
    if cfg.get("lib"):
        me.rec.use_library(cfg["lib"])
    import dcora_amd as da
    if da.device_count() < 1:
        raise SystemExit("no GPU visible: these cases run on the device")
    if mode == "single":
        np.savez(os.path.join(out_dir, "single.npz"), **me.single(da))
    else:
        rank, world, job = int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
        w = me.rec.Workload(da, me.rec.WORKLOADS[cfg["workload"]])
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **me.ranked(da, w, rank, world, job))


if __name__ == "__main__":
    main()
