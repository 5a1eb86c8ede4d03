"""one rank of a two-rank job of tools/record_session_blocks.py (ranked(): iterations, gather_X, round, certify, lift, the
rounds after it, through the exchange); started by that tool's run_ranks -- from tests/test_session_blocks_gpu.py or from
the tool's command line -- and by nothing else.  argv: rank world job dir.  dir holds job.json (workload, robust, lib:
another build's library or null); the rank writes rank<k>.npz there."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))


def main():
    rank, world, job, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import record_session_blocks as rec
    cfg = json.load(open(os.path.join(out_dir, "job.json")))
    if cfg.get("lib"):
        rec.use_library(cfg["lib"])
    import dcora_amd as da
    w = rec.Workload(da, rec.WORKLOADS[cfg["workload"]])
    out = rec.ranked(da, w, rank, world, job, cfg["robust"])
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)


if __name__ == "__main__":
    main()
