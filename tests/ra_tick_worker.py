"""one rank of a multi-process coloured run through the library's exchange; started by tests/test_coloured_run_gpu.py and by
nothing else.  argv: rank world job kind dataset R r sweeps out_dir how -- kind "ra" (dataset: path of a .pyfg file) or
"pgo" (dataset: name of a g2o fixture, R agents); how "run" (Exchange.run_coloured) or "loop" (Exchange.tick per colour +
Exchange.evaluate from Python)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    rank, world, job, kind, dataset = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    R, r, sweeps, out_dir, how = int(sys.argv[6]), int(sys.argv[7]), int(sys.argv[8]), sys.argv[9], sys.argv[10]
    import dcora_amd as da
    X0 = np.load(os.path.join(out_dir, "X0.npy"))
    device = rank % max(da.device_count(), 1)
    if kind == "ra":
        s = da.RaRbcdSession(da.RADataset(dataset), r, acceleration=False, rank=rank, world_size=world, device=device)
    else:
        import common
        s = da.RbcdSession(common.product_dataset(dataset), num_robots=R, r=r, acceleration=False, rank=rank,
                           world_size=world, device=device)
    ex = da.Exchange(s, job)
    ex.set_X(X0)
    if how == "run":
        out = ex.run_coloured(max_sweeps=sweeps, rgrad_tol=0.0)
        cost, gn = out["cost"], out["gradnorm"]
    else:
        col, nc = s.colours()
        cost, gn = [], []
        for _ in range(sweeps):
            for c in range(nc):
                ex.tick(np.flatnonzero(col == c).astype(np.int32))
            c2, g, bn, nxt = ex.evaluate()
            cost.append(c2)
            gn.append(g)
    X = ex.gather_X()
    info = ex.info()
    ex.barrier()
    np.savez(os.path.join(out_dir, "%s_rank%d.npz" % (how, rank)), cost=np.asarray(cost), gradnorm=np.asarray(gn), X=X,
             posts=info["posts"])
    ex.close()
    s.close()


if __name__ == "__main__":
    main()
