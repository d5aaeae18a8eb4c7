"""Worker for tests/test_monitor_dist.py (launched by torch.distributed.run, one process per rank, every rank on cuda:0, gloo with host
staging): a nested tunnel with a sphere stepped by case.DistributedStepper; after coarse steps SAMPLED every level's flow-monitor
record is reduced per rank and merged (DistributedStepper.monitor). Every rank writes what it received to <outdir>/rank<r>.pkl."""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch.distributed as dist

U, LEVELS, SAMPLED = 0.05, 2, (3, 4)        # an odd and an even coarse step


def main():
    outdir = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    from open_ludwig_amd import case, cases
    grids, params = cases.tunnel_with_sphere(levels=LEVELS, wall_model=True)
    st = case.DistributedStepper(grids, device=0, stage_through_host=True)
    got = {}
    for t in range(1, SAMPLED[-1] + 1):
        st.batch(t, 1, np.float32(U), params)
        if t in SAMPLED:
            for lvl in range(LEVELS):
                got[(t, lvl)] = st.monitor(lvl, t)              # collective; the merged record on every rank
    owned = [int(st.runner.views[lvl].n_owned) for lvl in range(LEVELS)]
    with open(os.path.join(outdir, f"rank{rank}.pkl"), "wb") as fh:
        pickle.dump({"records": got, "owned": owned}, fh)
    st.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
