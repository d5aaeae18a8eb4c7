"""Worker for tests/test_probes_dist.py (launched by torch.distributed.run, one process per rank, every rank on cuda:0, gloo with host
staging): a nested tunnel with a sphere stepped by case.DistributedStepper with probes whose stencils straddle the cut, in batches of
BATCH coarse steps; the series is gathered before the first batch, after a batch that sampled nothing and at the end; rank 0 writes
them to <outdir>/series.npz."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch.distributed as dist

U, LEVELS, STEPS, BATCH, START, INTERVAL = 0.05, 2, 8, 4, 5, 1      # the first batch samples nothing


def main():
    outdir = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    import _probes_common as common
    from open_ludwig_amd import case, cases, partition
    grids, params = cases.tunnel_with_sphere(levels=LEVELS, wall_model=True)
    plan = common.straddling_points(grids, partition.level_owners(grids, dist.get_world_size()))
    st = case.DistributedStepper(grids, device=0, stage_through_host=True)
    st.probes_setup(plan, START, INTERVAL, capacity=3)          # a batch of 4 samples drains the ring once inside the batch
    early = [st.probes_series()]                                # collective: before the first batch, and after a batch without samples
    for t in range(1, STEPS + 1, BATCH):
        st.batch(t, BATCH, np.float32(U), params)
        if t < START:
            early.append(st.probes_series())
    res = st.probes_series()                                    # collective
    n_mine = 0 if st.probes is None else st.probes.n_probes
    if rank == 0:
        np.savez(os.path.join(outdir, "series.npz"), steps=res[0], values=res[1],
                 early_steps=np.array([e[0].size for e in early]), early_shapes=np.array([e[1].shape for e in early]))
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), n_mine=np.array(n_mine))
    st.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
