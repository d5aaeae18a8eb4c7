"""Worker for tests/test_slices_dist.py (launched by torch.distributed.run, one process per rank, every rank on cuda:0, gloo with host
staging): a nested tunnel with a sphere stepped by case.DistributedStepper with slices whose planes cross the cut on every level;
rank 0 writes the gathered samples after coarse steps SAMPLED to <outdir>/slices.npz, every rank its number of own points."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch.distributed as dist

U, LEVELS, FIRST, SAMPLED = 0.05, 2, 4, (5, 6)       # one batch of FIRST steps, then one step per sample (odd and even)


def planes(grids):
    """an xy plane through the sphere with every field and an xz plane with density and Q: both cross the cut (along x) on every level"""
    from open_ludwig_amd import preprocess as pp, slices as sl
    return [sl.plan_slice(pp.SlicePlane("z", 2, 16.05, ((0.2, 47.8), (0.3, 31.7)), 0.173, pp.SLICE_FIELDS), grids),
            sl.plan_slice(pp.SlicePlane("y", 1, 13.37, ((1.0, 40.0), (2.0, 30.0)), 0.29, ("density", "q_criterion")), grids)]


def main():
    outdir = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    from open_ludwig_amd import case, cases
    grids, params = cases.tunnel_with_sphere(levels=LEVELS, wall_model=True)
    st = case.DistributedStepper(grids, device=0, stage_through_host=True)
    st.slices_setup(planes(grids), SAMPLED[0], 1)
    st.batch(1, FIRST, np.float32(U), params)
    got = {}
    for t in SAMPLED:
        st.batch(t, 1, np.float32(U), params)
        got[t] = st.slices_sample(t)                            # collective
    n_mine = int(sum(m.sum() for m in st._slice_mine_cache))
    if rank == 0:
        np.savez(os.path.join(outdir, "slices.npz"), **{f"t{t}_p{k}": v for t, vals in got.items() for k, v in enumerate(vals)})
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), n_mine=np.array(n_mine))
    st.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
