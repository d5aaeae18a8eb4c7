"""Worker for tests/test_force_series_dist.py (launched by torch.distributed.run, one process per rank, every rank on cuda:0, gloo with
host staging): the 2-level wall-modelled tunnel, cut across the sphere, stepped by case.DistributedStepper with a force series of
capacity 2 (so the ring is drained inside the batch too); rank 0 writes the gathered series to <outdir>/series.npz, every rank what it
owns."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch.distributed as dist

FIRST, LAST, INTERVAL = 28, 34, 2              # the steppers start from rest: the flow reaches the sphere before the first record
SAMPLED = tuple(range(FIRST, LAST + 1, INTERVAL))


def setup():
    """(grids, params, mesh, physical scales, inlet speed) of the case"""
    import _surface_common as common
    import _wall_cases as wc
    _, grids, params, _, u = wc.tunnel_two_levels()
    mesh, center, radius = common.tunnel_sphere_mesh(grids)
    return grids, params, mesh, common.tunnel_params(center, radius), u


def main():
    outdir = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    from open_ludwig_amd import case
    grids, params, mesh, sparams, u = setup()
    st = case.DistributedStepper(grids, device=0, stage_through_host=True)
    st.force_series_setup(mesh, sparams, FIRST, INTERVAL, capacity=2)
    st.batch(1, LAST - 3, u, params)
    first = st.force_series_new()                                             # collective: the records of the first batch only
    st.batch(LAST - 2, 3, u, params)
    got = st.force_series()                                                   # collective: the whole history
    if rank == 0:
        assert first[0].tolist() == [t for t in SAMPLED if t <= LAST - 3] and np.array_equal(got[1][: first[0].size], first[1])
        assert st._fseries.take_new()[0].size == 0                            # everything local was handed over once
    if rank == 0:
        np.savez(os.path.join(outdir, "series.npz"), steps=got[0], sums=got[1], covered=got[2])
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), n_tri=np.array(int(st._forces_sel.size)))
    st.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
