"""Worker for tests/test_surface_stats_dist.py (launched by torch.distributed.run, one process per rank, every rank on cuda:0, gloo
with host staging): a nested tunnel with a sphere stepped by case.DistributedStepper, surface statistics accumulated by every rank on
the triangles whose cell it owns and gathered to rank 0, which writes them to <outdir>/sums.npz. Every rank writes <outdir>/rank<r>.npz
with the number of triangles it accumulates."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch.distributed as dist

START, INTERVAL, STEPS, BATCH = 2, 3, 11, 4
U = 0.05


def main():
    outdir, levels = sys.argv[1], int(sys.argv[2])
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    import _surface_common as common
    from open_ludwig_amd import case, cases
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    mesh, center, radius = common.tunnel_sphere_mesh(grids)
    sparams = common.tunnel_params(center, radius)
    st = case.DistributedStepper(grids, device=0, stage_through_host=True)
    st.surface_stats_setup(mesh, sparams, START, INTERVAL)
    early = st.surface_stats_sums()                    # collective, before the first batch
    for t in range(1, STEPS + 1, BATCH):
        st.batch(t, min(BATCH, STEPS + 1 - t), np.float32(U), params)
    got = st.surface_stats_sums()                      # collective
    if rank == 0:
        np.savez(os.path.join(outdir, "sums.npz"), sums=got[0], n=np.array(got[1]), early_n=np.array(early[1]))
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), n_tri=np.array(st.surface.n_tri if st.surface is not None else 0))
    st.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
