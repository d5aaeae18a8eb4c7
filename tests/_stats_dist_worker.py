"""Worker for tests/test_statistics_dist.py (launched by torch.distributed.run, one process per rank, every rank on cuda:0, gloo with
host staging): a nested tunnel with a sphere stepped by case.DistributedStepper, time-averaged statistics sampled on every rank's
owned blocks and gathered to rank 0, which writes them to <outdir>/sums.npz. Every rank writes <outdir>/rank<r>.npz with the
Bouzidi cells it owns per level."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch.distributed as dist

SAMPLES = (2, 3, 6, 9, 10)
STEPS = 10
U = 0.05


def main():
    outdir, levels = sys.argv[1], int(sys.argv[2])
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    from open_ludwig_amd import case, cases
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    st = case.DistributedStepper(grids, device=0, stage_through_host=True)
    for t in range(1, STEPS + 1):
        st.batch(t, 1, np.float32(U), params)
        if t == SAMPLES[0]:
            st.stats_reset()
        if t in SAMPLES:
            st.stats_sample(t)
    out = {}
    for lvl in range(levels):
        sums = st.stats_sums(lvl)                      # collective
        if rank == 0:
            r, u, uu, n = sums
            out.update({f"rho{lvl}": r, f"vel{lvl}": u, f"vel2{lvl}": uu, f"n{lvl}": np.array(n)})
    if rank == 0:
        np.savez(os.path.join(outdir, "sums.npz"), **out)
    nbc = [lv.n_boundary_cells if lv is not None and st.runner.views[i].n_owned > 0 else 0 for i, lv in enumerate(st.runner.levels)]
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), nbc=np.array(nbc))
    st.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
