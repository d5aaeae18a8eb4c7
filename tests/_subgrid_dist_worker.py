"""Worker for tests/test_subgrid_dist.py (launched by torch.distributed.run, one process per rank, every rank on cuda:0, gloo with host
staging): a nested tunnel with a sphere stepped by case.DistributedStepper. After coarse steps ODD_EVEN every rank evaluates the
subgrid fields of its owned blocks from both velocity buffers and adds a sample to its sums; rank 0 writes the gathered fields and
the gathered sums to <outdir>/subgrid.npz. Every rank writes to <outdir>/rank<r>.npz how many of its owned blocks read a ghost block."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch.distributed as dist

ODD_EVEN = (3, 4)
U = 0.05


def main():
    outdir, levels = sys.argv[1], int(sys.argv[2])
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    from _gradient_dist_worker import _ghost_readers
    from open_ludwig_amd import case, cases
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    st = case.DistributedStepper(grids, device=0, stage_through_host=True)
    out, mine = {}, {}
    for t in range(1, max(ODD_EVEN) + 1):
        st.batch(t, 1, np.float32(U), params)
        if t == 1:
            st.subgrid_stats_reset()
        if t not in ODD_EVEN:
            continue
        st.subgrid_stats_sample(t)
        for lvl in range(levels):
            for vel_name in ("vel", "vel_temp"):
                res = st.subgrid_fields(lvl, vel_name)                            # collective
                if rank == 0:
                    out[f"nu_{t}_{lvl}_{vel_name}"], out[f"code_{t}_{lvl}_{vel_name}"] = res
            view = st.runner.views[lvl]
            if st.runner.levels[lvl] is not None and view.n_owned > 0:
                mine[f"readers_{lvl}"] = np.array(_ghost_readers(view.level.neighbor_table, view.n_owned).size)
                mine[f"owned_{lvl}"] = np.array(view.n_owned)
    for lvl in range(levels):
        sums = st.subgrid_stats_sums(lvl)                                         # collective
        if rank == 0:
            out[f"s_nu_{lvl}"], out[f"s_nunu_{lvl}"], out[f"s_eps_{lvl}"] = sums[:3]
            out[f"n_{lvl}"] = np.array(sums[3])
    if rank == 0:
        np.savez(os.path.join(outdir, "subgrid.npz"), **out)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **mine)
    st.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
