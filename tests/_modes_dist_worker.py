"""Worker for tests/test_modes_dist.py (launched by torch.distributed.run, one process per rank, every rank on cuda:0, gloo with host
staging): a nested tunnel with a sphere stepped by case.DistributedStepper with a mode set, every rank accumulating its owned blocks
inside batch(); the sums are gathered to rank 0, which writes them to <outdir>/sums.npz. Every rank writes <outdir>/rank<r>.npz with
the Bouzidi cells it owns per level."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch.distributed as dist

START, INTERVAL, STEPS = 2, 3, 9          # samples after coarse steps 2, 5, 8
N_ROWS, N_COLUMNS = 4, 3
U = 0.05


def table():
    W = np.random.default_rng(5).uniform(-1.0, 1.0, (N_ROWS, N_COLUMNS))
    W[1, 1] = 0.0
    return W


def main():
    outdir, levels = sys.argv[1], int(sys.argv[2])
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    from open_ludwig_amd import case, cases
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    st = case.DistributedStepper(grids, device=0, stage_through_host=True)
    st.modes_setup(table(), START, INTERVAL)
    st.batch(1, 4, np.float32(U), params)
    st.batch(5, STEPS - 4, np.float32(U), params)
    out = {}
    for lvl in range(levels):
        got = st.modes_sums(lvl)                       # collective
        if rank == 0:
            sums, n = got
            out.update({f"s{lvl}_{m}": a for m, a in enumerate(sums)})
            out[f"n{lvl}"] = np.array(n)
    if rank == 0:
        np.savez(os.path.join(outdir, "sums.npz"), **out)
    nbc = [lv.n_boundary_cells if lv is not None and st.runner.views[i].n_owned > 0 else 0 for i, lv in enumerate(st.runner.levels)]
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), nbc=np.array(nbc))
    st.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
