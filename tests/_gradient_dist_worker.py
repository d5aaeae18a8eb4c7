"""Worker for tests/test_gradient_fields_dist.py (launched by torch.distributed.run, one process per rank, every rank on cuda:0, gloo
with host staging): a nested tunnel with a sphere stepped by case.DistributedStepper; after coarse steps ODD_EVEN every rank computes
the velocity-gradient fields of its owned blocks from both velocity buffers, gathered to rank 0, which writes them to
<outdir>/fields.npz. Every rank also checks its own blocks against the float32 restatement on its LOCAL velocity (ghost blocks
included) and writes to <outdir>/rank<r>.npz how many owned cells read a ghost block and whether zeroing the ghosts changes them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch.distributed as dist

ODD_EVEN = (3, 4)
U = 0.05


def _ghost_readers(table, n_owned):
    """owned blocks with a face neighbour among the ghost blocks (1-based local ids > n_owned)"""
    faces = [4, 10, 12, 14, 16, 22]
    t = np.asarray(table)[:n_owned][:, faces]
    return np.flatnonzero((t > n_owned).any(axis=1))


def main():
    outdir, levels = sys.argv[1], int(sys.argv[2])
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    import _gradient_ref as ref
    from open_ludwig_amd import case, cases
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    st = case.DistributedStepper(grids, device=0, stage_through_host=True)
    out, mine = {}, {}
    for t in range(1, max(ODD_EVEN) + 1):
        st.batch(t, 1, np.float32(U), params)
        if t not in ODD_EVEN:
            continue
        for lvl in range(levels):
            scale = np.float32(1.0 / grids[lvl].dx)
            for vel_name in ("vel", "vel_temp"):
                res = st.gradient_fields(lvl, vel_name, scale)                 # collective
                if rank == 0:
                    out[f"w_{t}_{lvl}_{vel_name}"], out[f"q_{t}_{lvl}_{vel_name}"] = res
                lv, view = st.runner.levels[lvl], st.runner.views[lvl]
                if lv is None or view.n_owned == 0:
                    continue
                n = view.n_owned
                w, q = lv.gradient_fields(vel_name, scale)
                u = lv.download(vel_name)
                rw, rq = ref.gradient_fields(u, view.level.neighbor_table, view.level.obstacle, scale)
                key = f"{t}_{lvl}_{vel_name}"
                mine[f"equal_{key}"] = np.array(np.array_equal(w[:, :, :, :n], rw[:, :, :, :n]) and np.array_equal(q[:, :, :, :n], rq[:, :, :, :n]))
                readers = _ghost_readers(view.level.neighbor_table, n)
                mine[f"readers_{key}"] = np.array(readers.size)
                u0 = u.copy()
                u0[:, :, :, n:] = 0                                            # the ghosts' values matter to the owned result
                zw, _ = ref.gradient_fields(u0, view.level.neighbor_table, view.level.obstacle, scale)
                mine[f"ghost_matters_{key}"] = np.array(not np.array_equal(zw[:, :, :, readers], w[:, :, :, readers]))
    if rank == 0:
        np.savez(os.path.join(outdir, "fields.npz"), **out)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **mine)
    st.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
