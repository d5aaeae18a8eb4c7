"""Worker for tests/test_wall_diagnostics_dist.py (launched by torch.distributed.run, one process per rank, every rank on cuda:0, gloo
with host staging): the 2-level wall-modelled tunnel, cut across the sphere, stepped by case.DistributedStepper; rank 0 writes the merged
census of both levels and the gathered per-triangle values after coarse steps SAMPLED to <outdir>/wall.npz, every rank what it owns."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch.distributed as dist

FIRST, SAMPLED = 30, (31, 32)                  # the steppers start from rest: FIRST steps bring the inlet's flow to the sphere, then one
                                               # step per sample (odd and even)
COUNTS = ("near_cells", "evaluated", "log_law", "forced", "non_finite", "min_bits", "max_bits")


def setup():
    """(grids, params, mesh, physical scales) of the case"""
    import _surface_common as common
    import _wall_cases as wc
    _, grids, params, _, u = wc.tunnel_two_levels()
    mesh, center, radius = common.tunnel_sphere_mesh(grids)
    return grids, params, mesh, common.tunnel_params(center, radius), u


def pack(rec):
    return np.array([getattr(rec, n) for n in COUNTS] + [int(v) for v in rec.hist], dtype=np.uint64)


def main():
    outdir = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    from open_ludwig_amd import case
    grids, params, mesh, sparams, u = setup()
    st = case.DistributedStepper(grids, device=0, stage_through_host=True)
    st.wall_diagnostics_setup(mesh, sparams)
    st.batch(1, FIRST, u, params)
    got = {}
    for t in SAMPLED:
        st.batch(t, 1, u, params)
        recs = [st.wall_census(lvl, t) for lvl in range(len(grids))]          # collective
        vals = st.wall_surface_values(t)                                      # collective
        if rank == 0:
            got[f"t{t}_values"] = vals
            for lvl, rec in enumerate(recs):
                got[f"t{t}_census{lvl}"] = pack(rec)
    n_tri = int(st._wall_sel.size)
    n_blocks = [int(v.n_owned) if v is not None else 0 for v in st.runner.views]
    if rank == 0:
        np.savez(os.path.join(outdir, "wall.npz"), **got)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), n_tri=np.array(n_tri), n_blocks=np.array(n_blocks))
    st.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
