"""Wall diagnostics on 2 ranks (both on the one MI355X, gloo with host staging): every rank takes the census of its owned blocks and
evaluates the triangles whose cell it owns; the merged census of both levels and the gathered per-triangle values equal one device's
exactly - the record is integers, and a triangle's values depend on its own cell alone."""
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import case, partition, surface_stats as ss

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dist_launch import run_ranks  # noqa: E402


def test_two_rank_cut_runs_across_the_sphere():
    """CPU check of the layout the GPU test relies on: both ranks own near-wall cells of both levels and triangles of the body"""
    import _wall_dist_worker as w
    grids, params, mesh, sparams, _ = w.setup()
    owners = partition.level_owners(grids, 2)
    for g, own in zip(grids, owners):
        near = ((g.wall_dist > 0) & (g.wall_dist < 10) & ~g.obstacle).any(axis=(0, 1, 2))
        assert all((near & (np.asarray(own) == r)).any() for r in (0, 1)), g.level_id
    plan = ss.plan_surface(mesh, grids[-1], sparams)
    tri_owner = np.asarray(owners[-1])[plan.blocks[plan.found]]
    assert (tri_owner == 0).sum() > 50 and (tri_owner == 1).sum() > 50


@pytest.mark.gpu
def test_two_rank_census_and_triangle_values_equal_single_device(gpu, tmp_path):
    import _wall_dist_worker as w
    res = run_ranks("_wall_dist_worker.py", 2, tmp_path)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    got = np.load(os.path.join(tmp_path, "wall.npz"))
    mine = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2)]
    assert all(int(m["n_tri"]) > 0 and (m["n_blocks"] > 0).all() for m in mine)          # both ranks own triangles and blocks of both levels

    grids, params, mesh, sparams, u = w.setup()
    st = case.HipStepper(grids)
    try:
        plan = st.wall_diagnostics_setup(mesh, sparams)
        assert sum(int(m["n_tri"]) for m in mine) == int(plan.found.sum())
        st.batch(1, w.FIRST, u, params)
        for t in w.SAMPLED:
            st.batch(t, 1, u, params)
            for lvl in range(len(grids)):
                one = st.wall_census(lvl, t)
                assert np.array_equal(got[f"t{t}_census{lvl}"], w.pack(one)), f"step {t} level {lvl + 1}"
                assert one.evaluated > 0
            v = st.wall_surface_values(t)
            g2 = got[f"t{t}_values"]
            assert g2.shape == v.shape == (7, plan.n)
            assert np.array_equal(g2.view(np.uint32), v.view(np.uint32)), f"step {t}: rows {np.unique(np.nonzero(g2.view(np.uint32) != v.view(np.uint32))[0])}"
            assert ((v[6].astype(int) & 3) >= 2).sum() > plan.n // 2 and np.abs(v[1:4]).max() > 0
    finally:
        st.close()
