"""Slices on 2 ranks (both on the one MI355X, gloo with host staging): a point belongs to the rank that owns its base cell's block; its
corners and their face neighbours in the peer's blocks are read from the ghost copies the 'rho' / 'vel' halo refreshes (those cells
join the halo plans only when slices are configured), and DistributedStepper.slices_sample gathers to rank 0 in plane order. The
gathered samples - vorticity and Q included - equal one device's bit for bit only if every one of those ghost cells is current."""
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import case, cases, partition, slices as sl

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dist_launch import run_ranks  # noqa: E402


def test_two_rank_layout_reaches_peer_blocks():
    """CPU check of the layout the GPU test relies on. The cut runs across x and corners lie at +0 / +1 of the base cell, so on every
    level rank 0 has points with corners in rank 1's blocks, and both ranks have points whose corners are all their own but whose
    face neighbours (read only for the gradient) lie in the peer's blocks"""
    import _slices_dist_worker as w
    grids, _ = cases.tunnel_with_sphere(levels=w.LEVELS, wall_model=True)
    owners = partition.level_owners(grids, 2)
    plans = w.planes(grids)
    corner_peer = np.zeros((w.LEVELS, 2), int)
    neighbour_only = np.zeros((w.LEVELS, 2), int)
    for plan in plans:
        for p in np.flatnonzero(plan.valid)[::3]:
            li = int(plan.level[p])
            own = np.asarray(owners[li])
            base = int(own[plan.blocks[p, 0]])
            corners = set(own[plan.blocks[p]].tolist())
            if corners != {base}:
                corner_peer[li, base] += 1
            elif plan.gradient:
                cells = sl.stencil_cells(plan, np.array([p]), grids[li])
                neighbour_only[li, base] += int((own[cells // 512] != base).any())
    assert (corner_peer[:, 0] > 0).all() and (neighbour_only > 0).all()


@pytest.mark.gpu
def test_two_rank_slices_equal_single_device(gpu, tmp_path):
    import _slices_dist_worker as w
    res = run_ranks("_slices_dist_worker.py", 2, tmp_path)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    got = np.load(os.path.join(tmp_path, "slices.npz"))
    mine = [int(np.load(os.path.join(tmp_path, f"rank{r}.npz"))["n_mine"]) for r in range(2)]
    assert all(m > 0 for m in mine)                                  # both ranks own points

    grids, params = cases.tunnel_with_sphere(levels=w.LEVELS, wall_model=True)
    plans = w.planes(grids)
    assert sum(mine) == sum(int(p.valid.sum()) for p in plans)
    st = case.HipStepper(grids)
    try:
        st.slices_setup(plans, w.SAMPLED[0], 1)
        st.batch(1, w.FIRST, np.float32(w.U), params)
        for t in w.SAMPLED:
            st.batch(t, 1, np.float32(w.U), params)
            for k, v in enumerate(st.slices_sample(t)):
                g = got[f"t{t}_p{k}"]
                assert g.shape == v.shape == (9, plans[k].n)
                assert np.array_equal(g.view(np.uint32), v.view(np.uint32)), \
                    f"step {t} plane {k}: rows {np.unique(np.nonzero(g.view(np.uint32) != v.view(np.uint32))[0])}"
                assert np.abs(v[8, plans[k].valid]).max() > 0 and np.abs(v[1, plans[k].valid]).max() > 1e-3
    finally:
        st.close()
