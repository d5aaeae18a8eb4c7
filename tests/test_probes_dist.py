"""Probes on 2 ranks (both on the one MI355X, gloo with host staging; RCCL needs one device per rank): a probe belongs to the rank that
owns its base cell's block, corners in the peer's blocks are read from the ghost copies the 'rho' / 'vel' halo refreshes (the probe
corners join those halo plans), and DistributedStepper.probes_series gathers to rank 0 in probe order. Most probes' stencils straddle
the cut, so the gathered series equals the single-device series bit for bit only if those corner ghosts are current."""
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import case, cases, partition

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dist_launch import run_ranks  # noqa: E402


def test_straddling_layout_reaches_peer_blocks():
    """CPU check of the layout the GPU test relies on: probes on every level, each with corners in blocks of both ranks, some of
    them in a diagonal (edge or corner) neighbour - outside the face stencil the 'vel' halo carries without probes"""
    import _probes_common as common
    import _probes_dist_worker as w
    grids, _ = cases.tunnel_with_sphere(levels=w.LEVELS, wall_model=True)
    owners = partition.level_owners(grids, 2)
    plan = common.straddling_points(grids, owners)
    assert set(plan.level.tolist()) == set(range(w.LEVELS))
    diag, straddle, base_owner = 0, np.zeros(w.LEVELS, int), set()
    for p in range(plan.n):
        own = np.asarray(owners[int(plan.level[p])])[plan.blocks[p]]
        straddle[plan.level[p]] += len(set(own.tolist())) == 2
        base_owner.add(int(own[0]))
        g = grids[int(plan.level[p])]
        base = np.array(g.active_block_coords[plan.blocks[p, 0]])
        for c in range(8):
            d = np.array(g.active_block_coords[plan.blocks[p, c]]) - base
            diag += int(np.count_nonzero(d) >= 2 and own[c] != own[0])
    assert diag > 0 and (straddle >= 6).all() and base_owner == {0, 1}


@pytest.mark.gpu
def test_two_rank_series_equals_single_device(gpu, tmp_path):
    import _probes_common as common
    import _probes_dist_worker as w
    res = run_ranks("_probes_dist_worker.py", 2, tmp_path)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    got = np.load(os.path.join(tmp_path, "series.npz"))
    # gathered before any sample: empty series of every probe, not an error
    assert got["early_steps"].tolist() == [0, 0]
    assert [tuple(s) for s in got["early_shapes"]] == [(0, got["values"].shape[1], 4)] * 2
    mine = [int(np.load(os.path.join(tmp_path, f"rank{r}.npz"))["n_mine"]) for r in range(2)]
    assert all(m > 0 for m in mine)                                  # both ranks own probes

    grids, params = cases.tunnel_with_sphere(levels=w.LEVELS, wall_model=True)
    plan = common.straddling_points(grids, partition.level_owners(grids, 2))
    st = case.HipStepper(grids)
    try:
        st.probes_setup(plan, w.START, w.INTERVAL, capacity=8)
        for t in range(1, w.STEPS + 1, w.BATCH):
            st.batch(t, w.BATCH, np.float32(w.U), params)
        steps, vals = st.probes_series()
    finally:
        st.close()
    assert steps.tolist() == list(range(w.START, w.STEPS + 1)) and np.array_equal(got["steps"], steps)
    assert np.array_equal(got["values"].view(np.uint32), vals.view(np.uint32))
    assert np.isfinite(vals).all() and np.abs(vals[:, :, 1:]).max() > 0 and np.abs(vals[:, :, 0] - 1).max() > 0   # the flow has started
