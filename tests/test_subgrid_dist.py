"""The subgrid observer on 2 ranks (both on the one MI355X, gloo with host staging; RCCL needs one device per rank): two nested levels,
the cut crossing both, every rank working on its owned blocks, whose face stencils reach into ghost blocks the halo exchange refreshed.
The fields - from both velocity buffers, after an odd and after an even coarse step - and all three sums, gathered on rank 0, must be
one device's, bit for bit."""
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import case, cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dist_launch import run_ranks  # noqa: E402


@pytest.mark.gpu
def test_two_rank_fields_and_sums_equal_single_device(gpu, tmp_path):
    import _subgrid_dist_worker as w
    levels = 2
    res = run_ranks("_subgrid_dist_worker.py", 2, tmp_path, levels)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    got = np.load(os.path.join(tmp_path, "subgrid.npz"))
    per_rank = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2)]
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    for lvl in range(levels):                                  # the cut crosses both levels, and owned blocks read ghosts on both
        owned = [int(m[f"owned_{lvl}"]) for m in per_rank]
        assert all(n > 0 for n in owned) and sum(owned) == grids[lvl].n_blocks
        assert all(int(m[f"readers_{lvl}"]) > 0 for m in per_rank)
    st = case.HipStepper(grids)
    try:
        for t in range(1, max(w.ODD_EVEN) + 1):
            st.batch(t, 1, np.float32(w.U), params)
            if t == 1:
                st.subgrid_stats_reset()
            if t not in w.ODD_EVEN:
                continue
            st.subgrid_stats_sample(t)
            for lvl in range(levels):
                for vel_name in ("vel", "vel_temp"):
                    nu, code = st.subgrid_fields(lvl, vel_name)
                    key = f"{t}_{lvl}_{vel_name}"
                    # from rest the inlet's wave has not reached the finer level yet: there nu_t is the floor and the comparison that
                    # bites is S_eps, whose strain rates (the sponge's pull) differ from cell to cell
                    assert lvl > 0 or (code == 3).any()
                    assert np.array_equal(got[f"nu_{key}"].view(np.uint32), nu.view(np.uint32)), f"{key} nu_t"
                    assert np.array_equal(got[f"code_{key}"], code), f"{key} code"
        for lvl in range(levels):
            sums = st.subgrid_stats_sums(lvl)
            assert sums[3] == 2 == int(got[f"n_{lvl}"])
            for name, a in zip(("s_nu", "s_nunu", "s_eps"), sums[:3]):
                assert a.max() > 0
                assert np.array_equal(got[f"{name}_{lvl}"].view(np.uint64), a.view(np.uint64)), f"level {lvl + 1} {name}"
    finally:
        st.close()
