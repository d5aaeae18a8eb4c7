"""Fourier modes on 2 ranks (both on the one MI355X, gloo with host staging; RCCL needs one device per rank): every rank accumulates
its owned blocks inside DistributedStepper.batch, modes_sums gathers them like the statistics. The finest level has Bouzidi cells on
both sides of the cut. The gathered sums must be the single-device sums, bit for bit, in every column and level."""
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import case, cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dist_launch import run_ranks  # noqa: E402


@pytest.mark.gpu
def test_two_rank_sums_equal_single_device(gpu, tmp_path):
    import _modes_dist_worker as w
    levels = 2
    res = run_ranks("_modes_dist_worker.py", 2, tmp_path, levels)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    nbc = [np.load(os.path.join(tmp_path, f"rank{r}.npz"))["nbc"] for r in range(2)]
    assert nbc[0][-1] > 0 and nbc[1][-1] > 0, f"the sphere's Bouzidi cells should straddle the cut: {nbc}"
    got = np.load(os.path.join(tmp_path, "sums.npz"))

    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    st = case.HipStepper(grids)
    try:
        st.modes_setup(w.table(), w.START, w.INTERVAL)
        st.batch(1, w.STEPS, np.float32(w.U), params)
        for lvl in range(levels):
            sums, n = st.modes_sums(lvl)
            assert int(got[f"n{lvl}"]) == n == 3
            for m, a in enumerate(sums):
                assert np.array_equal(got[f"s{lvl}_{m}"], a, equal_nan=True), f"level {lvl + 1} column {m}"
            assert np.abs(sums[0][..., 1:]).max() > 0
    finally:
        st.close()
