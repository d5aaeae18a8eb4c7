"""Time-averaged statistics on 2 ranks (both on the one MI355X, gloo with host staging; RCCL needs one device per rank): every rank
accumulates its owned blocks, DistributedStepper.stats_sums gathers them like field(). The finest level has Bouzidi cells on both
sides of the cut. The gathered sums must be the single-device sums, bit for bit."""
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import case, cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dist_launch import run_ranks  # noqa: E402


@pytest.mark.gpu
def test_two_rank_sums_equal_single_device(gpu, tmp_path):
    import _stats_dist_worker as w
    levels = 2
    res = run_ranks("_stats_dist_worker.py", 2, tmp_path, levels)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    nbc = [np.load(os.path.join(tmp_path, f"rank{r}.npz"))["nbc"] for r in range(2)]
    assert nbc[0][-1] > 0 and nbc[1][-1] > 0, f"the sphere's Bouzidi cells should straddle the cut: {nbc}"
    got = np.load(os.path.join(tmp_path, "sums.npz"))

    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    st = case.HipStepper(grids)
    try:
        for t in range(1, w.STEPS + 1):
            st.batch(t, 1, np.float32(w.U), params)
            if t == w.SAMPLES[0]:
                st.stats_reset()
            if t in w.SAMPLES:
                st.stats_sample(t)
        for lvl in range(levels):
            r, u, uu, n = st.stats_sums(lvl)
            assert int(got[f"n{lvl}"]) == n == len(w.SAMPLES)
            for name, a in (("rho", r), ("vel", u), ("vel2", uu)):
                assert np.array_equal(got[f"{name}{lvl}"], a), f"level {lvl + 1} {name}"
    finally:
        st.close()
