"""The flow monitor on 2 ranks (both on the one MI355X, gloo with host staging; RCCL needs one device per rank): every rank reduces its
owned blocks on its device, DistributedStepper.monitor gathers and merges the small records. Counts, extremes and cells must be the
single-device record exactly - the initial rho = 1 field keeps ties alive, so the tie rule matters. The two Float64 sums may differ,
because the ranks' trees are added in rank order: a pairwise sum of n <= 2^31 non-negative terms errs by at most log2(n) 2^-53 ~ 3.4e-15
relative, two orders differ by at most twice that - 1e-13 allows it with room; every counted rho is asserted > 0, the bound's premise."""
import os
import pickle
import sys

import numpy as np
import pytest

from open_ludwig_amd import case, cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dist_launch import run_ranks  # noqa: E402

SUM_RTOL = 1e-13


@pytest.mark.gpu
def test_two_rank_records_equal_single_device(gpu, tmp_path):
    import _monitor_dist_worker as w
    res = run_ranks("_monitor_dist_worker.py", 2, tmp_path)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    ranks = [pickle.load(open(os.path.join(tmp_path, f"rank{r}.pkl"), "rb")) for r in range(2)]
    for lvl in range(w.LEVELS):
        assert ranks[0]["owned"][lvl] > 0 and ranks[1]["owned"][lvl] > 0, "both ranks should own blocks of every level"
    assert ranks[0]["records"] == ranks[1]["records"]                   # every rank received the merged record

    grids, params = cases.tunnel_with_sphere(levels=w.LEVELS, wall_model=True)
    st = case.HipStepper(grids)
    try:
        for t in range(1, w.SAMPLED[-1] + 1):
            st.batch(t, 1, np.float32(w.U), params)
            if t not in w.SAMPLED:
                continue
            for lvl, g in enumerate(grids):
                one, two = st.monitor(lvl, t), ranks[0]["records"][(t, lvl)]
                assert two.same_but_sums(one), f"step {t} level {lvl + 1}\n{one}\n{two}"
                assert (st.field(lvl, "rho")[~g.obstacle] > 0).all() and one.n_bad == 0
                for name in ("sum_rho", "sum_rho_v2"):
                    a, b = float(getattr(one, name)), float(getattr(two, name))
                    print(f"step {t} level {lvl + 1} {name}: one device {a!r}, two ranks {b!r}, relative difference {abs(a - b) / abs(a):.3e}")
                    assert abs(a - b) <= SUM_RTOL * abs(a), (t, lvl, name, a, b)
    finally:
        st.close()
