"""Force series on 2 ranks (both on the one MI355X, gloo with host staging): every rank reduces the triangles whose cell it owns, in
global triangle order, and rank 0 adds the ranks' records in rank order. The steps and the coverage count equal one device's exactly;
the sums come from other trees than one device's single tree, so they agree to Float64 rounding: each tree is within
ceil(log2 n) 2^-53 sum|x_i| of the exact sum to first order and the ranks' records take world - 1 more additions."""
import math
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import case, forces, partition, surface_stats as ss

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dist_launch import run_ranks  # noqa: E402

WORLD = 2


def test_two_rank_cut_runs_across_the_sphere():
    """CPU check of the layout the GPU test relies on: both ranks own triangles of the body"""
    import _force_series_dist_worker as w
    grids, params, mesh, sparams, _ = w.setup()
    owners = partition.level_owners(grids, WORLD)
    plan = ss.plan_surface(mesh, grids[-1], sparams)
    tri_owner = np.asarray(owners[-1])[plan.blocks[plan.found]]
    assert (tri_owner == 0).sum() > 50 and (tri_owner == 1).sum() > 50
    assert len(w.SAMPLED) > 2                                        # more records than the worker's ring holds


@pytest.mark.gpu
def test_two_rank_series_agrees_with_single_device(gpu, tmp_path):
    import _force_series_dist_worker as w
    res = run_ranks("_force_series_dist_worker.py", WORLD, tmp_path)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    got = np.load(os.path.join(tmp_path, "series.npz"))
    mine = [int(np.load(os.path.join(tmp_path, f"rank{r}.npz"))["n_tri"]) for r in range(WORLD)]
    assert all(m > 0 for m in mine)

    grids, params, mesh, sparams, u = w.setup()
    fin = len(grids) - 1
    st = case.HipStepper(grids)
    try:
        plan = st.force_series_setup(mesh, sparams, w.FIRST, w.INTERVAL)
        assert sum(mine) == int(plan.found.sum())
        mag = {}
        for t in range(1, w.LAST + 1):
            st.batch(t, 1, u, params)
            if t in w.SAMPLED:                                       # the nested finest level ends on an odd sub-step: `vel`
                p, tx, ty, tz, _ = ss.sample_values(plan, st.field(fin, "rho"), st.field(fin, "vel"), grids[fin].tau, sparams)
                mag[t] = np.abs(forces.force_series_contributions(mesh, p, tx, ty, tz, sparams)[0].astype(np.float64)).sum(axis=0)
        steps, sums, cov = st.force_series()
    finally:
        st.close()
    assert steps.tolist() == got["steps"].tolist() == list(w.SAMPLED)
    assert np.array_equal(cov, got["covered"]) and (cov > plan.n // 2).all() and (cov <= int(plan.found.sum())).all()
    n = plan.n
    worst = 0.0
    for i, t in enumerate(w.SAMPLED):
        bound = (math.ceil(math.log2(n)) + WORLD) * 2.0 ** -53 * mag[t]
        diff = np.abs(got["sums"][i] - sums[i])
        rel = diff / np.abs(sums[i])
        print(f"step {t}: max |diff| / bound {float((diff / bound).max()):.3f}, max relative difference {float(rel.max()):.3e}")
        worst = max(worst, float(rel.max()))
        assert (mag[t] > 0).all() and (np.abs(sums[i]) > 0).all()
        assert (diff <= bound).all(), (t, diff, bound)
    print(f"largest relative difference {worst:.3e}")
