"""Surface statistics on 2 ranks (both on the one MI355X, gloo with host staging): every rank accumulates the triangles whose nearest
fluid cell it owns, DistributedStepper.surface_stats_sums gathers them to rank 0 in triangle order. Per-triangle sums do not depend
on the partition, so they must be the single-device sums bit for bit."""
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import case, cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dist_launch import run_ranks  # noqa: E402


@pytest.mark.gpu
def test_two_rank_surface_sums_equal_single_device(gpu, tmp_path):
    import _surface_common as common
    import _surface_dist_worker as w
    levels = 2
    res = run_ranks("_surface_dist_worker.py", 2, tmp_path, levels)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    n_tri = [int(np.load(os.path.join(tmp_path, f"rank{r}.npz"))["n_tri"]) for r in range(2)]
    assert n_tri[0] > 0 and n_tri[1] > 0, f"the sphere's triangles should be owned on both sides of the cut: {n_tri}"
    got = np.load(os.path.join(tmp_path, "sums.npz"))
    assert int(got["early_n"]) == 0

    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    mesh, center, radius = common.tunnel_sphere_mesh(grids)
    assert sum(n_tri) == mesh.centers.shape[0] - 2                     # the two triangles inside the body belong to nobody
    st = case.HipStepper(grids)
    try:
        st.surface_stats_setup(mesh, common.tunnel_params(center, radius), w.START, w.INTERVAL)
        st.batch(1, w.STEPS, np.float32(w.U), params)
        sums, n = st.surface_stats_sums()
        assert int(got["n"]) == n == len(range(w.START, w.STEPS + 1, w.INTERVAL))
        assert np.array_equal(got["sums"], sums)
        assert np.abs(sums[2:5]).max() > 0
    finally:
        st.close()
