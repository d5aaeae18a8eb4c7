"""Velocity-gradient fields on 2 ranks (both on the one MI355X, gloo with host staging; RCCL needs one device per rank): every rank
computes on its owned blocks, whose face stencils reach into ghost blocks the halo exchange refreshed; DistributedStepper.gradient_fields
gathers them like field(). At an odd and an even coarse step, from both velocity buffers (on the finer level the one the flow file
takes after an even step is the output of the previous sub-step), the gathered fields must be the single-device fields, bit for bit."""
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import case, cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _dist_launch import run_ranks  # noqa: E402


@pytest.mark.gpu
def test_two_rank_fields_equal_single_device(gpu, tmp_path):
    import _gradient_dist_worker as w
    levels = 2
    res = run_ranks("_gradient_dist_worker.py", 2, tmp_path, levels)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    got = np.load(os.path.join(tmp_path, "fields.npz"))
    per_rank = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2)]
    for t in w.ODD_EVEN:
        for lvl in range(levels):
            for vel_name in ("vel", "vel_temp"):
                key = f"{t}_{lvl}_{vel_name}"
                for r, m in enumerate(per_rank):
                    assert bool(m[f"equal_{key}"]), f"rank {r} {key}: device != restatement on the local velocity"
                    assert int(m[f"readers_{key}"]) > 0 and bool(m[f"ghost_matters_{key}"]), f"rank {r} {key}: no ghost read"

    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    st = case.HipStepper(grids)
    try:
        for t in range(1, max(w.ODD_EVEN) + 1):
            st.batch(t, 1, np.float32(w.U), params)
            if t not in w.ODD_EVEN:
                continue
            for lvl in range(levels):
                scale = np.float32(1.0 / grids[lvl].dx)
                for vel_name in ("vel", "vel_temp"):
                    wv, q = st.gradient_fields(lvl, vel_name, scale)
                    key = f"{t}_{lvl}_{vel_name}"
                    assert np.abs(wv).max() > 0
                    assert np.array_equal(got[f"w_{key}"], wv), f"{key} vorticity"
                    assert np.array_equal(got[f"q_{key}"], q), f"{key} Q"
    finally:
        st.close()
