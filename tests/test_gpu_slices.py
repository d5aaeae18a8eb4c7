"""Slices on the device (ludwig_slices_*, DeviceSlices, HipStepper.slices_*, run_case's slice files). k_slice_sample evaluates the
probes' float32 trilinear and the gradient fields' float32 expressions in the same order with -ffp-contract=off, so every check
against the restatement (slices.sample_slice over tests/_gradient_ref.py) is bit for bit."""
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import case, cases, preprocess as pp, probes as pm, slices as sl
from open_ludwig_amd.statistics import t_sub_after

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
U = F32(0.05)
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")


def _bits(a):
    return np.asarray(a, dtype=F32).view(np.uint32)


def _planes(grids):
    """an xy plane through the sphere and an xz plane off-centre, both crossing every level"""
    return [sl.plan_slice(pp.SlicePlane("z", 2, 16.05, ((0.2, 47.8), (0.3, 31.7)), 0.173, pp.SLICE_FIELDS), grids),
            sl.plan_slice(pp.SlicePlane("y", 1, 13.37, ((1.0, 40.0), (2.0, 30.0)), 0.29, ("density", "q_criterion")), grids)]


def _restated(st, plans, grids, t):
    from _gradient_ref import gradient_fields

    def fields(li):
        vel_name = "vel_temp" if t_sub_after(li, t) % 2 == 0 else "vel"
        g = grids[li]
        vel = st.field(li, vel_name)
        w, q = gradient_fields(vel, g.neighbor_table, g.obstacle, F32(1.0 / g.dx))
        return st.field(li, "rho"), vel, w, q
    return [sl.sample_slice(p, fields, gradient=True) for p in plans]


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_device_slices_equal_restatement_at_even_and_odd_steps(gpu, levels):
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    plans = _planes(grids)
    assert set(plans[0].level[plans[0].valid].tolist()) == set(range(levels))
    st = case.HipStepper(grids)
    try:
        st.slices_setup(plans, 1, 1)
        for t in range(1, 7):
            st.batch(t, 1, U, params)
            if t in (5, 6):                                           # odd and even final sub-step of level 1
                got = st.slices_sample(t)
                want = _restated(st, plans, grids, t)
                for p, a, b in zip(plans, got, want):
                    assert a.shape == (9, p.n) and np.isfinite(a).all()
                    assert np.array_equal(_bits(a), _bits(b)), f"step {t}: rows {np.unique(np.nonzero(_bits(a) != _bits(b))[0])}"
                    assert not a[:, ~p.valid].any() and np.abs(a[1, p.valid]).max() > 1e-3 and np.abs(a[8, p.valid]).max() > 0
    finally:
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 3])
def test_device_slices_without_gradient_fields_equal_restatement(gpu, levels):
    """the default fields: k_slice_sample<false> and a 5-row result"""
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    plans = [sl.plan_slice(pp.SlicePlane("b", 2, 16.05, ((0.2, 47.8), (0.3, 31.7)), 0.173), grids),
             sl.plan_slice(pp.SlicePlane("c", 0, 27.3, None, 0.41, ("velocity",)), grids)]
    assert not any(p.gradient for p in plans)
    st = case.HipStepper(grids)
    try:
        st.slices_setup(plans, 5, 1)
        st.batch(1, 4, U, params)
        for t in (5, 6):
            st.batch(t, 1, U, params)
            got = st.slices_sample(t)

            def fields(li):
                return st.field(li, "rho"), st.field(li, "vel_temp" if t_sub_after(li, t) % 2 == 0 else "vel"), None, None
            for p, a in zip(plans, got):
                b = sl.sample_slice(p, fields)
                assert a.shape == b.shape == (5, p.n)
                assert np.array_equal(_bits(a), _bits(b)) and np.abs(a[4, p.valid]).max() > 0
        with pytest.raises(ValueError, match="no sampled step"):
            st.slices_sample(4)
    finally:
        st.close()


@pytest.mark.gpu
def test_slice_points_equal_probes_at_the_same_coordinates(gpu):
    grids, params = cases.tunnel_with_sphere(levels=3, wall_model=True)
    plan = _planes(grids)[0]
    idx = np.flatnonzero(plan.valid & plan.replaced.any(axis=1))[:20].tolist() + np.flatnonzero(plan.valid)[::97].tolist()
    pplan = pm.plan_probes(plan.points[idx], grids)
    st = case.HipStepper(grids)
    try:
        st.probes_setup(pplan, 4, 1, 8)
        st.slices_setup([plan], 4, 1)
        st.batch(1, 4, U, params)
        got = st.slices_sample(4)[0]
        steps, vals = st.probes_series()
        assert steps.tolist() == [4]
        assert np.array_equal(_bits(got[0:4, idx].T), _bits(vals[0]))
    finally:
        st.close()


@pytest.mark.gpu
def test_sampling_leaves_every_state_array_alone(gpu):
    grids, params = cases.tunnel_with_sphere(levels=3, wall_model=True)
    a, b = case.HipStepper(grids), case.HipStepper(grids)
    try:
        b.slices_setup(_planes(grids), 1, 1)
        for t in range(1, 6):
            a.batch(t, 1, U, params)
            b.batch(t, 1, U, params)
            b.slices_sample(t)
        for li in range(len(grids)):
            for n in STATES:
                assert np.array_equal(a.field(li, n), b.field(li, n)), f"level {li + 1} {n}: slices changed the flow"
    finally:
        a.close()
        b.close()


RE266K = {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}, "simulation": {"steps": 12, "output_freq": 12}},
          "advanced": {"diagnostics": {"freq": 6}}}


@pytest.mark.gpu
def test_ball1m_run_case_files_equal_the_device_download(gpu, tmp_path):
    planes = [{"name": "wake", "normal": "y", "position": 0.01, "bounds": [[-0.8, 2.5], [-0.6, 0.6]], "spacing": 0.01,
               "fields": list(pp.SLICE_FIELDS)}]
    seen = {}

    class Recording(case.HipStepper):
        def slices_sample(self, t):
            seen[t] = super().slices_sample(t)
            return seen[t]
    out = {}
    for on in (False, True):
        over = {**RE266K, "advanced": {**RE266K["advanced"], "slices": {"enabled": on, "start_step": 3, "interval": 4, "planes": planes}}}
        cfg = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), over)
        d = os.path.join(tmp_path, "on" if on else "off")
        case.run_case(cfg, Recording, setup=pp.setup_multilevel_domain(cfg, os.path.join(G, "ball1m.stl")), out_dir=d)
        out[on] = d
    names = sorted(os.listdir(out[False]))
    new = ["slice_wake_000003.vti", "slice_wake_000007.vti", "slice_wake_000011.vti", "slice_wake.pvd"]
    assert sorted(os.listdir(out[True])) == sorted(names + new) and sorted(seen) == [3, 7, 11]
    for n in names:
        if n != "convergence.csv":                                     # wall time and MLUPS columns
            assert open(os.path.join(out[False], n), "rb").read() == open(os.path.join(out[True], n), "rb").read(), n
    for t, (v,) in seen.items():                                       # one plane
        _, arr = sl.read_vti(os.path.join(out[True], "slice_wake_%06d.vti" % t))
        assert np.array_equal(_bits(arr["Density"]), _bits(v[0])) and np.array_equal(_bits(arr["Velocity"]), _bits(v[1:4].T))
        assert np.array_equal(_bits(arr["VelocityMagnitude"]), _bits(v[4]))
        assert np.array_equal(_bits(arr["Vorticity"]), _bits(v[5:8].T)) and np.array_equal(_bits(arr["QCriterion"]), _bits(v[8]))
        valid = arr["Valid"].astype(bool)
        assert valid.any() and not valid.all() and np.abs(arr["Density"][valid] - 1).max() < 0.05
