"""Probes on the device (ludwig_probes_*, ludwig_execute_timestep_batch_probes, DeviceProbes, HipStepper.probes_*, run_case's
probes.csv). The kernel evaluates probes.trilinear's float32 expressions in the same order with -ffp-contract=off, so the checks
against the restatement are bit for bit."""
import os

import numpy as np
import pytest

import _probes_common as common
from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, preprocess as pp, probes as pm
from open_ludwig_amd.statistics import t_sub_after

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
U = F32(0.05)
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")


def _newest(d, li, t):
    return d.download("rho"), d.download("vel_temp" if t_sub_after(li, t) % 2 == 0 else "vel")


def _bits(a):
    return np.asarray(a, dtype=F32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("interval", [1, 3])
def test_device_series_equals_restatement_and_leaves_the_flow_alone(gpu, levels, interval):
    """batches of 8 sampled inside the C batch vs the numpy interpolation of the fields an unprobed run downloads after each step"""
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    plan = common.tunnel_points(grids)
    assert set(plan.level.tolist()) == set(range(levels)) and plan.replaced.any()
    start, n_steps = 2, 16
    ref = [adapt(g, 0) for g in grids]
    dev = [adapt(g, 0) for g in grids]
    P = pm.DeviceProbes(plan, dev, 8, start, interval)
    try:
        want_steps, want = [], []
        for t in range(1, n_steps + 1):
            execute_timestep_batch(ref, t, 1, U, params)
            if pm.is_sample_step(t, start, interval):
                want_steps.append(t)
                want.append(pm.sample_fields(plan, lambda li: _newest(ref[li], li, t)))
        got_steps, got = [], []
        for t0 in range(1, n_steps + 1, 8):
            execute_timestep_batch(dev, t0, 8, U, params, probes=P)
            s, v = P.download()
            got_steps += s.tolist()
            got.append(v)
        got = np.concatenate(got)
        assert got_steps == want_steps and {t % 2 for t in got_steps} == {0, 1}
        assert got.shape == (len(want_steps), plan.n, 4) and np.isfinite(got).all()
        assert np.array_equal(_bits(got), _bits(np.stack(want)))
        assert np.abs(got[:, :, 1]).max() > 1e-3
        for lvl, (a, b) in enumerate(zip(ref, dev)):
            for n in STATES:
                assert np.array_equal(a.download(n), b.download(n)), f"level {lvl + 1} {n}: probes changed the flow"
        s, v = P.download()
        assert s.size == 0 and v.shape == (0, plan.n, 4)
    finally:
        P.close()
        for d in ref + dev:
            d.close()


@pytest.mark.gpu
def test_python_recursion_gives_the_native_bits(gpu):
    grids, params = cases.tunnel_with_sphere(levels=3, wall_model=True)
    plan = common.tunnel_points(grids)
    series = []
    for native in (True, False):
        dev = [adapt(g, 0) for g in grids]
        P = pm.DeviceProbes(plan, dev, 8, 1, 2)
        execute_timestep_batch(dev, 1, 8, U, params, native=native, probes=P)
        series.append(P.download())
        P.close()
        for d in dev:
            d.close()
    assert np.array_equal(series[0][0], [1, 3, 5, 7]) and np.array_equal(series[0][0], series[1][0])
    assert np.array_equal(_bits(series[0][1]), _bits(series[1][1]))


@pytest.mark.gpu
def test_standalone_sample_of_a_linear_field_is_analytic(gpu):
    """an uploaded linear field, sampled with ludwig_probes_sample: the analytic value to float32 rounding (no restatement involved)"""
    grids, _ = cases.tunnel_with_sphere(levels=3, wall_model=True)
    plan = common.tunnel_points(grids)
    a = np.array([1.0, 0.01, -0.02, 0.005])
    b = np.array([[0.001, -0.0005, 0.0002], [0.002, 0.001, 0.0], [-0.001, 0.0015, 0.0007], [0.0, 0.0003, -0.002]])
    dev = [adapt(g, 0) for g in grids]
    P = pm.DeviceProbes(plan, dev, 2)
    try:
        for li, (d, g) in enumerate(zip(dev, grids)):
            c = [(x - 0.5) * g.dx for x in cases.global_cell_coords(g)]
            lin = [(a[k] + b[k, 0] * c[0] + b[k, 1] * c[1] + b[k, 2] * c[2]).astype(F32) for k in range(4)]
            d.upload("rho", np.asfortranarray(lin[0]))
            d.upload("vel", np.asfortranarray(np.stack(lin[1:], axis=-1)))
        for li in range(3):
            P.sample(li, t_sub_after(li, 1))                 # odd sub-steps: the `vel` buffer; one slot, coarse step 1
        steps, vals = P.download()
        assert steps.tolist() == [1] and vals.shape == (1, plan.n, 4)
        exact = a[None, :] + plan.domain @ b.T
        interior = ~plan.replaced.any(axis=1)
        assert interior.sum() >= 5
        err = np.abs(vals[0][interior] - exact[interior]) / np.abs(exact[interior]).clip(1e-3)
        assert err.max() < 2e-6, err.max()
        assert np.isfinite(vals).all()
    finally:
        P.close()
        for d in dev:
            d.close()


@pytest.mark.gpu
def test_overflow_and_mismatched_levels_fail_before_any_step(gpu):
    grids, params = cases.tunnel_with_sphere(levels=2, wall_model=True)
    plan = common.tunnel_points(grids)
    lib = _lib.load()
    dev = [adapt(g, 0) for g in grids]
    other = [adapt(g, 0) for g in grids]
    P = pm.DeviceProbes(plan, dev, 2, 1, 1)
    import ctypes as C
    fl = params.to_c()
    try:
        execute_timestep_batch(dev, 1, 2, U, params)
        before = [{n: d.download(n) for n in STATES} for d in dev]

        def batch(levels, t0, n, start=1, interval=1):
            arr = (C.c_void_p * len(levels))(*[d.handle for d in levels])
            return lib.ludwig_execute_timestep_batch_probes(arr, len(levels), t0, n, float(U), C.byref(fl), P.handle, start, interval)
        assert batch(dev, 3, 3) == -5                                  # 3 samples, room for 2
        assert batch(dev, 3, 8, 3, 3) == -5                            # steps 3, 6, 9 > 2
        assert batch(other, 3, 1) == -1                                # another level array
        assert batch(dev[:1], 3, 1) == -1                              # fewer levels
        assert batch(dev, 3, 1, 1, 0) == -1                            # interval < 1
        for lvl, d in enumerate(dev):
            for n in STATES:
                assert np.array_equal(before[lvl][n], d.download(n)), f"level {lvl + 1} {n}: stepped before failing"
        s, _ = P.download()
        assert s.size == 0
        assert batch(dev, 3, 2) == 0                                   # exactly the free ring
        assert batch(dev, 5, 1) == -5
        s, v = P.download()
        assert s.tolist() == [3, 4] and np.isfinite(v).all()
        assert lib.ludwig_probes_sample(P.handle, 2, 0) == -1 and lib.ludwig_probes_sample(P.handle, 0, -1) == -1
        P.sample(0, 5)
        P.sample(0, 6)
        assert lib.ludwig_probes_sample(P.handle, 0, 7) == -5           # ring full
        n = C.c_int32(0)
        vals = np.zeros((1, plan.n, 4), np.float32)
        steps = np.zeros(1, np.int64)
        assert lib.ludwig_probes_download(P.handle, vals.ctypes.data, steps.ctypes.data, 1, C.byref(n)) == -1   # 2 waiting
        s, v = P.download()
        assert s.tolist() == [5, 6]
        lvl1 = plan.level == 1
        assert np.isnan(v[:, lvl1]).all() and np.isfinite(v[:, ~lvl1]).all()    # level 2 was not sampled in those slots
    finally:
        P.close()
        for d in dev + other:
            d.close()


@pytest.mark.gpu
def test_hip_stepper_drains_every_batch_and_cuts_a_long_one(gpu):
    grids, params = cases.tunnel_with_sphere(levels=2, wall_model=True)
    plan = common.tunnel_points(grids)
    st = case.HipStepper(grids)
    ref = case.HipStepper(grids)
    try:
        st.probes_setup(plan, 1, 1, capacity=4)
        st.batch(1, 10, U, params)                       # 10 samples through a ring of 4: cut at 4, 8
        ref.batch(1, 10, U, params)
        steps, vals = st.probes_series()
        assert steps.tolist() == list(range(1, 11)) and st.probes.capacity == 4
        want = pm.sample_fields(plan, lambda li: _newest(ref.dev[li], li, 10))
        assert np.array_equal(_bits(vals[-1]), _bits(want))
        for lvl in range(2):
            for n in STATES:
                assert np.array_equal(st.field(lvl, n), ref.field(lvl, n))
    finally:
        st.close()
        ref.close()


RE266K = {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}, "simulation": {"steps": 16, "output_freq": 16}},
          "advanced": {"diagnostics": {"freq": 8}}}


@pytest.mark.gpu
def test_ball1m_run_case_writes_probe_files_and_nothing_else_changes(gpu, tmp_path):
    pts = [[0.8, 0.02, -0.03], [1.5, 0.2, 0.1], [-0.56, 0.013, 0.011], [-3.5, 0.0, 0.0], [2.6, 0.4, -0.3]]
    out = {}
    for on in (False, True):
        over = {**RE266K, "advanced": {**RE266K["advanced"], "probes": {"enabled": on, "interval": 1, "points": pts}}}
        cfg = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), over)
        d = os.path.join(tmp_path, "on" if on else "off")
        case.run_case(cfg, case.HipStepper, setup=pp.setup_multilevel_domain(cfg, os.path.join(G, "ball1m.stl")), out_dir=d)
        out[on] = d
    names = sorted(os.listdir(out[False]))
    assert sorted(os.listdir(out[True])) == sorted(names + ["probes.csv", "probes_points.csv"])
    for n in names:
        if n != "convergence.csv":                                     # wall time and MLUPS columns
            assert open(os.path.join(out[False], n), "rb").read() == open(os.path.join(out[True], n), "rb").read(), n
    head, steps, vals = pm.read_series_csv(os.path.join(out[True], "probes.csv"))
    assert head[2:6] == ["p0_rho", "p0_ux", "p0_uy", "p0_uz"] and steps.tolist() == list(range(1, 17))
    assert np.isfinite(vals).all() and np.abs(vals[:, :, 0] - 1).max() < 0.05
    levels = [l.strip().split(",")[-1] for l in open(os.path.join(out[True], "probes_points.csv")).readlines()[1:]]
    assert levels == ["3", "3", "3", "1", "2"]
