"""Surface statistics on the device (ludwig_surface_stats_*, ludwig_execute_timestep_batch_sampled, DeviceSurfaceStats,
HipStepper.surface_stats_*, run_case's surface_mean_*.vtu / forces_mean.csv). k_accumulate_surface_stats evaluates the float32
expressions of forces.stress_from_cells with -ffp-contract=off and adds exact float64 values in sample order, so the checks against
the numpy restatement (surface_stats.HostSurfaceStats) are bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, preprocess as pp, probes as pm
from open_ludwig_amd import surface_stats as ss
from open_ludwig_amd.statistics import is_sample_step, sample_steps, t_sub_after

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _probes_common as pcommon  # noqa: E402
import _surface_common as common  # noqa: E402

F32 = np.float32
U = F32(0.05)
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")


def _tunnel(levels):
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    mesh, center, radius = common.tunnel_sphere_mesh(grids)
    return grids, params, mesh, common.tunnel_params(center, radius)


def _newest(d, fin, t):
    return d.download("rho"), d.download("vel_temp" if t_sub_after(fin, t) % 2 == 0 else "vel")


@pytest.mark.gpu
@pytest.mark.parametrize("levels,interval", [(1, 1), (3, 2)])
def test_device_sums_equal_restatement_and_leave_the_flow_alone(gpu, levels, interval):
    """in-batch sampling (batches of 8) vs HostSurfaceStats on the fields a run without a set downloads after each step; one level
    samples odd and even steps (vel and vel_temp), three levels have Bouzidi cells on the finest"""
    grids, params, mesh, sparams = _tunnel(levels)
    fin = levels - 1
    assert grids[fin].n_boundary_cells > 0
    plan = ss.plan_surface(mesh, grids[fin], sparams)
    start, n_steps = 3, 16
    ref = [adapt(g, 0) for g in grids]
    dev = [adapt(g, 0) for g in grids]
    S = ss.DeviceSurfaceStats(plan, dev[fin], fin, grids[fin].tau, sparams, start, interval)
    host = ss.HostSurfaceStats(plan, grids[fin].tau, sparams, start, interval)
    try:
        parities = set()
        for t in range(1, n_steps + 1):
            execute_timestep_batch(ref, t, 1, U, params)
            if is_sample_step(t, start, interval):
                host.accumulate(*_newest(ref[fin], fin, t))
                parities.add(t_sub_after(fin, t) % 2)
        for t0 in range(1, n_steps + 1, 8):
            execute_timestep_batch(dev, t0, 8, U, params, surface=S)
        sums, n = S.download()
        want, n_want = host.download()
        assert n == n_want == len(sample_steps(1, n_steps, start, interval))
        assert parities == ({0, 1} if levels == 1 else {1})
        assert np.array_equal(sums, want), int((sums != want).sum())
        assert np.abs(sums[2:5]).max() > 0 and (sums[1] > 0).sum() >= plan.found.sum() - 2
        # not found (on 3 levels: the part of the sphere the finest level does not cover, and the two triangles deep in the body)
        assert (~plan.found).any() == (levels == 3) and not sums[:, ~plan.found].any()
        for lvl, (a, b) in enumerate(zip(ref, dev)):
            for name in STATES:
                assert np.array_equal(a.download(name), b.download(name)), f"level {lvl + 1} {name}: the set changed the flow"
        S.reset()
        assert S.download()[1] == 0 and not S.download()[0].any()
    finally:
        S.close()
        for d in ref + dev:
            d.close()


@pytest.mark.gpu
def test_native_batch_python_recursion_and_explicit_accumulate_agree(gpu):
    grids, params, mesh, sparams = _tunnel(2)
    fin = 1
    plan = ss.plan_surface(mesh, grids[fin], sparams)
    got = []
    for mode in ("native", "python", "explicit"):
        dev = [adapt(g, 0) for g in grids]
        S = ss.DeviceSurfaceStats(plan, dev[fin], fin, grids[fin].tau, sparams, 2, 3)
        try:
            if mode == "explicit":
                for t in range(1, 11):
                    execute_timestep_batch(dev, t, 1, U, params)
                    if S.is_sample_step(t):
                        S.accumulate(t_sub_after(fin, t))
            else:
                execute_timestep_batch(dev, 1, 10, U, params, native=mode == "native", surface=S)
            got.append(S.download())
        finally:
            S.close()
            for d in dev:
                d.close()
    assert [n for _, n in got] == [3, 3, 3]
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][0], got[2][0])


@pytest.mark.gpu
def test_probe_series_unchanged_by_a_surface_set(gpu):
    """ludwig_execute_timestep_batch_probes with probes, and _sampled with the same probes plus a surface set: the same series"""
    grids, params, mesh, sparams = _tunnel(3)
    pplan = pcommon.tunnel_points(grids)
    splan = ss.plan_surface(mesh, grids[2], sparams)
    series = []
    for with_surface in (False, True):
        dev = [adapt(g, 0) for g in grids]
        P = pm.DeviceProbes(pplan, dev, 8, 1, 2)
        S = ss.DeviceSurfaceStats(splan, dev[2], 2, grids[2].tau, sparams, 1, 1) if with_surface else None
        try:
            execute_timestep_batch(dev, 1, 8, U, params, probes=P, surface=S)
            series.append(P.download())
            if S is not None:
                assert S.download()[1] == 8
        finally:
            P.close()
            if S is not None:
                S.close()
            for d in dev:
                d.close()
    assert series[0][0].tolist() == series[1][0].tolist() == [1, 3, 5, 7]
    assert np.array_equal(series[0][1].view(np.uint32), series[1][1].view(np.uint32))


@pytest.mark.gpu
def test_error_paths_fail_before_any_step_and_an_empty_set_works(gpu):
    grids, params, mesh, sparams = _tunnel(2)
    plan = ss.plan_surface(mesh, grids[1], sparams)
    lib = _lib.load()
    dev = [adapt(g, 0) for g in grids]
    other = adapt(grids[1], 0)
    S = ss.DeviceSurfaceStats(plan, other, 1, grids[1].tau, sparams)
    E = ss.DeviceSurfaceStats(plan.subset([]), dev[1], 1, grids[1].tau, sparams)
    fl = params.to_c()
    try:
        execute_timestep_batch(dev, 1, 2, U, params)
        before = [{n: d.download(n) for n in STATES} for d in dev]

        def batch(s, t0, n, start=1, interval=1):
            arr = (C.c_void_p * len(dev))(*[d.handle for d in dev])
            smp = _lib.BatchSamplers(None, 0, 1, s.handle.value, start, interval)
            return lib.ludwig_execute_timestep_batch_sampled(arr, len(dev), t0, n, float(U), C.byref(fl), C.byref(smp))
        assert batch(S, 3, 2) == -1 and "not in the batch" in lib.ludwig_last_error().decode()
        assert batch(E, 3, 2, 1, 0) == -1 and "interval" in lib.ludwig_last_error().decode()
        for lvl, d in enumerate(dev):
            for n in STATES:
                assert np.array_equal(before[lvl][n], d.download(n)), f"level {lvl + 1} {n}: stepped before failing"
        assert S.download()[1] == 0 and E.download()[1] == 0
        assert batch(E, 3, 4, 3, 2) == 0                                      # n_tri = 0: counted, nothing launched
        sums, n = E.download()
        assert n == 2 and sums.shape == (7, 0)
        h = C.c_void_p()
        sp = _lib.SurfaceParams(0.0, 0.5, 0.0, 0.0, 0.0, 1.0, 1.0, 0)
        i32 = lambda *v: np.array(v, np.int32)
        f = np.zeros(3, np.float32)
        for blocks, cells in ((i32(grids[1].n_blocks), i32(0)), (i32(-2), i32(0)), (i32(0), i32(512)), (i32(0), i32(-1))):
            assert lib.ludwig_surface_stats_create(dev[1].handle, 1, blocks.ctypes.data, cells.ctypes.data, f.ctypes.data, f.ctypes.data,
                                                   C.byref(sp), C.byref(h)) == -1 and not h.value
        assert lib.ludwig_surface_stats_accumulate(E.handle, -1) == -1
        out = np.zeros(7, np.float64)
        assert lib.ludwig_surface_stats_download(S.handle, out.ctypes.data, 8, None) == -1        # wrong size
    finally:
        S.close()
        E.close()
        for d in dev + [other]:
            d.close()


RE266K = {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}, "simulation": {"steps": 16, "output_freq": 16}},
          "advanced": {"diagnostics": {"freq": 8}}}


@pytest.mark.gpu
def test_ball1m_device_sums_equal_restatement(gpu):
    cfg = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), RE266K)
    grids, mesh, params, _ = pp.setup_multilevel_domain(cfg, os.path.join(G, "ball1m.stl"))
    sp = pp.solver_params(cfg, params)
    fin = len(grids) - 1
    st = case.HipStepper(grids)
    try:
        plan = st.surface_stats_setup(mesh, params, 1, 2)
        host = ss.HostSurfaceStats(plan, grids[fin].tau, params, 1, 2)
        for t0 in (1, 5, 9):
            st.batch(t0, 4, F32(0.03), sp)                          # sampled inside the batches at 1, 3, ..., 11
        # the restatement needs the state after each sampled step: a second stepper, one step at a time
        ref = case.HipStepper(grids)
        try:
            for t in range(1, 13):
                ref.batch(t, 1, F32(0.03), sp)
                if (t - 1) % 2 == 0:
                    host.accumulate(*_newest(ref.dev[fin], fin, t))
        finally:
            ref.close()
        sums, n = st.surface_stats_sums()
        want, n_want = host.download()
        assert n == n_want == 6 and plan.found.all()
        assert np.array_equal(sums, want), int((sums != want).sum())
    finally:
        st.close()


@pytest.mark.gpu
def test_ball1m_run_case_writes_surface_mean_files_and_nothing_else_changes(gpu, tmp_path):
    out = {}
    for on in (False, True):
        over = {**RE266K, "advanced": {**RE266K["advanced"], "surface_statistics": {"enabled": on, "start_step": 8, "interval": 8}}}
        cfg = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), over)
        setup = pp.setup_multilevel_domain(cfg, os.path.join(G, "ball1m.stl"))
        d = os.path.join(tmp_path, "on" if on else "off")
        case.run_case(cfg, case.HipStepper, setup=setup, out_dir=d)
        out[on] = (d, setup, cfg)
    off, on = out[False][0], out[True][0]
    names = sorted(os.listdir(off))
    assert sorted(os.listdir(on)) == sorted(names + ["surface_mean_000016.vtu", "forces_mean.csv"])
    for n in names:
        if n != "convergence.csv":                                     # wall time and MLUPS columns
            assert open(os.path.join(off, n), "rb").read() == open(os.path.join(on, n), "rb").read(), n
    _, (grids, mesh, params, _), cfg = out[True]
    assert cfg.async_depth == 8 and cfg.diag_freq == 8 and len(grids) == 3
    v = common.read_vtu(os.path.join(on, "surface_mean_000016.vtu"))
    assert [int(v["fields"][k][0]) for k in ("StatisticsSamples", "StatisticsFirstStep", "StatisticsLastStep")] == [2, 8, 16]
    cp, cp_rms = v["cells"]["Cp_mean"], v["cells"]["Cp_rms"]
    assert np.isfinite(cp).all() and np.isfinite(cp_rms).all() and (cp_rms >= 0).all() and (cp_rms > 0).any()
    assert v["cells"]["MappingQuality"].all()
    # forces_mean.csv against the mean of forces.csv's rows at the same steps (8 and 16). The finest level of the nested ball ends
    # every coarse step on an odd sub-step, so both read `vel`, and Cd, Cl are linear in the loads: the two differ by rounding only -
    # forces.csv prints 6 decimals (5e-7 per row), and both integrate in float32 (pairwise sums over the triangles: at most
    # 2 log2(n_tri) eps32 of the sum of the magnitudes of the terms, taken here from the mean loads, plus the float32 cast of the means)
    rows = [l.strip().split(",") for l in open(os.path.join(on, "forces.csv"))][1:]
    head = open(os.path.join(on, "forces.csv")).readline().strip().split(",")
    by_step = {int(r[0]): r for r in rows}
    mean = [l.strip().split(",") for l in open(os.path.join(on, "forces_mean.csv"))]
    assert len(mean) == 2 and mean[1][:4] == ["16", "2", "8", "16"]
    q_ref = 0.5 * params.rho_physical * params.u_physical ** 2 * params.reference_area
    p_mean = v["cells"]["Pressure_Pa_mean"].astype(np.float64)
    t_mean = np.stack([v["cells"][k].astype(np.float64) for k in ("ShearX_Pa_mean", "ShearY_Pa_mean", "ShearZ_Pa_mean")], axis=1)
    A = mesh.areas
    eps = float(np.finfo(np.float32).eps)
    n_tri = mesh.centers.shape[0]
    for col, axis in (("Cd", 0), ("Cl", 2)):
        mag = (np.abs(p_mean * mesh.normals[:, axis] * A).sum() + np.abs(t_mean[:, axis] * A).sum()) / q_ref
        tol = 2 * 5e-7 + (2 * np.log2(n_tri) + 4) * eps * mag
        want = 0.5 * (float(by_step[8][head.index(col)]) + float(by_step[16][head.index(col)]))
        got = float(mean[1][ss.FORCES_MEAN_CSV_HEADER.split(",").index(col)])
        assert abs(got - want) <= tol, (col, got, want, tol)
