"""Streamlines traced on the device (ludwig_streamlines_*, DeviceLevel / HipStepper.streamlines, run_case's stream_*.vtp).

The device evaluates the float32 expressions of open_ludwig_amd/streamlines.py (trace_host) in the same order with -ffp-contract=off,
so every check against the restatement is np.array_equal on counts, codes and the used records (NaN meeting NaN), not a tolerance."""
import copy
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import _streamline_cases as sc
from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, preprocess as pp, streamlines as sl

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")


def _device_levels(dev, grids, t_coarse):
    """what trace_host reads, from the device's own downloads"""
    class Fields:
        def field(self, li, name):
            return dev[li].download(name)
    return sl.stepper_levels(Fields(), grids, t_coarse)


@pytest.mark.gpu
def test_uniform_flow_and_solid_body_rotation_on_27_blocks(gpu):
    """uploaded fields, no step: the exact vertices of uniform flow, the midpoint rule's analytic drift on a linear field, forward and
    backward; the odd coarse step reads vel, the even one vel_temp"""
    g = sc.box27()
    d = adapt(g, 0)
    try:
        rho, vel = sc.uniform_fields()
        d.upload("rho", rho)
        d.upload("vel", vel)
        d.upload("vel_temp", np.zeros_like(vel))
        seeds, sign = sc.both_directions(sc.UNIFORM_SEEDS)
        d.streamlines_setup(seeds, sign, 0.5, 1e-6, 100)
        got = d.streamlines(1)
        sc.check_uniform(*got, seeds, sign)
        sc.assert_same(got, sl.trace_host(sc.one_level(g, rho, vel), seeds, sign, 0.5, 1e-6, 100))
        counts, codes, _ = d.streamlines(2)                                 # vel_temp is at rest: one vertex, then too slow
        assert (counts == 1).all() and (codes == sl.END_SLOW).all()
        rho, vel = sc.rotation_fields()
        d.upload("rho", rho)
        d.upload("vel_temp", vel)
        for step, radius, n in sc.ROTATION:
            seeds, sign = sc.both_directions(sc.rotation_seeds(radius))
            d.streamlines_setup(seeds, sign, step, 1e-6, n)
            got = d.streamlines(4)
            sc.check_rotation(*got, step, radius, n)
            sc.assert_same(got, sl.trace_host(sc.one_level(g, rho, vel), seeds, sign, step, 1e-6, n))
    finally:
        d.close()


@pytest.mark.gpu
def test_planted_obstacles_non_finite_and_slow_cells_and_seeds_that_fail(gpu):
    g, rho, vel, seeds, sign = sc.planted()
    d = adapt(g, 0)
    try:
        d.upload("rho", rho)
        d.upload("vel_temp", vel)
        lv = sc.one_level(g, rho, vel)
        for max_steps in (sc.PLANTED_MAX_STEPS, 0):
            d.streamlines_setup(seeds, sign, 0.5, sc.MIN_SPEED, max_steps)
            got = d.streamlines(0)
            sc.assert_same(got, sl.trace_host(lv, seeds, sign, 0.5, sc.MIN_SPEED, max_steps))
            if max_steps:
                assert set(got[1].tolist()) == {0, 1, 2, 3} and got[0][1:4].tolist() == [0, 0, 0] and got[1][1:4].tolist() == [1, 1, 2]
                u = sl.used(got[0], got[2])
                assert np.isnan(u).any() and np.isinf(u).any()
            else:
                assert set(got[0].tolist()) == {0, 1} and (got[1][got[0] == 1] == 0).all()
    finally:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_tunnel_levels_match_restatement_after_3_and_4_steps(gpu, levels):
    """the locator on a real hierarchy: lines that change level, midpoints on another level, the sphere, the grid's extent; right
    after a batch whose rho store may have been elided. Tracing the step before reads level 1's other velocity buffer."""
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    dev = [adapt(g, 0) for g in grids]
    seeds, sign = sc.tunnel_rake()
    s = sl.DeviceStreamlines(dev, seeds, sign, sc.TUNNEL_STEP, sc.TUNNEL_MIN_SPEED, sc.TUNNEL_MAX_STEPS)
    try:
        t_done = 0
        for t_coarse in (3, 4):
            execute_timestep_batch(dev, t_done + 1, t_coarse - t_done, F32(0.05), params)
            t_done = t_coarse
            s.trace(t_coarse)
            got = s.download()
            before = [{n: d.download(n) for n in STATES} for d in dev]
            sc.assert_same(got, sl.trace_host(_device_levels(dev, grids, t_coarse), seeds, sign, sc.TUNNEL_STEP, sc.TUNNEL_MIN_SPEED,
                                              sc.TUNNEL_MAX_STEPS))
            assert ((got[1] == sl.END_OBSTACLE) & (got[0] >= 2)).any() and ((got[1] == sl.END_OUTSIDE) & (got[0] >= 2)).any()
            if levels > 1:
                assert sl.level_changes(got[0], got[2]).max() >= 2
            s.trace(t_coarse - 1)
            other = s.download()
            a, b = sl.used(*got[::2]), sl.used(*other[::2])
            assert a.shape != b.shape or not np.array_equal(a, b, equal_nan=True)
            # a trace writes nothing but its own buffers
            for lvl, (d, b) in enumerate(zip(dev, before)):
                for n in STATES:
                    assert np.array_equal(d.download(n), b[n]), f"level {lvl + 1} {n}"
    finally:
        s.close()
        for d in dev:
            d.close()


@pytest.mark.gpu
def test_error_paths_and_the_empty_set(gpu):
    g = sc.box27()
    lib = _lib.load()
    d = adapt(g, 0)
    seeds, sign = sc.both_directions(sc.UNIFORM_SEEDS)
    arr = (C.c_void_p * 1)(d.handle)
    out = C.c_void_p()

    def create(levels=arr, n=len(sign), sd=seeds, sg=sign, step=0.5, min_speed=1e-6, max_steps=10):
        return lib.ludwig_streamlines_create(levels, 1, n, sd.ctypes.data, sg.ctypes.data, step, min_speed, max_steps, C.byref(out))
    try:
        for kw in ({"step": 0.0}, {"step": -0.5}, {"step": float("nan")}, {"step": float("inf")}, {"max_steps": -1}, {"n": -1},
                   {"sg": np.where(np.arange(len(sign)) == 2, F32(0.5), sign).astype(F32)}, {"sg": np.zeros_like(sign)},
                   {"sg": np.full_like(sign, np.nan)}):
            assert create(**kw) == -1 and out.value is None, kw                  # LUDWIG_ERR_INVALID
            assert lib.ludwig_last_error()
        assert lib.ludwig_streamlines_create(arr, 0, len(sign), seeds.ctypes.data, sign.ctypes.data, 0.5, 1e-6, 10, C.byref(out)) == -1
        assert lib.ludwig_streamlines_create(arr, 1, len(sign), None, sign.ctypes.data, 0.5, 1e-6, 10, C.byref(out)) == -1
        # n_lines = 0: a set that launches nothing and downloads nothing
        s = sl.DeviceStreamlines([d], np.zeros((0, 3), F32), np.zeros(0, F32), 0.5, 1e-6, 10)
        assert lib.ludwig_streamlines_download(s.handle, None, None, None, 0) == -5       # LUDWIG_ERR_STATE before the first trace
        s.trace(1)
        counts, codes, rec = s.download()
        assert counts.shape == codes.shape == (0,) and rec.shape == (0, 11, 8)
        s.close()
        with pytest.raises(RuntimeError, match="closed"):
            s.trace(1)
        # a wrong byte count, and a download before the first trace
        s = sl.DeviceStreamlines([d], seeds, sign, 0.5, 1e-6, 10)
        buf = np.zeros((len(sign), 11, 8), F32)
        cnt = np.zeros(len(sign), np.int32)
        assert lib.ludwig_streamlines_download(s.handle, cnt.ctypes.data, cnt.ctypes.data, buf.ctypes.data, buf.nbytes) == -5
        assert lib.ludwig_streamlines_trace(s.handle, -1) == -1
        s.trace(1)
        assert lib.ludwig_streamlines_download(s.handle, cnt.ctypes.data, cnt.ctypes.data, buf.ctypes.data, buf.nbytes - 4) == -1
        assert lib.ludwig_streamlines_download(s.handle, None, cnt.ctypes.data, buf.ctypes.data, buf.nbytes) == -1
        s.close()
        with pytest.raises(ValueError):
            sl.DeviceStreamlines([d], seeds, sign[:-1], 0.5, 1e-6, 10)
    finally:
        d.close()
    # LUDWIG_ERR_STATE: a level made without block_pointer, a level that holds ghost blocks
    bare = copy.copy(g)
    bare.block_pointer = np.zeros(0, np.int32)
    ghost = copy.copy(g)
    ghost.n_owned = g.n_blocks - 3
    for host, word in ((bare, b"block_pointer"), (ghost, b"ghost")):
        d = adapt(host, 0)
        try:
            with pytest.raises(_lib.LudwigError) as e:
                sl.DeviceStreamlines([d], seeds, sign, 0.5, 1e-6, 10)
            assert e.value.code == -5 and word in lib.ludwig_last_error()
        finally:
            d.close()


CUBE = {"basic": {"num_levels": 3, "surface_resolution": 14, "simulation": {"steps": 10, "output_freq": 8, "ramp_steps": 4}},
        "advanced": {"diagnostics": {"freq": 4}}}
STREAMS = {"enabled": True, "start_step": 2, "interval": 3, "step": 0.5, "max_steps": 60, "min_speed": 1e-7, "direction": "both",
           "seeds": [{"name": "rake", "line": {"from": [-4.0, -1.5, -0.2], "to": [-4.0, 1.5, 0.3], "count": 5}},
                     {"name": "pts", "points": [[-2.0, 0.3, 0.1], [0.0, 0.0, 0.0], [1.0e3, 0.0, 0.0], [-3.9, 0.6, -0.4]]}]}


@pytest.mark.gpu
def test_run_case_writes_lines_at_the_sampled_steps_and_leaves_the_rest_unchanged(gpu, tmp_path):
    """cube1m on two levels, 10 coarse steps, lines after steps 2, 5 and 8: the files hold what trace_host makes of the downloaded
    fields, and every other output file keeps its bytes"""
    stl = os.path.join(G, "cube1m.stl")
    runs = {}
    for on in (False, True):
        over = copy.deepcopy(CUBE)
        if on:
            over["advanced"]["streamlines"] = STREAMS
        cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), over)
        setup = pp.setup_multilevel_domain(cfg, stl)
        want = {}

        class Recording(case.HipStepper):
            def streamlines(self, t_coarse):
                got = super().streamlines(t_coarse)
                host = sl.trace_host(sl.stepper_levels(self, self.host, t_coarse), self.stream_set_seeds, self.stream_set_sign,
                                     cfg.streamlines_step, cfg.streamlines_min_speed, cfg.streamlines_max_steps)
                sc.assert_same(got, host)
                want[t_coarse] = host
                return got

            def streamlines_setup(self, seeds, sign, *args, **kwargs):
                self.stream_set_seeds, self.stream_set_sign = seeds, sign
                super().streamlines_setup(seeds, sign, *args, **kwargs)
        out = os.path.join(tmp_path, "on" if on else "off")
        lines = []
        case.run_case(cfg, Recording, setup=setup, out_dir=out, log=lines.append)
        runs[on] = (out, cfg, setup, want, lines)
    off, on = runs[False][0], runs[True][0]
    cfg, (grids, _, params, _), want, lines = runs[True][1], runs[True][2], runs[True][3], runs[True][4]
    steps = [2, 5, 8]
    new = [f"stream_{n}_{s:06d}.vtp" for n in ("rake", "pts") for s in steps] + ["stream_rake.pvd", "stream_pts.pvd"]
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + new)
    for name in os.listdir(off):
        if name != "convergence.csv":                                       # wall time and MLUPS columns
            assert filecmp.cmp(os.path.join(off, name), os.path.join(on, name), shallow=False), name
    from open_ludwig_amd.slices import read_pvd
    for n in ("rake", "pts"):
        assert read_pvd(os.path.join(on, f"stream_{n}.pvd")) == [(s * params.time_scale, f"stream_{n}_{s:06d}.vtp") for s in steps]
    assert not runs[False][3] and sorted(want) == steps
    plan = sl.SeedPlan([(s.name, np.asarray(s.points)) for s in cfg.streamlines_seeds], "both", params.mesh_offset, grids[0].dx)
    assert plan.n_lines == 18
    written = 0
    for s_step in steps:
        counts, codes, rec = want[s_step]
        for gi, name in enumerate(("rake", "pts")):
            ln = sl.group_lines(plan, gi, counts, codes, rec)
            arr = sl.read_vtp(os.path.join(on, f"stream_{name}_{s_step:06d}.vtp"))
            assert int(arr["NumberOfLines"]) == len(ln.offsets) and int(arr["NumberOfPoints"]) == len(ln.points)
            assert np.array_equal(arr["Points"], ln.points) and np.array_equal(arr["offsets"], ln.offsets)
            assert np.array_equal(arr["connectivity"], np.arange(len(ln.points)))
            assert np.array_equal(arr["Density"], ln.rho) and np.array_equal(arr["Velocity"], ln.vel) and np.array_equal(arr["Level"], ln.level)
            assert np.array_equal(arr["Seed"], ln.seed) and np.array_equal(arr["Direction"], ln.direction)
            assert np.array_equal(arr["EndCode"], ln.end_code)
            written += len(ln.offsets)
            assert sum(f"streamlines {name!r}: step {s_step}:" in l for l in lines) == 1
    assert written > 0
    # the first vertex of a line is its seed in the flow file's frame: the STL point moved by the mesh offset
    arr = sl.read_vtp(os.path.join(on, "stream_rake_000008.vtp"))
    first = arr["Points"][np.r_[0, arr["offsets"][:-1]]]
    seeds_domain = np.asarray(cfg.streamlines_seeds[0].points)[arr["Seed"]] + np.asarray(params.mesh_offset)
    assert np.abs(first - seeds_domain).max() < 1e-5
