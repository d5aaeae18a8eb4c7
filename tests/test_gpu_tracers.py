"""Tracers advected on the device (ludwig_tracers_*, ludwig_execute_timestep_batch_tracers, HipStepper.tracers_*, run_case's
tracers_*.vtp).

The device evaluates the float32 expressions of open_ludwig_amd/tracers.py (advance_host, snapshot_host) in the same order with
-ffp-contract=off, so every check against the restatement is np.array_equal on the snapshot records (NaN meeting NaN), not a tolerance.
A record carries the slot's position and its code, so equal records are equal positions and states."""
import copy
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import _streamline_cases as sc
import _tracer_cases as tc
from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, preprocess as pp, tracers as tr

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")


class _Fields:
    """what stepper_levels reads, from the device's own downloads"""

    def __init__(self, dev):
        self.dev = dev

    def field(self, li, name):
        return self.dev[li].download(name)


def _snapshot(s, t):
    s.snapshot(t)
    return s.download()


def _run_against_host(d, g, vel, seeds, generations, every, dt, advances, check_every=1):
    """advance a set over the one uploaded level `advances` times (coarse step 1: it reads vel) and compare with the restatement after
    every check_every-th advance; returns the host's (P, state) history at the checked advances"""
    lv = tc.velocity_level(g, vel)
    s = tr.DeviceTracers([d], seeds, generations, every, 1, 1, dt)
    H = tr.HostTracers(seeds, generations, every, dt)
    history = []
    try:
        for k in range(advances):
            s.advance(1)
            H.advance(lv)
            if (k + 1) % check_every == 0 or k == advances - 1:
                rec, n = _snapshot(s, 1)
                assert n == k + 1
                tc.assert_same_records(rec, H.snapshot(lv))
                history.append((H.P.copy(), H.state.copy()))
    finally:
        s.close()
    return history


@pytest.mark.gpu
def test_uniform_flow_rotation_and_the_release_ring_on_27_blocks(gpu):
    """uploaded fields, no step: the exact drift of uniform flow and where it ends, one full turn of solid-body rotation at dt = 4, the
    ring of 3 generations; the odd coarse step reads vel, the even one vel_temp"""
    g = sc.box27()
    d = adapt(g, 0)
    try:
        _, vel = sc.uniform_fields()
        d.upload("vel", vel)
        d.upload("vel_temp", np.zeros_like(vel))
        tc.check_uniform(_run_against_host(d, g, vel, tc.UNIFORM_SEEDS, 1, 1000, 1.0, tc.UNIFORM_ADVANCES))
        s = tr.DeviceTracers([d], tc.UNIFORM_SEEDS, 1, 1, 1, 1)
        s.advance(1)
        odd, even = _snapshot(s, 1)[0], _snapshot(s, 2)[0]                  # vel_temp is at rest
        assert (odd[:, 3] != 0).all() and (even[:, 3:6] == 0).all() and np.array_equal(odd[:, 0:3], even[:, 0:3])
        s.close()
        hist = _run_against_host(d, g, vel, tc.RING_SEEDS, tc.RING_G, tc.RING_EVERY, tc.RING_DT, tc.RING_ADVANCES)
        assert (hist[5][1].reshape(tc.RING_G, -1)[0] != 0).sum() >= 2 and (hist[6][1].reshape(tc.RING_G, -1)[0] == 0).all()
        _, vel = sc.rotation_fields()
        d.upload("vel", vel)
        seeds, n = tc.rotation_seeds(), tc.ROTATION_ADVANCES[4]
        hist = _run_against_host(d, g, vel, seeds, 1, 10 ** 6, 4.0, n + 1, check_every=16)
        drift = np.abs(tc.radii(hist[-1][0]) - tc.radii(seeds))
        print(f"rotation dt 4 n {n}: drift {drift.tolist()}")
        assert (hist[-1][1] == 0).all() and (drift <= tc.ROTATION_DRIFT).all()
    finally:
        d.close()


@pytest.mark.gpu
def test_planted_obstacles_non_finite_velocities_and_seeds_that_fail(gpu):
    g, vel, seeds = tc.planted()
    d = adapt(g, 0)
    try:
        d.upload("vel", vel)
        hist = _run_against_host(d, g, vel, seeds, 1, 10 ** 6, tc.PLANTED_DT, tc.PLANTED_ADVANCES)
        state = hist[-1][1]
        assert set(state.tolist()) == {0, 1, 2, 3} and {i: int(state[i]) for i in tc.PLANTED_ENDS} == tc.PLANTED_ENDS
    finally:
        d.close()


def _tunnel(levels):
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    return grids, params, [adapt(g, 0) for g in grids]


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_tunnel_in_batch_equals_out_of_batch_equals_host(gpu, levels):
    """stepper A: one batch of 6 coarse steps advancing the set inside it (interval 1; on a fresh copy start_step 2, interval 2).
    Stepper B: the same steps as six batches of one without a set, ludwig_tracers_advance between them and advance_host on its
    downloaded velocity. All three agree bit for bit, and A's state arrays are B's: a tracer writes nothing but its own buffers."""
    seeds = tc.tunnel_seeds()
    u = F32(0.05)
    grids, params, dev_b = _tunnel(levels)
    sets_b = [tr.DeviceTracers(dev_b, seeds, tc.TUNNEL_G, tc.TUNNEL_EVERY, st, iv) for st, iv in tc.TUNNEL_SCHEDULES]
    hosts = [tr.HostTracers(seeds, tc.TUNNEL_G, tc.TUNNEL_EVERY, iv) for _, iv in tc.TUNNEL_SCHEDULES]
    try:
        for t in range(1, tc.TUNNEL_STEPS + 1):
            execute_timestep_batch(dev_b, t, 1, u, params)
            lv = None
            for s, H in zip(sets_b, hosts):
                if s.is_advance_step(t):
                    lv = lv if lv is not None else tr.stepper_levels(_Fields(dev_b), grids, t)
                    s.advance(t)
                    H.advance(lv)
        lv = tr.stepper_levels(_Fields(dev_b), grids, tc.TUNNEL_STEPS)
        want = [H.snapshot(lv) for H in hosts]
        for s, H, w in zip(sets_b, hosts, want):
            rec, n = _snapshot(s, tc.TUNNEL_STEPS)
            assert n == H.n_advances == tr.advances_through(tc.TUNNEL_STEPS, s.start_step, s.interval)
            tc.assert_same_records(rec, w)
            assert (w[:, 7] == 0).sum() > len(seeds)
            if levels > 1:
                assert H.info["level_changed"] >= 1 and H.info["midpoint_other_level"] >= 1
        state_b = [{n: d.download(n) for n in STATES} for d in dev_b]
    finally:
        for s in sets_b:
            s.close()
        for d in dev_b:
            d.close()
    for (start, interval), w in zip(tc.TUNNEL_SCHEDULES, want):
        _, _, dev_a = _tunnel(levels)
        s = tr.DeviceTracers(dev_a, seeds, tc.TUNNEL_G, tc.TUNNEL_EVERY, start, interval)
        try:
            execute_timestep_batch(dev_a, 1, tc.TUNNEL_STEPS, u, params, tracers=s)
            rec, n = _snapshot(s, tc.TUNNEL_STEPS)
            assert n == tr.advances_through(tc.TUNNEL_STEPS, start, interval)
            tc.assert_same_records(rec, w)
            for lvl, (d, b) in enumerate(zip(dev_a, state_b)):
                for name in STATES:
                    assert np.array_equal(d.download(name), b[name]), f"level {lvl + 1} {name}"
        finally:
            s.close()
            for d in dev_a:
                d.close()


@pytest.mark.gpu
def test_error_paths_and_the_empty_set(gpu):
    (g,), params = cases.periodic_box((3, 3, 3))                            # a state the batches below can step
    lib = _lib.load()
    d, other = adapt(g, 0), adapt(g, 0)
    seeds = tc.UNIFORM_SEEDS
    arr = (C.c_void_p * 1)(d.handle)
    out = C.c_void_p()

    def create(levels=arr, n_levels=1, n=len(seeds), sd=seeds.ctypes.data, generations=2, every=1, dt=1.0, res=C.byref(out)):
        return lib.ludwig_tracers_create(levels, n_levels, n, sd, generations, every, dt, res)
    try:
        for kw in ({"generations": 0}, {"generations": -1}, {"every": 0}, {"dt": 0.0}, {"dt": -1.0}, {"dt": float("nan")}, {"dt": float("inf")},
                   {"n": -1}, {"n_levels": 0}, {"sd": None}, {"levels": None}, {"n": 1 << 20, "generations": 1 << 10}):
            assert create(**kw) == -1 and out.value is None, kw              # LUDWIG_ERR_INVALID
            assert lib.ludwig_last_error()
        assert create(res=None) == -1
        # n_seeds = 0: a set that launches nothing and downloads nothing, in a batch and outside
        s = tr.DeviceTracers([d], np.zeros((0, 3), F32), 4, 1, 1, 1)
        assert lib.ludwig_tracers_download(s.handle, None, 0, None) == -5    # LUDWIG_ERR_STATE before the first snapshot
        s.advance(1)
        execute_timestep_batch([d], 1, 2, F32(0.0), params, tracers=s)
        rec, n = _snapshot(s, 2)
        assert rec.shape == (0, 8) and n == 3
        s.close()
        with pytest.raises(RuntimeError, match="closed"):
            s.advance(1)
        # a download before the first snapshot, a wrong byte count, null records, a negative step
        s = tr.DeviceTracers([d], seeds, 2, 1, 1, 1)
        buf = np.zeros((4, 8), F32)
        assert lib.ludwig_tracers_download(s.handle, buf.ctypes.data, buf.nbytes, None) == -5
        assert lib.ludwig_tracers_advance(s.handle, -1) == -1 and lib.ludwig_tracers_snapshot(s.handle, -1) == -1
        s.snapshot(1)
        assert lib.ludwig_tracers_download(s.handle, buf.ctypes.data, buf.nbytes - 4, None) == -1
        assert lib.ludwig_tracers_download(s.handle, None, buf.nbytes, None) == -1
        assert lib.ludwig_tracers_download(s.handle, buf.ctypes.data, buf.nbytes, None) == 0         # n_advances may be NULL
        assert (buf[:, 7] == tr.EMPTY).all() and (buf[:, 6] == -1).all() and (buf[:, 0:6] == 0).all()
        # a batch handed a set made over other levels, or a bad interval: refused before anything is stepped
        before = {n: other.download(n) for n in STATES}
        with pytest.raises(_lib.LudwigError) as e:
            execute_timestep_batch([other], 1, 2, F32(0.0), params, tracers=s)
        assert e.value.code == -1 and b"other levels" in lib.ludwig_last_error()
        s.interval = 0
        with pytest.raises(_lib.LudwigError) as e:
            execute_timestep_batch([d], 1, 2, F32(0.0), params, tracers=s)
        assert e.value.code == -1 and b"interval" in lib.ludwig_last_error()
        for n in STATES:
            assert np.array_equal(other.download(n), before[n]), n
        assert _snapshot(s, 1)[1] == 0                                      # and nothing was advanced
        s.close()
    finally:
        d.close()
        other.close()
    # LUDWIG_ERR_STATE: a level made without block_pointer, a level that holds ghost blocks
    bare = copy.copy(g)
    bare.block_pointer = np.zeros(0, np.int32)
    ghost = copy.copy(g)
    ghost.n_owned = g.n_blocks - 3
    for host, word in ((bare, b"block_pointer"), (ghost, b"ghost")):
        d = adapt(host, 0)
        try:
            with pytest.raises(_lib.LudwigError) as e:
                tr.DeviceTracers([d], seeds, 2, 1, 1, 1)
            assert e.value.code == -5 and word in lib.ludwig_last_error()
        finally:
            d.close()


CUBE = {"basic": {"num_levels": 3, "surface_resolution": 14, "simulation": {"steps": 10, "output_freq": 8, "ramp_steps": 4}},
        "advanced": {"diagnostics": {"freq": 4}}}
TRACERS = {"enabled": True, "start_step": 2, "interval": 1, "release_every": 2, "generations": 3, "output_interval": 4,
           "seeds": [{"name": "rake", "line": {"from": [-4.0, -1.5, -0.2], "to": [-4.0, 1.5, 0.3], "count": 5}},
                     {"name": "pts", "points": [[-2.0, 0.3, 0.1], [0.0, 0.0, 0.0], [1.0e3, 0.0, 0.0], [-3.9, 0.6, -0.4]]}]}


@pytest.mark.gpu
def test_run_case_advances_inside_the_batches_and_leaves_the_rest_unchanged(gpu, tmp_path):
    """cube1m, 10 coarse steps, advances from step 2 on at interval 1, snapshots after steps 2, 6 and 10: batch boundaries only where
    output_interval puts them, the files hold what the restatement makes of the downloaded fields, every other file keeps its bytes"""
    stl = os.path.join(G, "cube1m.stl")
    runs = {}
    for on in (False, True):
        over = copy.deepcopy(CUBE)
        if on:
            over["advanced"]["tracers"] = TRACERS
        cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), over)
        setup = pp.setup_multilevel_domain(cfg, stl)
        batches, snaps = [], {}

        class Recording(case.HipStepper):
            def batch(self, t_start, n, u_curr, params):
                batches.append((t_start, n))
                super().batch(t_start, n, u_curr, params)

            def tracers_snapshot(self, t_coarse):
                snaps[t_coarse] = super().tracers_snapshot(t_coarse)
                return snaps[t_coarse]
        out = os.path.join(tmp_path, "on" if on else "off")
        lines = []
        case.run_case(cfg, Recording, setup=setup, out_dir=out, log=lines.append)
        runs[on] = (out, cfg, setup, batches, snaps, lines)
    off, on = runs[False][0], runs[True][0]
    cfg, (grids, _, params, _), batches, snaps, lines = runs[True][1:]
    steps = [2, 6, 10]
    # the run without the key cuts where async_depth does; with it, additionally after the snapshot steps - and nowhere else
    ends_off, ends_on = [a + n - 1 for a, n in runs[False][3]], [a + n - 1 for a, n in batches]
    assert ends_on == sorted(set(ends_off) | set(steps)) and len(ends_on) < 9
    new = [f"tracers_{n}_{s:06d}.vtp" for n in ("rake", "pts") for s in steps] + ["tracers_rake.pvd", "tracers_pts.pvd"]
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + new)
    for name in os.listdir(off):
        if name != "convergence.csv":                                       # wall time and MLUPS columns
            assert filecmp.cmp(os.path.join(off, name), os.path.join(on, name), shallow=False), name
    from open_ludwig_amd.slices import read_pvd
    for n in ("rake", "pts"):
        assert read_pvd(os.path.join(on, f"tracers_{n}.pvd")) == [(s * params.time_scale, f"tracers_{n}_{s:06d}.vtp") for s in steps]
    assert not runs[False][4] and sorted(snaps) == steps
    plan = tr.TracerPlan([(s.name, np.asarray(s.points)) for s in cfg.tracers_seeds], params.mesh_offset, grids[0].dx)
    assert plan.n_seeds == 9
    written = 0
    for s_step in steps:
        rec, k = snaps[s_step]
        assert k == s_step - 1                                              # one advance per coarse step from step 2 on
        for gi, name in enumerate(("rake", "pts")):
            p = tr.group_particles(plan, gi, rec, k, s_step, 3, 2, 2, 1)
            arr = tr.read_vtp(os.path.join(on, f"tracers_{name}_{s_step:06d}.vtp"))
            assert int(arr["NumberOfPoints"]) == int(arr["NumberOfVerts"]) == len(p.points) and int(arr["NumberOfLines"]) == len(p.offsets)
            assert np.array_equal(arr["Points"], p.points) and np.array_equal(arr["Velocity"], p.vel) and np.array_equal(arr["Level"], p.level)
            assert np.array_equal(arr["ParticleId"], p.particle_id) and np.array_equal(arr["Seed"], p.seed) and np.array_equal(arr["Age"], p.age)
            assert np.array_equal(arr["connectivity"], p.connectivity) and np.array_equal(arr["offsets"], p.offsets)
            written += len(p.points)
            assert sum(f"tracers {name!r}: step {s_step}:" in l for l in lines) == 1
    assert written > 0
    # a particle keeps its id across files: release 2's rake particles (ids 18..22), born behind step 6, are in the last two files
    a, b = (tr.read_vtp(os.path.join(on, f"tracers_rake_{s:06d}.vtp")) for s in (6, 10))
    for pid in range(18, 23):
        assert a["Age"][a["ParticleId"] == pid].tolist() == [0] and b["Age"][b["ParticleId"] == pid].tolist() == [4]
