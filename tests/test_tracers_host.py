"""Tracers, host side: the numpy restatement of the definition (tracers.advance_host / snapshot_host - the checker the device is compared
with), the release ring's bookkeeping, the configuration keys, the streaklines, the PolyData writer and the bindings. No GPU."""
import copy
import ctypes as C
import filecmp
import os
import re

import numpy as np
import pytest

import _streamline_cases as sc
import _tracer_cases as tc
from open_ludwig_amd import _lib, case, cases, output, preprocess as pp, tracers as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(G, "cube1m_config.yaml")
F32 = np.float32


def test_uniform_flow_moves_by_dt_u_and_dies_where_the_midpoint_leaves_the_grid():
    g = sc.box27()
    _, vel = sc.uniform_fields()
    lv = tc.velocity_level(g, vel)
    P, state = tr.new_state(2, 1)
    assert P.dtype == F32 and state.dtype == np.int32 and (state == tr.EMPTY).all()
    history = []
    for k in range(tc.UNIFORM_ADVANCES):
        tr.advance_host(lv, P, state, tc.UNIFORM_SEEDS, k, 1, 1000, 1.0)
        history.append((P.copy(), state.copy()))
    tc.check_uniform(history)
    rec = tr.snapshot_host(lv, P, state)
    assert rec.dtype == F32 and rec.shape == (2, 8)
    assert rec[0].tolist() == [*P[0].tolist(), 0.0, 0.0, 0.0, -1.0, 1.0]                  # dead: position, zeros, level -1, its state
    assert np.array_equal(rec[1, 0:3], P[1]) and abs(rec[1, 3] - sc.U0) < 1e-8 and rec[1, 4:].tolist() == [0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("dt", [1, 4])
def test_solid_body_rotation_keeps_its_radius_and_euler_would_not(dt):
    """one full turn: the midpoint rule drifts by at most 1e-3 cells (measured 3.7e-5 at dt = 1, 2.3e-5 at dt = 4), the same loop with the
    midpoint removed by 0.05-0.10 (dt = 1) and 0.21-0.41 cells (dt = 4): a restatement that lost its midpoint fails here"""
    g = sc.box27()
    _, vel = sc.rotation_fields()
    lv = tc.velocity_level(g, vel)
    seeds, n = tc.rotation_seeds(), tc.ROTATION_ADVANCES[dt]
    P, state = tr.new_state(len(seeds), 1)
    for k in range(n + 1):                                                  # advance 0 releases, n moves follow
        tr.advance_host(lv, P, state, seeds, k, 1, 10 ** 6, float(dt))
    drift = np.abs(tc.radii(P) - tc.radii(seeds))
    euler = np.abs(tc.radii(tc.euler_host(lv, seeds, n, dt)) - tc.radii(seeds))
    print(f"rotation dt {dt} n {n}: drift {drift.tolist()}; Euler {euler.tolist()}")
    assert (state == tr.ALIVE).all() and (drift <= tc.ROTATION_DRIFT).all()
    lo, hi = tc.EULER_DRIFT[dt]
    assert (euler >= 0.95 * lo).all() and (euler <= 1.05 * hi).all()
    assert np.abs(P[:, 2] - seeds[:, 2]).max() <= 1e-4


def test_planted_states_reach_every_code_and_a_dead_slot_keeps_its_position():
    g, vel, seeds = tc.planted()
    lv = tc.velocity_level(g, vel)
    P, state = tr.new_state(len(seeds), 1)
    died_at = {}
    for k in range(tc.PLANTED_ADVANCES):
        before, was = P.copy(), state.copy()
        tr.advance_host(lv, P, state, seeds, k, 1, 10 ** 6, tc.PLANTED_DT)
        if k > 0:
            dead = was != tr.ALIVE
            assert np.array_equal(P[dead], before[dead], equal_nan=True) and np.array_equal(state[dead], was[dead])
            newly = (was == tr.ALIVE) & (state != tr.ALIVE)
            assert np.array_equal(P[newly], before[newly], equal_nan=True)  # P stays where the sample failed
            for i in np.flatnonzero(newly):
                died_at[int(i)] = k
    assert set(state.tolist()) == {tr.ALIVE, tr.OUTSIDE, tr.OBSTACLE, tr.NONFINITE}
    assert {i: int(state[i]) for i in tc.PLANTED_ENDS} == tc.PLANTED_ENDS
    assert died_at[1] == died_at[2] == died_at[3] == 1                      # a bad seed dies at its first advance, not at its release
    rec = tr.snapshot_host(lv, P, state)
    assert np.array_equal(rec[:, 7], state.astype(F32)) and np.array_equal(rec[:, 0:3], P, equal_nan=True)
    assert (rec[state != 0, 3:7] == np.array([0, 0, 0, -1], F32)).all() and (rec[state == 0, 6] == 0).all()


def test_release_ring_overwrites_the_oldest_generation_without_advancing_it():
    g = sc.box27()
    _, vel = sc.uniform_fields()
    lv = tc.velocity_level(g, vel)
    n, G_, every = len(tc.RING_SEEDS), tc.RING_G, tc.RING_EVERY
    H = tr.HostTracers(tc.RING_SEEDS, G_, every, tc.RING_DT)
    for k in range(tc.RING_ADVANCES):
        before = H.state.copy()
        H.advance(lv)
        st = H.state.reshape(G_, n)
        released = k // every + 1                                           # releases so far
        for gen in range(G_):
            assert (st[gen] == tr.EMPTY).all() == (gen >= released), (k, gen)          # empty before a generation's first release
        for K, start, interval in ((k + 1, 1, 1), (k + 1, 5, 3)):
            got, want = tr.slot_ids(K, n, G_, every, start, interval), tc.slot_ids_loop(K, n, G_, every, start, interval)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (K, got, want)
        if k == 6:                                                          # the fourth release: generation 0 again
            assert (before.reshape(G_, n)[0] != tr.ALIVE).sum() >= 2        # it held dead slots
            assert (st[0] == tr.ALIVE).all() and np.array_equal(H.P[:n], tc.RING_SEEDS, equal_nan=True)      # overwritten, not advanced
    assert H.n_advances == tc.RING_ADVANCES
    rel, pid, birth = tr.slot_ids(tc.RING_ADVANCES, n, G_, every, 5, 3)
    assert rel.reshape(G_, n)[:, 0].tolist() == [3, 4, 2] and pid.reshape(G_, n)[1].tolist() == [20, 21, 22, 23, 24]
    assert birth.reshape(G_, n)[:, 0].tolist() == [5 + 3 * 6, 5 + 4 * 6, 5 + 2 * 6]
    assert all((a == -1).all() for a in tr.slot_ids(0, n, G_, every))
    assert tr.advances_through(4, 5, 3) == 0 and tr.advances_through(5, 5, 3) == 1 and tr.advances_through(10, 5, 3) == 2


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_tunnel_rake_changes_level_between_advances_and_at_midpoints(levels):
    """the inputs of the device test, from the CPU oracle: on more than one level a particle changes level between two advances and a
    midpoint lies on another level than its start, at interval 1 and at start_step 2, interval 2"""
    from oracle import oracle
    oracle.set_num_threads(min(8, os.cpu_count() or 1))
    seeds = tc.tunnel_seeds()
    for start, interval in tc.TUNNEL_SCHEDULES:
        grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)

        class Fields:
            def field(self, li, name):
                return getattr(grids[li], name)
        H = tr.HostTracers(seeds, tc.TUNNEL_G, tc.TUNNEL_EVERY, interval)
        for t in range(1, tc.TUNNEL_STEPS + 1):
            oracle.execute_timestep_batch(grids, t, 1, F32(0.05), params)
            if t >= start and (t - start) % interval == 0:
                H.advance(tr.stepper_levels(Fields(), grids, t))
        assert H.n_advances == tr.advances_through(tc.TUNNEL_STEPS, start, interval)
        rec = H.snapshot(tr.stepper_levels(Fields(), grids, tc.TUNNEL_STEPS))
        assert (rec[:, 7] == 0).sum() > len(seeds)
        if levels > 1:
            assert H.info["level_changed"] >= 1 and H.info["midpoint_other_level"] >= 1
            assert set(rec[rec[:, 7] == 0, 6].tolist()) == set(range(levels))


SEEDS = [{"name": "a", "points": [[-4.0, 0.1, 0.2]]}]


def _load(tracer_cfg, steps=None):
    over = {"advanced": {"tracers": tracer_cfg}}
    if steps is not None:
        over["basic"] = {"simulation": {"steps": steps}}
    return pp.load_case_configuration(CFG, over)


def test_configuration_defaults_and_parsing():
    for name in ("ball1m_config.yaml", "cube1m_config.yaml", "bunny_config.yaml"):
        cfg = pp.load_case_configuration(os.path.join(G, name))
        assert not cfg.tracers_enabled and cfg.tracers_seeds == ()
        assert (cfg.tracers_start_step, cfg.tracers_interval, cfg.tracers_release_every, cfg.tracers_generations, cfg.tracers_output_interval,
                cfg.tracers_max_particles) == (1, 1, 10, 64, 100, 4_000_000)
    assert not _load({"enabled": False, "seeds": [{"name": ""}]}).tracers_enabled
    cfg = _load({"enabled": True, "start_step": 3, "interval": 2, "release_every": 5, "generations": 7, "output_interval": 8, "max_particles": 28,
                 "seeds": SEEDS + [{"name": "b-1", "line": {"from": [0, 0, 0], "to": [2, 0, 0], "count": 3}}]})
    assert cfg.tracers_enabled and (cfg.tracers_start_step, cfg.tracers_interval, cfg.tracers_release_every, cfg.tracers_generations,
                                    cfg.tracers_output_interval, cfg.tracers_max_particles) == (3, 2, 5, 7, 8, 28)      # 4 x 7: exactly the cap
    a, b = cfg.tracers_seeds
    assert (a.name, a.points) == ("a", ((-4.0, 0.1, 0.2),)) and (b.name, b.points) == ("b-1", ((0.0, 0, 0), (1.0, 0, 0), (2.0, 0, 0)))


@pytest.mark.parametrize("tracer_cfg, key", [
    ({"enabled": True, "seeds": []}, "advanced.tracers.seeds"),
    ({"enabled": True, "seeds": [{"points": [[0, 0, 0]]}]}, "advanced.tracers.seeds[0].name"),
    ({"enabled": True, "seeds": SEEDS + SEEDS}, "advanced.tracers.seeds[1].name"),
    ({"enabled": True, "seeds": [{"name": "a"}]}, "advanced.tracers.seeds[0]"),
    ({"enabled": True, "seeds": [{"name": "a", "points": [[0, 0]]}]}, "advanced.tracers.seeds[0].points"),
    ({"enabled": True, "interval": 0, "seeds": SEEDS}, "advanced.tracers.interval"),
    ({"enabled": True, "start_step": 0, "seeds": SEEDS}, "advanced.tracers.start_step"),
    ({"enabled": True, "release_every": 0, "seeds": SEEDS}, "advanced.tracers.release_every"),
    ({"enabled": True, "generations": 0, "seeds": SEEDS}, "advanced.tracers.generations"),
    ({"enabled": True, "output_interval": 0, "seeds": SEEDS}, "advanced.tracers.output_interval"),
    ({"enabled": True, "interval": 4, "output_interval": 6, "seeds": SEEDS}, "advanced.tracers.output_interval"),
    ({"enabled": True, "max_particles": 0, "seeds": SEEDS}, "advanced.tracers.max_particles"),
    ({"enabled": True, "generations": 8, "max_particles": 7, "seeds": SEEDS}, "advanced.tracers.max_particles"),
    ({"enabled": True, "interval": "x", "seeds": SEEDS}, "advanced.tracers"),
    ([1, 2], "advanced.tracers"),
])
def test_configuration_errors_name_their_key(tracer_cfg, key):
    with pytest.raises(ValueError) as e:
        _load(tracer_cfg)
    assert key in str(e.value), str(e.value)


def test_particle_id_overflow_and_jump_warning_are_named_before_the_first_step():
    big = {"enabled": True, "release_every": 1, "generations": 2, "max_particles": 10 ** 7,
           "seeds": [{"name": "r", "line": {"from": [0, 0, 0], "to": [1, 1, 1], "count": 3000}}]}
    _load(big, steps=700_000)                                               # 700 000 releases x 3 000 seeds < 2^31
    with pytest.raises(ValueError, match="ParticleId"):
        _load(big, steps=720_000)
    tr.check_capacity(3, 2, 6, 10, 1, 1, 1)
    with pytest.raises(ValueError, match="max_particles"):
        tr.check_capacity(3, 2, 5, 10, 1, 1, 1)
    assert tr.jump_warning(1, 0.05, 3) is None and tr.jump_warning(5, 0.05, 3) is None          # 1.0 exactly: no warning
    w = tr.jump_warning(6, 0.05, 3)
    assert w and "finest cell" in w and "interval 6" in w


def test_streaklines_run_newest_first_and_break_at_a_dead_particle():
    n, G_ = 3, 5
    K = 9                                                                   # release_every 2: releases 0..4, generation g holds release g
    rel, pid, _ = tr.slot_ids(K, n, G_, 2)
    assert rel.reshape(G_, n)[:, 0].tolist() == [0, 1, 2, 3, 4]
    alive = np.ones((G_, n), bool)
    alive[2, 1] = False                                                     # seed 1: 4 3 | 1 0
    alive[3, 2] = alive[1, 2] = False                                       # seed 2: 4 | 2 | 0: no run of two
    lines = tr.streaklines(alive.reshape(-1), rel, n, G_)
    slot = lambda g, s: g * n + s
    assert [l.tolist() for l in lines] == [[slot(4, 0), slot(3, 0), slot(2, 0), slot(1, 0), slot(0, 0)],
                                           [slot(4, 1), slot(3, 1)], [slot(1, 1), slot(0, 1)]]
    # after the ring has wrapped (K = 13: releases 0..6, generations hold 5, 6, 2, 3, 4) the order follows the release, not the slot
    rel, _, _ = tr.slot_ids(13, n, G_, 2)
    lines = tr.streaklines(np.ones(n * G_, bool), rel, n, G_)
    assert lines[0].tolist() == [slot(1, 0), slot(0, 0), slot(4, 0), slot(3, 0), slot(2, 0)]
    # a generation never released is empty and ends the line
    rel, _, _ = tr.slot_ids(3, n, G_, 2)
    assert [l.tolist() for l in tr.streaklines(np.ones(n * G_, bool), rel, n, G_)] == [[slot(1, s), slot(0, s)] for s in range(n)]


def test_write_vtp_tracers_round_trip(tmp_path):
    g = sc.box27()
    _, vel = sc.uniform_fields()
    lv = tc.velocity_level(g, vel)
    n, G_, every = len(tc.RING_SEEDS), tc.RING_G, tc.RING_EVERY
    H = tr.HostTracers(tc.RING_SEEDS, G_, every, tc.RING_DT)
    for _ in range(6):                                                      # every generation released once, none twice
        H.advance(lv)
    rec = H.snapshot(lv)
    plan = tr.TracerPlan([("two", np.zeros((2, 3))), ("three", np.zeros((3, 3)))], (0, 0, 0), 0.25)
    plan.seeds = tc.RING_SEEDS
    start, interval, step = 5, 8, 5 + 5 * 8
    rel, pid, birth = tr.slot_ids(6, n, G_, every, start, interval)
    for gi, name in enumerate(plan.names):
        p = tr.group_particles(plan, gi, rec, 6, step, G_, every, start, interval)
        keep = np.flatnonzero((rec[:, 7] == 0) & np.tile(plan.group == gi, G_))
        assert keep.size > 0 and np.array_equal(p.particle_id, pid[keep]) and np.array_equal(p.age, step - birth[keep])
        assert np.array_equal(p.seed, np.tile(plan.seed_index, G_)[keep]) and (p.level == 1).all()
        for compress in (True, False):
            path = output.write_vtp_tracers(str(tmp_path / f"{name}{int(compress)}"), p.points, p.vel, p.level, p.particle_id, p.seed, p.age,
                                            p.connectivity, p.offsets, compress)
            assert path.endswith(".vtp") and not os.path.exists(path + ".part")
            text = open(path).read()
            assert 'type="PolyData"' in text and "<Verts>" in text and "<Lines>" in text and ("vtkZLibDataCompressor" in text) == compress
            arr = tr.read_vtp(path)
            assert int(arr["NumberOfPoints"]) == int(arr["NumberOfVerts"]) == keep.size and int(arr["NumberOfLines"]) == len(p.offsets)
            assert np.array_equal(arr["verts_connectivity"], np.arange(keep.size)) and np.array_equal(arr["verts_offsets"], np.arange(1, keep.size + 1))
            assert np.array_equal(arr["Points"], (rec[keep, 0:3].astype(np.float64) * 0.25).astype(F32)) and arr["Points"].dtype == F32
            assert np.array_equal(arr["Velocity"], rec[keep, 3:6]) and np.array_equal(arr["Level"], p.level) and arr["Level"].dtype == np.int32
            assert np.array_equal(arr["ParticleId"], p.particle_id) and np.array_equal(arr["Seed"], p.seed) and np.array_equal(arr["Age"], p.age)
            assert np.array_equal(arr["connectivity"], p.connectivity) and np.array_equal(arr["offsets"], p.offsets)
    # group "two" = the seeds (23.2, ..) and (3.25, ..): the second is alive in all three generations, newest first
    p = tr.group_particles(plan, 0, rec, 6, step, G_, every, start, interval)
    ids = [p.particle_id[p.connectivity[a:b]].tolist() for a, b in zip(np.r_[0, p.offsets[:-1]], p.offsets)]
    assert [2 * n + 1, n + 1, 1] in ids and all(a > b for l in ids for a, b in zip(l, l[1:]))
    assert "alive" in tr.summary(plan, 0, rec, G_) and "empty 0" in tr.summary(plan, 0, rec, G_)
    # no particle at all is a valid file
    none = tr.group_particles(plan, 0, rec, 0, step, G_, every, start, interval)
    arr = tr.read_vtp(output.write_vtp_tracers(str(tmp_path / "empty"), none.points, none.vel, none.level, none.particle_id, none.seed, none.age,
                                               none.connectivity, none.offsets))
    assert int(arr["NumberOfPoints"]) == 0 and int(arr["NumberOfLines"]) == 0


TRACER_CFG = {"enabled": True, "start_step": 2, "interval": 1, "release_every": 2, "generations": 2, "output_interval": 3,
              "seeds": [{"name": "rake", "line": {"from": [-4.0, -1.5, -0.2], "to": [-4.0, 1.5, 0.3], "count": 5}},
                        {"name": "pts", "points": [[-2.0, 0.3, 0.1], [0.0, 0.0, 0.0], [1.0e3, 0.0, 0.0]]}]}


def test_run_case_with_a_stepper_without_tracers_advances_on_the_host(tmp_path):
    """the CPU oracle behind run_case: HostTracers on downloaded velocity, batches cut at every advance step, files at the snapshot
    steps, every other file unchanged"""
    from _steppers import OracleStepper
    from oracle import oracle
    oracle.set_num_threads(min(8, os.cpu_count() or 1))
    base = {"basic": {"num_levels": 1, "surface_resolution": 7, "simulation": {"steps": 6, "output_freq": 8, "ramp_steps": 4}},
            "advanced": {"boundary": {"method": "bounce_back"}, "high_re": {"wall_model": {"enabled": False}},
                         "numerics": {"c_wale": 0.0, "nu_sgs_background": 0.0}, "diagnostics": {"freq": 4}}}
    outs, lines, batches = {}, [], {False: [], True: []}
    for on in (False, True):
        over = copy.deepcopy(base)
        if on:
            over["advanced"]["tracers"] = TRACER_CFG
        cfg = pp.load_case_configuration(CFG, over)
        outs[on] = str(tmp_path / ("on" if on else "off"))

        class Recording(OracleStepper):
            def batch(self, t_start, n, u_curr, params, _log=batches[on]):
                _log.append((t_start, n))
                super().batch(t_start, n, u_curr, params)
        case.run_case(cfg, Recording, stl_path=os.path.join(G, "cube1m.stl"), out_dir=outs[on], log=lines.append)
    assert [b[0] + b[1] - 1 for b in batches[True]] == [2, 3, 4, 5, 6] and len(batches[False]) < 5          # from start_step 2 on
    new = [f"tracers_{n}_{t:06d}.vtp" for n in ("rake", "pts") for t in (2, 5)] + ["tracers_rake.pvd", "tracers_pts.pvd"]
    assert sorted(os.listdir(outs[True])) == sorted(os.listdir(outs[False]) + new)
    for name in os.listdir(outs[False]):
        if name != "convergence.csv":
            assert filecmp.cmp(os.path.join(outs[False], name), os.path.join(outs[True], name), shallow=False), name
    from open_ludwig_amd.slices import read_pvd
    assert [f for _, f in read_pvd(os.path.join(outs[True], "tracers_rake.pvd"))] == ["tracers_rake_000002.vtp", "tracers_rake_000005.vtp"]
    first = tr.read_vtp(os.path.join(outs[True], "tracers_rake_000002.vtp"))
    assert first["ParticleId"].tolist() == [0, 1, 2, 3, 4] and first["Age"].tolist() == [0] * 5 and int(first["NumberOfLines"]) == 0
    rake = tr.read_vtp(os.path.join(outs[True], "tracers_rake_000005.vtp"))          # 4 advances: releases 0 (step 2) and 1 (step 4) of 8 seeds
    assert sorted(rake["ParticleId"].tolist()) == [0, 1, 2, 3, 4, 8, 9, 10, 11, 12] and set(rake["Level"].tolist()) == {1}
    assert sorted(set(rake["Age"].tolist())) == [1, 3] and int(rake["NumberOfLines"]) == 5 and rake["offsets"].tolist() == [2, 4, 6, 8, 10]
    logged = [l for l in lines if l.startswith("tracers 'pts': step 5")]
    assert len(logged) == 1 and "6 slots" in logged[0] and "outside 2" in logged[0]


def test_distributed_stepper_refuses_and_names_the_key():
    st = object.__new__(case.DistributedStepper)                           # the refusal needs no device and no process group
    with pytest.raises(RuntimeError, match=r"advanced\.tracers"):
        st.tracers_setup(None)
    cfg = pp.load_case_configuration(CFG, {"basic": {"num_levels": 1, "surface_resolution": 7},
                                           "advanced": {"tracers": {"enabled": True, "seeds": SEEDS}}})
    closed = []

    class Refusing:
        def __init__(self, grids):
            pass

        tracers_setup = case.DistributedStepper.tracers_setup

        def close(self):
            closed.append(True)
    with pytest.raises(RuntimeError, match=r"advanced\.tracers"):
        case.run_case(cfg, Refusing, stl_path=os.path.join(G, "cube1m.stl"), steps=1)
    assert closed == [True]


def test_header_exports_and_julia_list_the_tracer_calls():
    new = ["ludwig_tracers_create", "ludwig_tracers_destroy", "ludwig_tracers_advance", "ludwig_tracers_snapshot", "ludwig_tracers_download",
           "ludwig_execute_timestep_batch_tracers"]
    header = open(os.path.join(ROOT, "include", "ludwig_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "LudwigHIP.jl")).read()
    lib = _lib.load()
    for name in new:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        # the binding reaches an in-batch observer through the observed batch call, as an entry of the observer's kind
        called = "ludwig_execute_timestep_batch_observed" if name.startswith("ludwig_execute_timestep_batch_") else name
        assert f"(:{called}, LIB)" in jl, name
    assert "entry(OBSERVE_TRACERS, tracers, start_step, interval)" in jl
    assert lib.ludwig_abi_version() == 1
    for name, k in (("EMPTY", tr.EMPTY), ("ALIVE", tr.ALIVE), ("OUTSIDE", tr.OUTSIDE), ("OBSTACLE", tr.OBSTACLE), ("NONFINITE", tr.NONFINITE)):
        assert re.search(r"LUDWIG_TRACER_" + name + r"\s*=\s*%d\b" % k, header), name


def test_calls_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    out = C.c_void_p(1)
    assert lib.ludwig_tracers_create(None, 1, 0, None, 1, 1, 1.0, C.byref(out)) == -1 and out.value is None
    assert lib.ludwig_tracers_create(None, 1, 0, None, 1, 1, 1.0, None) == -1
    assert lib.ludwig_tracers_advance(None, 1) == -1
    assert lib.ludwig_tracers_snapshot(None, 1) == -1
    assert lib.ludwig_tracers_download(None, None, 0, None) == -1
    assert b"null" in lib.ludwig_last_error()
    lib.ludwig_tracers_destroy(None)
