"""What tests/test_gpu_record_state.py stands on, checked without a device: the table of entry points is complete, the states it steps
through differ from step to step nearly everywhere (so that a reader of stale arrays cannot pass a bit-for-bit comparison), the nest of
its ban test builds and stays finite, and every reader with a host restatement gives another output on the state of two steps earlier."""
import os
import re

import numpy as np
import pytest

import _observer_sets as obs
import _record_state_cases as rc
import test_gpu_record_state as gpu_tests
from open_ludwig_amd import _lib, flux_planes as fp, isosurface as iso, monitor as mon, preprocess as pp, render as rd, streamlines as st
from open_ludwig_amd import tracers as tr
from oracle import oracle

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the table ----
def declared_in_header():
    text = open(os.path.join(ROOT, "include", "ludwig_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return set(re.findall(r"\b(ludwig_[a-z0-9_]+)\s*\(", text))


def test_every_entry_point_is_classed():
    header, exported, table = declared_in_header(), set(_lib.EXPORTED_SYMBOLS), set(rc.ENTRY_POINTS)
    assert len(header) > 100, "the header's declarations were not found"
    assert not (header | exported) - table, f"not classed in tests/_record_state_cases.py: {sorted((header | exported) - table)}"
    assert not table - exported, f"the table names what the library does not export: {sorted(table - exported)}"
    for name, entry in rc.ENTRY_POINTS.items():
        assert entry[0] in (rc.READER, rc.WRITER, rc.RULER, rc.NEUTRAL, rc.UNCOVERED), name


def test_every_reader_writer_and_ruler_names_a_case_that_exists():
    uncovered = [n for n, e in rc.ENTRY_POINTS.items() if e[0] == rc.UNCOVERED]
    assert len(uncovered) <= rc.MAX_UNCOVERED, uncovered
    for name in uncovered:
        assert len(rc.ENTRY_POINTS[name]) == 3 and rc.ENTRY_POINTS[name][2], f"{name}: an uncovered entry says why"
    for name, entry in rc.ENTRY_POINTS.items():
        if entry[0] in (rc.NEUTRAL, rc.UNCOVERED):
            assert entry[1] is None, name
            continue
        cases = entry[1] if isinstance(entry[1], tuple) else (entry[1],)
        assert cases and all(cases), f"{name}: a {entry[0]} names its case"
        for case in cases:
            m = re.fullmatch(r"(\w+)(?:\[(.+)\])?", case)
            assert m, f"{name}: case {case!r}"
            fn, param = m.groups()
            assert fn in rc.CASE_FUNCTIONS and callable(getattr(gpu_tests, fn, None)), f"{name}: no test {fn}"
            if param is not None:
                assert param in gpu_tests.PARAMETERS[fn], f"{name}: {fn} has no case {param}"
            else:
                assert fn not in gpu_tests.PARAMETERS or fn == "test_seeded_walk", f"{name}: {fn} is parametrised, name the case"
    for fn in rc.CASE_FUNCTIONS:
        assert callable(getattr(gpu_tests, fn, None)), fn


def test_every_reader_kind_of_the_helpers_is_a_first_reader_or_a_ban():
    assert set(gpu_tests.FIRST_READERS) | set(obs.BANNING_KINDS) == set(obs.KINDS) | set(obs.LEVEL_KINDS) | set(gpu_tests.DOWNLOADS)
    assert set(gpu_tests.IN_BATCH) <= set(obs.KINDS)


# ---- staleness can show ----
@pytest.mark.parametrize("nb", [gpu_tests.NB, gpu_tests.NB2], ids=lambda b: "x".join(map(str, b)))
def test_the_newest_state_differs_from_what_its_buffers_held_two_steps_earlier(nb):
    states = gpu_tests.oracle_states(nb)
    for n in range(1, 6):
        fn, vn = oracle.newest_buffers(0, n)
        earlier = states[max(n - 2, 0)]                     # the last time these buffers were written, or the upload
        for name in (fn, vn, "rho"):
            now, then = states[n][name], earlier[name]
            assert np.isfinite(now).all()
            share = float(np.mean(now != then))
            assert share >= 0.99, f"{nb}, step {n}, {name}: only {share:.6f} of the elements differ from step {max(n - 2, 0)}"
        assert (states[n]["rho"] != states[n - 1]["rho"]).mean() >= 0.99, f"{nb}, step {n}: rho against the step before"


def test_the_nest_of_the_ban_test_builds_and_stays_finite():
    grids, params = gpu_tests.nest()
    assert [g.n_blocks for g in grids] == [27, 8] and grids[1].level_id == 2
    oracle.execute_timestep_batch(grids[:1], 1, 2, F32(0.0), params)
    before = {name: getattr(grids[1], name).copy() for name in ("f", "vel", "rho")}
    oracle.execute_timestep_batch(grids, 3, 2, F32(0.0), params)
    oracle.execute_timestep_batch(grids[:1], 5, 1, F32(0.0), params)
    for g in grids:
        for name in gpu_tests.STATE:
            assert np.isfinite(getattr(g, name)).all(), (g.level_id, name)
    for name, a in before.items():
        assert (getattr(grids[1], name) != a).mean() > 0.99, f"level 2 {name} did not move"


def test_the_walks_step_and_read():
    plans = [gpu_tests.walk_plan(seed) for seed in range(5)]
    assert all(len(p) == 12 for p in plans) and plans == [gpu_tests.walk_plan(seed) for seed in range(5)]
    drawn = {op for p in plans for op, _ in p}
    assert drawn == set(gpu_tests.WALK_OPS), f"never drawn: {set(gpu_tests.WALK_OPS) - drawn}"


# ---- readers with a host restatement: another state, another output ----
def _host_readers(grids):
    g = grids[0]
    plan = fp.plan_flux_plane(pp.FluxPlane("x", 0, 12.0, None, 1.0), grids)
    cam, persp = rd.Camera.build(obs.CAMERA, *obs.IMAGE_SIZE).arrays()
    table = rd.bake_table("coolwarm", 0.05)
    coords = np.asarray(g.active_block_coords)

    def tracers(rho, vel):
        T = tr.HostTracers(obs.SEEDS, 2, 1, 1.0)
        levels = tr.velocity_levels(grids, lambda li: vel)
        T.advance(levels)
        T.advance(levels)
        return [T.snapshot(levels)]

    def surface(rho, vel, value):
        s = iso.scalar_host("velocity_magnitude", rho, vel, None, None)
        out = iso.extract_host(s, g.obstacle, g.neighbor_table, None, np.zeros(3, np.int32), np.full(3, iso.CELL_MAX, np.int32), value, rho, vel, coords)
        assert out[0].shape[0] > 0
        return list(out)

    def image(rho, vel, lo, hi):
        levels = rd.host_levels(grids, [rd.scalar_host("velocity_magnitude", rho, vel, None, None)])
        return list(rd.render_host(levels, camera=cam, perspective=persp, width=obs.IMAGE_SIZE[0], height=obs.IMAGE_SIZE[1], step=0.5, lo=lo, hi=hi,
                                   max_samples=4096, table=table))

    return {
        "monitor.host_monitor": lambda rho, vel, ref: [mon.host_monitor(rho, vel, g.obstacle, g.active_block_coords)],
        "flux_planes.host_record": lambda rho, vel, ref: list(fp.host_record(plan, lambda li: (rho, vel))),
        "streamlines.trace_host": lambda rho, vel, ref: list(st.trace_host(st.host_levels(grids, lambda li: (rho, vel)), obs.SEEDS,
                                                                           np.ones(len(obs.SEEDS), F32), 0.5, 1.0e-6, 40)),
        "isosurface.extract_host": lambda rho, vel, ref: surface(rho, vel, obs.iso_values(ref)[1]),
        "render.render_host": lambda rho, vel, ref: image(rho, vel, *obs.render_ranges(ref)["velocity_magnitude"]),
        "tracers.advance_host": lambda rho, vel, ref: tracers(rho, vel),
    }


HOST_READERS = ("monitor.host_monitor", "flux_planes.host_record", "streamlines.trace_host", "isosurface.extract_host", "render.render_host",
                "tracers.advance_host")


def _differ(a, b):
    if len(a) != len(b):
        return True
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.asarray(x), np.asarray(y)
            if x.shape != y.shape or not np.array_equal(x, y):
                return True
        elif x != y:
            return True
    return False


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", HOST_READERS)
def test_a_host_reader_gives_another_output_on_the_state_of_two_steps_earlier(name, n):
    grids, _ = gpu_tests.box()
    states = gpu_tests.oracle_states(gpu_tests.NB)
    read = _host_readers(grids)[name]
    vn = obs.newest_vel(n)
    now, then = states[n], states[max(n - 2, 0)]
    ref = gpu_tests.newest(now, n)
    a, b = read(now["rho"], now[vn], ref), read(then["rho"], then[vn], ref)
    assert _differ(a, b), f"{name}: the states after {n} and {max(n - 2, 0)} steps give the same output"
    assert not _differ(a, read(now["rho"], now[vn], ref)), f"{name} is not a function of its input"
