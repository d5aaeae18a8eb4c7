"""Streamlines, host side: the numpy restatement of the definition (streamlines.trace_host - the checker the device is compared with),
the seeds, the configuration keys, the PolyData writer and the bindings. No GPU."""
import copy
import filecmp
import os
import re

import numpy as np
import pytest

import _streamline_cases as sc
from open_ludwig_amd import _lib, case, cases, output, preprocess as pp, streamlines as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(G, "cube1m_config.yaml")
F32 = np.float32


def test_uniform_flow_gives_exact_vertices_and_ends_at_the_grid_edge():
    g = sc.box27()
    rho, vel = sc.uniform_fields()
    seeds, sign = sc.both_directions(sc.UNIFORM_SEEDS)
    counts, codes, rec = sl.trace_host(sc.one_level(g, rho, vel), seeds, sign, 0.5, 1e-6, 100)
    sc.check_uniform(counts, codes, rec, seeds, sign)
    assert np.array_equal(rec[:, :, 3][rec[:, :, 3] != 0], np.ones(counts.sum(), F32))        # rho of every used record
    assert rec.dtype == F32 and counts.dtype == codes.dtype == np.int32
    assert (sl.used(counts, rec)[:, 4] == sc.U0).all()


@pytest.mark.parametrize("step, radius, n", sc.ROTATION)
def test_solid_body_rotation_drifts_as_the_midpoint_rule_must(step, radius, n):
    """the analytic bound of the midpoint rule with a unit direction on a linear field; a shared wrong definition (plain Euler: 2 eps^2
    per step, 0.2 cells here) fails it"""
    g = sc.box27()
    rho, vel = sc.rotation_fields()
    seeds, sign = sc.both_directions(sc.rotation_seeds(radius))
    counts, codes, rec = sl.trace_host(sc.one_level(g, rho, vel), seeds, sign, step, 1e-6, n)
    sc.check_rotation(counts, codes, rec, step, radius, n)


def test_planted_states_reach_every_end_code_and_replaced_corners():
    g, rho, vel, seeds, sign = sc.planted()
    info = {}
    lv = sc.one_level(g, rho, vel)
    counts, codes, rec = sl.trace_host(lv, seeds, sign, 0.5, sc.MIN_SPEED, sc.PLANTED_MAX_STEPS, info)
    assert set(codes.tolist()) == {sl.END_STEPS, sl.END_OUTSIDE, sl.END_OBSTACLE, sl.END_SLOW}
    assert info["replaced"] > 0
    n = len(seeds) // 2
    for k in (0, n):                                                        # forward and backward
        assert counts[k + 1: k + 4].tolist() == [0, 0, 0] and codes[k + 1: k + 4].tolist() == [1, 1, 2]
    # a speed equal to min_speed exactly continues: the first vertex carries it, and a second one follows
    assert np.array_equal(rec[0, 0, 4:7], np.array([sc.MIN_SPEED, 0, 0], F32)) and counts[0] >= 2 and counts[n] >= 2
    # the line towards the absent fourth block ends there with code 1, inside block (1, 2, 1)
    assert codes[4] == sl.END_OUTSIDE and counts[4] > 2 and 7.0 < rec[4, counts[4] - 1, 0] < 8.5 and rec[4, counts[4] - 1, 1] > 8.5
    u = sl.used(counts, rec)
    assert np.isnan(u).any() and np.isinf(u).any()                          # the planted NaN and infinity were sampled
    assert (counts <= sc.PLANTED_MAX_STEPS + 1).all() and (counts[codes == sl.END_STEPS] == sc.PLANTED_MAX_STEPS + 1).all()
    # max_steps = 0: one vertex and code 0 wherever the seed can be sampled
    c0, e0, r0 = sl.trace_host(lv, seeds, sign, 0.5, sc.MIN_SPEED, 0)
    ok = counts > 0
    assert np.array_equal(c0, ok.astype(np.int32)) and (e0[ok] == 0).all() and np.array_equal(e0[~ok], codes[~ok])
    assert np.array_equal(r0[:, 0], rec[:, 0], equal_nan=True)


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_tunnel_rake_exercises_the_locator(levels):
    """the inputs of the device test: lines that change level, midpoints on another level than their step's start, lines that end in the
    sphere and at the grid's extent - after 3 and after 4 coarse steps (both velocity buffers of level 1)"""
    from oracle import oracle
    oracle.set_num_threads(min(8, os.cpu_count() or 1))
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    seeds, sign = sc.tunnel_rake()

    class Fields:
        def field(self, li, name):
            return getattr(grids[li], name)
    got, t_done = [], 0
    for t_coarse in (3, 4):
        oracle.execute_timestep_batch(grids, t_done + 1, t_coarse - t_done, F32(0.05), params)
        t_done = t_coarse
        info = {}
        counts, codes, rec = sl.trace_host(sl.stepper_levels(Fields(), grids, t_coarse), seeds, sign, sc.TUNNEL_STEP, sc.TUNNEL_MIN_SPEED,
                                           sc.TUNNEL_MAX_STEPS, info)
        assert ((codes == sl.END_OBSTACLE) & (counts >= 2)).any() and ((codes == sl.END_OUTSIDE) & (counts >= 2)).any()
        if levels > 1:
            assert sl.level_changes(counts, rec).max() >= 2 and info["midpoint_other_level"] >= 1
            assert set(sl.used(counts, rec)[:, 7].tolist()) == set(range(levels))
        got.append(sl.used(counts, rec))
    assert got[0].shape != got[1].shape or not np.array_equal(got[0], got[1], equal_nan=True)


def test_seed_expansion_positions_and_frames():
    pts = sl.expand_group({"name": "a", "line": {"from": [0, 0, 0], "to": [1, 2, -4], "count": 5}})
    assert np.array_equal(pts, np.array([0, 0.25, 0.5, 0.75, 1.0])[:, None] * np.array([1.0, 2.0, -4.0]))
    assert np.array_equal(sl.expand_group({"line": {"from": [1, 2, 3], "to": [9, 9, 9], "count": 1}}), [[1.0, 2.0, 3.0]])
    assert np.array_equal(sl.expand_group({"points": [[1, 2, 3], [4, 5, 6]]}), [[1.0, 2, 3], [4, 5, 6]])
    for bad in ({}, {"points": [[1, 2, 3]], "line": {"from": [0] * 3, "to": [1] * 3, "count": 2}}, {"points": []}, {"points": [[1, 2]]},
                {"line": {"from": [0] * 3, "to": [1] * 3}}, {"line": {"from": [0] * 3, "to": [1] * 3, "count": 0}},
                {"points": [[0, float("nan"), 0]]}):
        with pytest.raises(ValueError, match="seeds"):
            sl.expand_group(bad)
    P = sl.seed_positions([[0.1, 0.2, 0.3]], (1.0, 2.0, 3.0), 0.25)
    assert P.dtype == F32 and np.array_equal(P, np.array([[1.1 / 0.25, 2.2 / 0.25, 3.3 / 0.25]]).astype(F32))
    assert np.array_equal(sl.to_domain(P, 0.25), (P.astype(np.float64) * 0.25).astype(F32))
    plan = sl.SeedPlan([("a", pts), ("b", np.array([[1.0, 1, 1]]))], "both", (0, 0, 0), 0.5)
    assert plan.n_lines == 12 and plan.sign.tolist() == [1.0, -1.0] * 6 and plan.seed_index.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 0, 0]
    assert plan.group.tolist() == [0] * 10 + [1, 1] and np.array_equal(plan.seeds[2], (pts[1] / 0.5).astype(F32))
    assert sl.SeedPlan([("a", pts)], "backward", (0, 0, 0), 0.5).sign.tolist() == [-1.0] * 5
    with pytest.raises(ValueError):
        sl.line_signs("sideways")


SEEDS = [{"name": "a", "points": [[-4.0, 0.1, 0.2]]}]


def _load(stream_cfg):
    return pp.load_case_configuration(CFG, {"advanced": {"streamlines": stream_cfg}})


def test_configuration_defaults_and_parsing():
    for name in ("ball1m_config.yaml", "cube1m_config.yaml", "bunny_config.yaml"):
        cfg = pp.load_case_configuration(os.path.join(G, name))
        assert not cfg.streamlines_enabled and cfg.streamlines_seeds == ()
        assert (cfg.streamlines_start_step, cfg.streamlines_interval, cfg.streamlines_step, cfg.streamlines_max_steps, cfg.streamlines_min_speed,
                cfg.streamlines_direction, cfg.streamlines_max_vertices) == (1, 100, 0.5, 2000, 1.0e-6, "both", 20_000_000)
    assert not _load({"enabled": False, "seeds": [{"name": ""}]}).streamlines_enabled
    cfg = _load({"enabled": True, "start_step": 3, "interval": 7, "step": 0.25, "max_steps": 50, "min_speed": 1e-4, "direction": "forward",
                 "max_vertices": 1000, "seeds": SEEDS + [{"name": "b-1", "line": {"from": [0, 0, 0], "to": [2, 0, 0], "count": 3}}]})
    assert cfg.streamlines_enabled and (cfg.streamlines_start_step, cfg.streamlines_interval, cfg.streamlines_step, cfg.streamlines_max_steps,
                                        cfg.streamlines_min_speed, cfg.streamlines_direction, cfg.streamlines_max_vertices) == \
        (3, 7, 0.25, 50, 1e-4, "forward", 1000)
    a, b = cfg.streamlines_seeds
    assert (a.name, a.points) == ("a", ((-4.0, 0.1, 0.2),)) and (b.name, b.points) == ("b-1", ((0.0, 0, 0), (1.0, 0, 0), (2.0, 0, 0)))
    assert pp.STREAMLINE_DIRECTIONS == sl.DIRECTIONS
    _load({"enabled": True, "max_steps": 9, "max_vertices": 20, "seeds": SEEDS})             # 2 lines x 10 vertices: exactly the cap


@pytest.mark.parametrize("stream_cfg, key", [
    ({"enabled": True, "seeds": []}, "advanced.streamlines.seeds"),
    ({"enabled": True, "seeds": [{"points": [[0, 0, 0]]}]}, "advanced.streamlines.seeds[0].name"),
    ({"enabled": True, "seeds": SEEDS + SEEDS}, "advanced.streamlines.seeds[1].name"),
    ({"enabled": True, "seeds": [{"name": "a"}]}, "advanced.streamlines.seeds[0]"),
    ({"enabled": True, "seeds": [{"name": "a", "points": [[0, 0]]}]}, "advanced.streamlines.seeds[0].points"),
    ({"enabled": True, "seeds": [{"name": "a", "line": {"from": [0, 0, 0], "to": [1, 1, 1], "count": 0}}]}, "advanced.streamlines.seeds[0].line.count"),
    ({"enabled": True, "interval": 0, "seeds": SEEDS}, "advanced.streamlines.interval"),
    ({"enabled": True, "start_step": 0, "seeds": SEEDS}, "advanced.streamlines.start_step"),
    ({"enabled": True, "step": 0.0, "seeds": SEEDS}, "advanced.streamlines.step"),
    ({"enabled": True, "step": float("nan"), "seeds": SEEDS}, "advanced.streamlines.step"),
    ({"enabled": True, "min_speed": -1.0, "seeds": SEEDS}, "advanced.streamlines.min_speed"),
    ({"enabled": True, "max_steps": -1, "seeds": SEEDS}, "advanced.streamlines.max_steps"),
    ({"enabled": True, "direction": "up", "seeds": SEEDS}, "advanced.streamlines.direction"),
    ({"enabled": True, "max_vertices": 0, "seeds": SEEDS}, "advanced.streamlines.max_vertices"),
    ({"enabled": True, "max_steps": 9, "max_vertices": 19, "seeds": SEEDS}, "advanced.streamlines.max_vertices"),
    ({"enabled": True, "seeds": [{"name": "r", "line": {"from": [0, 0, 0], "to": [1, 1, 1], "count": 5000}}]}, "advanced.streamlines.max_vertices"),
])
def test_configuration_errors_name_their_key(stream_cfg, key):
    with pytest.raises(ValueError) as e:
        _load(stream_cfg)
    assert key in str(e.value), str(e.value)


def test_write_vtp_lines_round_trip(tmp_path):
    g, rho, vel, seeds, sign = sc.planted()
    counts, codes, rec = sl.trace_host(sc.one_level(g, rho, vel), seeds, sign, 0.5, sc.MIN_SPEED, sc.PLANTED_MAX_STEPS)
    n = len(seeds)
    plan = sl.SeedPlan([("all", np.zeros((n, 3)))], "forward", (0, 0, 0), 0.25)
    plan.seeds, plan.sign = seeds, sign
    ln = sl.group_lines(plan, 0, counts, codes, rec)
    keep = np.flatnonzero(counts >= 2)
    assert ln.n_short == n - keep.size > 0 and ln.offsets.tolist() == np.cumsum(counts[keep]).tolist()
    for compress in (True, False):
        path = output.write_vtp_lines(str(tmp_path / f"s{int(compress)}"), ln.points, ln.offsets, ln.rho, ln.vel, ln.level, ln.seed,
                                      ln.direction, ln.end_code, compress)
        assert path.endswith(".vtp") and not os.path.exists(path + ".part")
        text = open(path).read()
        assert 'type="PolyData"' in text and "<Lines>" in text and ("vtkZLibDataCompressor" in text) == compress
        arr = sl.read_vtp(path)
        assert int(arr["NumberOfLines"]) == keep.size and int(arr["NumberOfPolys"]) == 0 and int(arr["NumberOfPoints"]) == counts[keep].sum()
        u = np.concatenate([rec[i, : counts[i]] for i in keep])
        assert np.array_equal(arr["Points"], sl.to_domain(u[:, 0:3], 0.25)) and arr["Points"].dtype == F32
        assert np.array_equal(arr["connectivity"], np.arange(len(u))) and np.array_equal(arr["offsets"], ln.offsets)
        assert np.array_equal(arr["Density"], u[:, 3], equal_nan=True) and np.array_equal(arr["Velocity"], u[:, 4:7], equal_nan=True)
        assert np.array_equal(arr["Level"], np.ones(len(u), np.int32)) and arr["Level"].dtype == np.int32
        assert np.array_equal(arr["Seed"], plan.seed_index[keep]) and np.array_equal(arr["Direction"], sign[keep].astype(np.int32))
        assert np.array_equal(arr["EndCode"], codes[keep]) and set(arr["Direction"].tolist()) == {1, -1}
    # no line at all is a valid file
    none = sl.group_lines(plan, 0, np.zeros(n, np.int32), np.ones(n, np.int32), rec)
    arr = sl.read_vtp(output.write_vtp_lines(str(tmp_path / "empty"), none.points, none.offsets, none.rho, none.vel, none.level, none.seed,
                                             none.direction, none.end_code))
    assert int(arr["NumberOfLines"]) == 0 and arr["Points"].size == 0 and none.n_short == n


STREAM_CFG = {"enabled": True, "start_step": 2, "interval": 3, "step": 0.5, "max_steps": 60, "min_speed": 1e-7, "direction": "both",
              "seeds": [{"name": "rake", "line": {"from": [-4.0, -1.5, -0.2], "to": [-4.0, 1.5, 0.3], "count": 5}},
                        {"name": "pts", "points": [[-2.0, 0.3, 0.1], [0.0, 0.0, 0.0], [1.0e3, 0.0, 0.0]]}]}


def test_run_case_with_a_stepper_without_streamlines_traces_on_the_host(tmp_path):
    """the CPU oracle behind run_case: files at the sampled steps from trace_host, every other file unchanged"""
    from _steppers import OracleStepper
    from oracle import oracle
    oracle.set_num_threads(min(8, os.cpu_count() or 1))
    base = {"basic": {"num_levels": 1, "surface_resolution": 7, "simulation": {"steps": 6, "output_freq": 8, "ramp_steps": 4}},
            "advanced": {"boundary": {"method": "bounce_back"}, "high_re": {"wall_model": {"enabled": False}},
                         "numerics": {"c_wale": 0.0, "nu_sgs_background": 0.0}, "diagnostics": {"freq": 4}}}
    outs, lines = {}, []
    for on in (False, True):
        over = copy.deepcopy(base)
        if on:
            over["advanced"]["streamlines"] = STREAM_CFG
        cfg = pp.load_case_configuration(CFG, over)
        outs[on] = str(tmp_path / ("on" if on else "off"))
        case.run_case(cfg, OracleStepper, stl_path=os.path.join(G, "cube1m.stl"), out_dir=outs[on], log=lines.append)
    new = [f"stream_{n}_{t:06d}.vtp" for n in ("rake", "pts") for t in (2, 5)] + ["stream_rake.pvd", "stream_pts.pvd"]
    assert sorted(os.listdir(outs[True])) == sorted(os.listdir(outs[False]) + new)
    for name in os.listdir(outs[False]):
        if name != "convergence.csv":
            assert filecmp.cmp(os.path.join(outs[False], name), os.path.join(outs[True], name), shallow=False), name
    from open_ludwig_amd.slices import read_pvd
    assert [f for _, f in read_pvd(os.path.join(outs[True], "stream_rake.pvd"))] == ["stream_rake_000002.vtp", "stream_rake_000005.vtp"]
    rake = sl.read_vtp(os.path.join(outs[True], "stream_rake_000005.vtp"))
    assert int(rake["NumberOfLines"]) > 0 and set(rake["Level"].tolist()) == {1} and set(rake["Seed"].tolist()) <= set(range(5))
    pts = sl.read_vtp(os.path.join(outs[True], "stream_pts_000005.vtp"))
    logged = [l for l in lines if l.startswith("streamlines 'pts': step 5")]
    assert len(logged) == 1 and "6 lines" in logged[0] and "fewer than 2 vertices" in logged[0]


def test_distributed_stepper_refuses_and_names_the_key():
    st = object.__new__(case.DistributedStepper)                           # the refusal needs no device and no process group
    with pytest.raises(RuntimeError, match=r"advanced\.streamlines"):
        st.streamlines_setup(None, None)
    cfg = pp.load_case_configuration(CFG, {"basic": {"num_levels": 1, "surface_resolution": 7},
                                           "advanced": {"streamlines": {"enabled": True, "seeds": SEEDS}}})
    closed = []

    class Refusing:
        def __init__(self, grids):
            pass

        streamlines_setup = case.DistributedStepper.streamlines_setup

        def close(self):
            closed.append(True)
    with pytest.raises(RuntimeError, match=r"advanced\.streamlines"):
        case.run_case(cfg, Refusing, stl_path=os.path.join(G, "cube1m.stl"), steps=1)
    assert closed == [True]


def test_header_exports_and_julia_list_the_streamline_calls():
    new = ["ludwig_streamlines_create", "ludwig_streamlines_destroy", "ludwig_streamlines_trace", "ludwig_streamlines_download"]
    header = open(os.path.join(ROOT, "include", "ludwig_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "LudwigHIP.jl")).read()
    lib = _lib.load()
    for name in new:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert f"(:{name}, LIB)" in jl, name
    assert lib.ludwig_abi_version() == 1
    for name, k in (("STEPS", sl.END_STEPS), ("OUTSIDE", sl.END_OUTSIDE), ("OBSTACLE", sl.END_OBSTACLE), ("SLOW", sl.END_SLOW)):
        assert re.search(r"LUDWIG_STREAM_END_" + name + r"\s*=\s*%d\b" % k, header), name


def test_calls_reject_bad_arguments_without_a_device():
    import ctypes as C
    lib = _lib.load()
    out = C.c_void_p(1)
    assert lib.ludwig_streamlines_create(None, 1, 0, None, None, 0.5, 1e-6, 10, C.byref(out)) == -1 and out.value is None
    assert lib.ludwig_streamlines_create(None, 1, 0, None, None, 0.5, 1e-6, 10, None) == -1
    assert lib.ludwig_streamlines_trace(None, 1) == -1
    assert lib.ludwig_streamlines_download(None, None, None, None, 0) == -1
    assert b"null" in lib.ludwig_last_error()
    lib.ludwig_streamlines_destroy(None)
