"""Probes without a GPU: the advanced.probes keys, the host planner (level, stencil, corner replacement, weights), the float32
restatement of the device interpolation, the C entry points' argument checks, and run_case's probes.csv / probes_points.csv with the
CPU oracle stepping."""
import ctypes as C
import filecmp
import os
import re
import sys

import numpy as np
import pytest

from open_ludwig_amd import _lib, case, cases, preprocess as pp, probes as pm
from open_ludwig_amd.statistics import t_sub_after

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
F32 = np.float32
RE266K = {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}, "simulation": {"steps": 6000, "output_freq": 1000}}}


def _probes_cfg(**kw):
    return {"advanced": {"probes": dict({"enabled": True}, **kw)}}


# ---- configuration ----
def test_shipped_configs_parse_with_probes_off():
    for name in ("ball1m_config.yaml", "cube1m_config.yaml", "bunny_config.yaml"):
        cfg = pp.load_case_configuration(os.path.join(G, name))
        assert not cfg.probes_enabled and cfg.probes_points == () and cfg.probes_names == ()


def test_probe_keys_parse_and_validate():
    p = os.path.join(G, "ball1m_config.yaml")
    cfg = pp.load_case_configuration(p, _probes_cfg(start_step=5, interval=3, points=[[1, 0, 0], [1.5, 0.1, -0.2]], names=["a", "b"]))
    assert cfg.probes_enabled and (cfg.probes_start_step, cfg.probes_interval) == (5, 3)
    assert cfg.probes_points == ((1.0, 0.0, 0.0), (1.5, 0.1, -0.2)) and cfg.probes_names == ("a", "b")
    d = pp.load_case_configuration(p, _probes_cfg(points=[[1, 0, 0], [2, 0, 0]]))
    assert (d.probes_start_step, d.probes_interval, d.probes_names) == (1, 1, ("p0", "p1"))
    off = pp.load_case_configuration(p, {"advanced": {"probes": {"enabled": False, "interval": 0, "points": [[1, 2]]}}})
    assert not off.probes_enabled and off.probes_points == ()
    bad = [dict(interval=0, points=[[1, 0, 0]]), dict(interval=-2, points=[[1, 0, 0]]), dict(start_step=0, points=[[1, 0, 0]]),
           dict(points=[]), dict(points=[[1, 0]]), dict(points=[[1, 0, float("nan")]]), dict(points=[[1, 0, 0]], names=["a", "b"]),
           dict(points=[[1, 0, 0], [2, 0, 0]], names=["a", "a"]), dict(points=[[1, 0, 0]], names=["a,b"])]
    for b in bad:
        with pytest.raises(ValueError):
            pp.load_case_configuration(p, _probes_cfg(**b))


# ---- planner ----
def _tunnel3():
    return cases.tunnel_with_sphere(levels=3, wall_model=True)


def test_planner_refuses_points_outside_the_domain_and_inside_the_body():
    grids, _ = _tunnel3()
    for q in ([-0.1, 5, 5], [48.01, 5, 5], [5, 32.5, 5], [5, 5, -3]):
        with pytest.raises(ValueError, match="'far'.*outside the domain"):
            pm.plan_probes([[5, 5, 5], q], grids, names=["ok", "far"])
    with pytest.raises(ValueError, match="'low'.*base cell lies outside"):                # within half a coarse cell of a low face
        pm.plan_probes([[0.2, 5, 5]], grids, names=["low"])
    with pytest.raises(ValueError, match="'core'.*obstacle"):
        pm.plan_probes([[19.3, 16.1, 16.1]], grids, names=["core"])                      # the sphere's centre (19.2, 16, 16)
    with pytest.raises(ValueError, match="'in'.*outside"):                                # the offset is applied
        pm.plan_probes([[5, 5, 5]], grids, offset=(50.0, 0.0, 0.0), names=["in"])


def _check_stencil(plan, grids, p):
    """every corner is the cell i0 + d of the probe's level where that is a fluid cell of an active block, else the base cell"""
    g = grids[int(plan.level[p])]
    gg = plan.domain[p] / g.dx - 0.5
    i0 = np.floor(gg).astype(int)
    assert np.array_equal(plan.weights[p], (gg - i0).astype(F32))
    base = pm._cell(g, i0)
    for c in range(8):
        want = pm._cell(g, i0 + np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1]))
        fluid = want is not None and not g.obstacle[want[1], want[2], want[3], want[0]]
        got = (int(plan.blocks[p, c]), int(plan.cells[p, c]))
        use = want if fluid else base
        assert got == (use[0], use[1] + 8 * use[2] + 64 * use[3]), (p, c)
        assert plan.replaced[p, c] == (not fluid)


def _wall_point(grids, level, y, z, xs, offset=(0.0, 0.0, 0.0)):
    """the first x along the line whose plan puts the probe on `level` with an obstacle corner replaced"""
    for x in xs:
        try:
            pl = pm.plan_probes([[x, y, z]], grids, offset)
        except ValueError:
            continue
        if pl.level[0] == level and pl.replaced[0].any():
            return x
    raise AssertionError("no wall point found")


def test_planner_level_choice_and_corner_replacement_on_the_tunnel():
    grids, _ = _tunnel3()
    # level 3 spans cells 48..111 (x 12..28 at dx 0.25), level 2 blocks 3..8 (x 8..32 at dx 0.5), level 1 the box 48 x 32 x 32
    x_wall = _wall_point(grids, 2, 16.05, 16.05, np.arange(12.3, 16.0, 0.05))
    pts = [[27.1, 16.1, 16.2],          # level 3 interior, fluid
           [27.95, 15.1, 14.2],         # level 3, last cell before its +x edge: the +x corners are replaced
           [10.3, 20.1, 20.2],          # level 2 only
           [47.9, 2.1, 2.2],            # level 1 at the domain's +x face
           [3.1, 31.8, 31.9],           # level 1 at the +y / +z faces
           [x_wall, 16.05, 16.05]]      # level 3 next to the sphere
    plan = pm.plan_probes(pts, grids)
    assert plan.level.tolist() == [2, 2, 1, 0, 0, 2]
    assert not plan.replaced[0].any() and not plan.replaced[2].any()
    assert plan.replaced[1].tolist() == [False, True, False, True, False, True, False, True]
    assert plan.replaced[3].tolist() == [False, True, False, True, False, True, False, True]
    assert plan.replaced[4].tolist() == [False, False, True, True, True, True, True, True]
    assert plan.replaced[5].any() and not plan.replaced[5].all()
    for p in range(plan.n):
        _check_stencil(plan, grids, p)
    assert plan.blocks.dtype == np.int32 and plan.cells.dtype == np.int32 and plan.weights.dtype == np.float32
    assert ((plan.weights >= 0) & (plan.weights < 1)).all()


@pytest.fixture(scope="module")
def ball():
    cfg = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), RE266K)
    return cfg, pp.setup_multilevel_domain(cfg, os.path.join(G, "ball1m.stl"))


def test_planner_on_ball1m(ball):
    _, (grids, mesh, params, _) = ball
    off = params.mesh_offset
    # the sphere has radius 0.5 about the STL origin: wake, next to the wall, upstream on level 1, level 2
    x_wall = _wall_point(grids, 2, 0.013, 0.011, np.arange(-0.6, -0.45, 0.004), off)
    pts = [[1.0, 0.05, -0.03], [1.6, 0.2, 0.1], [x_wall, 0.013, 0.011], [-3.5, 0.0, 0.0], [-2.6, 0.0, 0.0]]
    plan = pm.plan_probes(pts, grids, off)
    assert np.array_equal(plan.domain, np.asarray(pts) + off)
    assert plan.level.tolist()[:4] == [2, 2, 2, 0]
    assert plan.level[4] == 1
    for p in range(plan.n):
        _check_stencil(plan, grids, p)
    with pytest.raises(ValueError, match="'inside'.*obstacle"):
        pm.plan_probes([[0.0, 0.0, 0.0]], grids, off, names=["inside"])
    with pytest.raises(ValueError, match="'away'.*outside the domain"):
        pm.plan_probes([[7.0, 0.0, 0.0]], grids, off, names=["away"])


def test_ball1m_refinement_edge_replaces_the_outer_corners(ball):
    _, (grids, _, params, _) = ball
    g = grids[2]
    hi = (max(c[0] for c in g.active_block_coords)) * 8          # cells of level 3 end at hi - 1 along x
    x = (hi - 1 + 0.5 + 0.4) * g.dx - params.mesh_offset[0]       # base cell = the last one, w = 0.4
    plan = pm.plan_probes([[x, 0.01, 0.02]], grids, params.mesh_offset)
    assert plan.level[0] == 2 and plan.replaced[0].tolist() == [False, True] * 4
    _check_stencil(plan, grids, 0)


# ---- interpolation ----
def test_trilinear_order_is_x_then_y_then_z():
    r = np.random.default_rng(3)
    v = r.standard_normal((1000, 8)).astype(F32)
    w = r.random((1000, 3)).astype(F32)
    one = F32(1)
    L = lambda a, b, t: (one - t) * a + t * b
    x = [L(v[:, 2 * i], v[:, 2 * i + 1], w[:, 0]) for i in range(4)]
    want = L(L(x[0], x[1], w[:, 1]), L(x[2], x[3], w[:, 1]), w[:, 2])
    got = pm.trilinear(v, w)
    assert got.dtype == F32 and np.array_equal(got, want)
    assert np.array_equal(pm.trilinear(v, np.zeros((1000, 3), F32)), v[:, 0])
    assert np.array_equal(pm.trilinear(v, np.ones((1000, 3), F32)), v[:, 7])


def test_linear_field_is_reproduced_at_interior_probes():
    grids, _ = _tunnel3()
    r = np.random.default_rng(11)
    pts = np.column_stack([r.uniform(1, 46, 300), r.uniform(1, 31, 300), r.uniform(1, 31, 300)])
    ok = []
    for q in pts:
        try:
            pm.plan_probes([q], grids)
            ok.append(q)
        except ValueError:
            pass
    plan = pm.plan_probes(ok, grids)
    interior = ~plan.replaced.any(axis=1)
    assert interior.sum() > 100 and set(plan.level[interior].tolist()) == {0, 1, 2}
    a = np.array([1.0, 0.01, -0.02, 0.005])
    b = np.array([[0.001, -0.0005, 0.0002], [0.002, 0.001, 0.0], [-0.001, 0.0015, 0.0007], [0.0, 0.0003, -0.002]])

    def fields(li):
        g = grids[li]
        c = [(x - 0.5) * g.dx for x in cases.global_cell_coords(g)]                     # cell centres, domain frame
        lin = [(a[k] + b[k, 0] * c[0] + b[k, 1] * c[1] + b[k, 2] * c[2]).astype(F32) for k in range(4)]
        return np.asfortranarray(lin[0]), np.asfortranarray(np.stack(lin[1:], axis=-1))
    got = pm.sample_fields(plan, fields)
    exact = a[None, :] + plan.domain @ b.T
    err = np.abs(got[interior] - exact[interior]) / np.maximum(np.abs(exact[interior]), 1e-3)
    assert err.max() < 2e-6, err.max()


# ---- C ABI ----
def test_header_exports_and_julia_list_the_probe_calls():
    new = ["ludwig_probes_create", "ludwig_probes_destroy", "ludwig_probes_sample", "ludwig_probes_download",
           "ludwig_execute_timestep_batch_probes"]
    header = open(os.path.join(ROOT, "include", "ludwig_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "LudwigHIP.jl")).read()
    lib = _lib.load()
    for name in new:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        # the binding reaches an in-batch observer through the observed batch call, as an entry of the observer's kind
        called = "ludwig_execute_timestep_batch_observed" if name.startswith("ludwig_execute_timestep_batch_") else name
        assert f"(:{called}, LIB)" in jl, name
    assert "entry(OBSERVE_PROBES, probes, start_step, interval)" in jl
    assert lib.ludwig_abi_version() == 1


def test_probe_calls_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    one = np.zeros(8, np.int32)
    w = np.zeros(3, np.float32)
    li = np.zeros(1, np.int32)
    out = C.c_void_p()
    nulls = (C.c_void_p * 1)(None)
    assert lib.ludwig_probes_create(None, 1, 1, li.ctypes.data, one.ctypes.data, one.ctypes.data, w.ctypes.data, 4, C.byref(out)) == -1
    assert lib.ludwig_probes_create(nulls, 1, 1, li.ctypes.data, one.ctypes.data, one.ctypes.data, w.ctypes.data, 4, None) == -1
    assert lib.ludwig_probes_create(nulls, 1, 1, li.ctypes.data, one.ctypes.data, one.ctypes.data, w.ctypes.data, 4, C.byref(out)) == -1
    assert "null" in lib.ludwig_last_error().decode() and not out.value
    for n_levels, n_probes, cap in ((0, 1, 4), (1, 0, 4), (1, 1, 0)):
        assert lib.ludwig_probes_create(nulls, n_levels, n_probes, li.ctypes.data, one.ctypes.data, one.ctypes.data, w.ctypes.data, cap,
                                        C.byref(out)) == -1
    assert lib.ludwig_probes_sample(None, 0, 0) == -1
    n = C.c_int32(0)
    v = np.zeros(16, np.float32)
    s = np.zeros(1, np.int64)
    assert lib.ludwig_probes_download(None, v.ctypes.data, s.ctypes.data, 1, C.byref(n)) == -1
    lib.ludwig_probes_destroy(None)
    fl = _lib.StepFlags()
    assert lib.ludwig_execute_timestep_batch_probes(None, 1, 1, 1, 0.0, C.byref(fl), None, 1, 1) == -1
    assert lib.ludwig_execute_timestep_batch_probes(nulls, 1, 1, 1, 0.0, C.byref(fl), None, 1, 1) == -1
    assert lib.ludwig_execute_timestep_batch_probes(nulls, 1, 1, 1, 0.0, None, None, 1, 1) == -1


# ---- run_case with the CPU oracle ----
CUBE = {"basic": {"num_levels": 1, "surface_resolution": 7, "simulation": {"steps": 10, "output_freq": 8}},
        "advanced": {"boundary": {"method": "bounce_back"}, "high_re": {"wall_model": {"enabled": False}},
                     "numerics": {"c_wale": 0.0, "nu_sgs_background": 0.0}, "diagnostics": {"freq": 4}}}


class ProbeOracleStepper:
    """the CPU oracle with probes sampled from its host arrays through the numpy restatement (what a device stepper's
    probes_series returns)"""

    def __init__(self, grids):
        from _steppers import OracleStepper
        self.inner = OracleStepper(grids)
        self.grids = grids
        self.field = self.inner.field
        self.plan = None
        self.steps, self.vals = [], []

    def probes_setup(self, plan, start_step, interval, capacity):
        self.plan, self.start, self.interval = plan, start_step, interval

    def batch(self, t_start, n, u_curr, params):
        for t in range(t_start, t_start + n):
            self.inner.batch(t, 1, u_curr, params)
            if self.plan is not None and pm.is_sample_step(t, self.start, self.interval):
                self.steps.append(t)
                self.vals.append(pm.sample_fields(self.plan, lambda li: (self.grids[li].rho, getattr(
                    self.grids[li], "vel_temp" if t_sub_after(li, t) % 2 == 0 else "vel"))))

    def probes_series(self):
        return np.array(self.steps, np.int64), (np.stack(self.vals) if self.vals else np.zeros((0, self.plan.n, 4), F32))

    def close(self):
        pass


def test_run_case_writes_probe_files_and_leaves_the_rest_unchanged(tmp_path):
    from oracle import oracle
    oracle.set_num_threads(min(8, os.cpu_count() or 1))
    stl = os.path.join(G, "cube1m.stl")
    pts = [[1.3, 0.1, -0.05], [0.9, 0.05, 0.2], [-2.0, 1.0, 1.0], [2.5, -0.3, 0.4]]
    runs = {}
    for on in (False, True):
        over = {**CUBE, "advanced": {**CUBE["advanced"], "probes": {"enabled": on, "start_step": 2, "interval": 3, "points": pts,
                                                                    "names": ["wake", "top", "up", "side"]}}}
        cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), over)
        setup = pp.setup_multilevel_domain(cfg, stl)
        out = os.path.join(tmp_path, "on" if on else "off")
        holder = {}

        def factory(grids):
            holder["st"] = ProbeOracleStepper(grids)
            return holder["st"]
        case.run_case(cfg, factory, setup=setup, out_dir=out)
        runs[on] = (out, holder["st"], setup)
    off, on = runs[False][0], runs[True][0]
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + ["probes.csv", "probes_points.csv"])
    for name in os.listdir(off):
        if name != "convergence.csv":                                       # wall time and MLUPS columns
            assert filecmp.cmp(os.path.join(off, name), os.path.join(on, name), shallow=False), name
    st, (grids, _, params, _) = runs[True][1], runs[True][2]
    head, steps, vals = pm.read_series_csv(os.path.join(on, "probes.csv"))
    assert head[:6] == ["step", "time", "wake_rho", "wake_ux", "wake_uy", "wake_uz"] and len(head) == 2 + 4 * 4
    assert steps.tolist() == [2, 5, 8]
    s_steps, s_vals = st.probes_series()
    assert np.array_equal(steps, s_steps)
    assert np.array_equal(vals.view(np.uint32), s_vals.view(np.uint32))               # bit for bit through the text
    assert np.isfinite(vals).all() and np.abs(vals[:, :, 0] - 1).max() < 0.1
    rows = [l.strip().split(",") for l in open(os.path.join(on, "probes.csv")).readlines()[1:]]
    assert [r[1] for r in rows] == ["%.6e" % (s * params.time_scale) for s in (2, 5, 8)]
    pts_rows = [l.strip().split(",") for l in open(os.path.join(on, "probes_points.csv"))]
    assert pts_rows[0] == ["name", "x", "y", "z", "x_domain", "y_domain", "z_domain", "level"]
    assert [r[0] for r in pts_rows[1:]] == ["wake", "top", "up", "side"]
    for r, q in zip(pts_rows[1:], pts):
        assert [float(v) for v in r[1:4]] == [float(v) for v in q]
        assert np.array_equal(np.array([float(v) for v in r[4:7]]), np.asarray(q, float) + params.mesh_offset)
        assert r[7] == "1"
