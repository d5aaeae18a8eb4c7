"""Slices without a GPU: the advanced.slices keys, the vectorised planner against plan_probes, the float32 restatement, the VTI / PVD
writers read back, the C entry points' argument checks, and run_case's slice files with the CPU oracle stepping."""
import ctypes as C
import filecmp
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import _lib, case, cases, preprocess as pp, probes as pm, slices as sl
from open_ludwig_amd.statistics import t_sub_after

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
F32 = np.float32
BALL = os.path.join(G, "ball1m_config.yaml")


def _cfg(**kw):
    return {"advanced": {"slices": dict({"enabled": True}, **kw)}}


def _plane(**kw):
    return dict({"name": "mid", "normal": "y", "position": 0.0}, **kw)


# ---- configuration ----
def test_shipped_configs_parse_with_slices_off():
    for name in ("ball1m_config.yaml", "cube1m_config.yaml", "bunny_config.yaml"):
        cfg = pp.load_case_configuration(os.path.join(G, name))
        assert not cfg.slices_enabled and cfg.slices_planes == ()


def test_slice_keys_parse():
    cfg = pp.load_case_configuration(BALL, _cfg(start_step=5, interval=3, planes=[
        _plane(name="wake_y0", bounds=[[-0.5, 2.0], [-0.4, 0.6]], spacing=0.002, fields=["q_criterion", "density", "vorticity"]),
        _plane(name="z1", normal="Z", position=0.25)]))
    assert cfg.slices_enabled and (cfg.slices_start_step, cfg.slices_interval) == (5, 3)
    a, b = cfg.slices_planes
    assert (a.name, a.normal, a.position, a.bounds, a.spacing) == ("wake_y0", 1, 0.0, ((-0.5, 2.0), (-0.4, 0.6)), 0.002)
    assert a.fields == ("density", "vorticity", "q_criterion")                  # SLICE_FIELDS order
    assert (b.normal, b.bounds, b.spacing, b.fields) == (2, None, None, ("density", "velocity", "velocity_magnitude"))
    d = pp.load_case_configuration(BALL, _cfg(planes=[_plane()]))
    assert (d.slices_start_step, d.slices_interval) == (1, 1)
    off = pp.load_case_configuration(BALL, {"advanced": {"slices": {"enabled": False, "interval": 0, "planes": [{"normal": "w"}]}}})
    assert not off.slices_enabled and off.slices_planes == ()


@pytest.mark.parametrize("bad,match", [
    (dict(interval=0, planes=[_plane()]), "interval"),
    (dict(start_step=0, planes=[_plane()]), "start_step"),
    (dict(planes=[]), "at least one plane"),
    (dict(planes=[_plane(normal="w")]), "normal"),
    (dict(planes=[_plane(fields=["density", "pressure"])]), "pressure"),
    (dict(planes=[_plane(spacing=0.0)]), "spacing"),
    (dict(planes=[_plane(spacing=-1e-3)]), "spacing"),
    (dict(planes=[_plane(bounds=[[1.0, -1.0], [0.0, 1.0]])]), "bounds"),
    (dict(planes=[_plane(bounds=[[0.0, float("nan")], [0.0, 1.0]])]), "bounds"),
    (dict(planes=[_plane(bounds=[[0.0, float("inf")], [0.0, 1.0]])]), "bounds"),
    (dict(planes=[_plane(), _plane()]), "unique"),
    (dict(planes=[_plane(name="a/b")]), "file-name"),
    (dict(planes=[_plane(bounds=[[0.0, 10.0], [0.0, 10.0]], spacing=1e-3)]), "points, more than"),
])
def test_slice_keys_refuse_malformed_entries(bad, match):
    with pytest.raises(ValueError, match=match):
        pp.load_case_configuration(BALL, _cfg(**bad))


# ---- planner ----
def _tunnel3():
    return cases.tunnel_with_sphere(levels=3, wall_model=True)


def test_planner_equals_plan_probes_bit_for_bit_across_the_sphere_and_three_levels():
    grids, _ = _tunnel3()
    spec = pp.SlicePlane("s", 2, 16.05, ((0.1, 47.9), (0.3, 31.7)), 0.137)    # through the sphere's centre (19.2, 16, 16)
    off = (0.25, -0.125, 0.0)
    plan = sl.plan_slice(spec, grids, off)
    assert plan.dims == (int(np.floor((47.9 - 0.1) / 0.137)) + 1, int(np.floor((31.7 - 0.3) / 0.137)) + 1)
    assert set(plan.level[plan.valid].tolist()) == {0, 1, 2} and plan.replaced[plan.valid].any() and not plan.valid.all()
    i, j = 17, 33
    p = i + plan.dims[0] * j
    assert plan.points[p].tolist() == [0.1 + i * 0.137, 0.3 + j * 0.137, 16.05]
    assert np.array_equal(plan.domain, plan.points + np.array(off))
    idx = np.flatnonzero(plan.valid)
    ref = pm.plan_probes(plan.points[idx], grids, off)
    for name in ("level", "blocks", "cells", "weights", "replaced"):
        assert np.array_equal(getattr(plan, name)[idx], getattr(ref, name)), name
    assert np.array_equal(plan.domain[idx], ref.domain)
    inside_body = 0
    for q in plan.points[~plan.valid]:
        with pytest.raises(ValueError) as e:
            pm.plan_probes([q], grids, off)
        inside_body += "obstacle" in str(e.value)
    assert inside_body > 0
    for a in ("level", "blocks", "cells", "weights"):
        assert not getattr(plan, a)[~plan.valid].any()


def test_planner_defaults_and_refusals():
    grids, _ = _tunnel3()
    plan = sl.plan_slice(pp.SlicePlane("d", 0, 30.0), grids, (-1.0, 0.0, 0.0))
    h = grids[-1].dx
    ext = np.array([grids[0].grid_dim_y, grids[0].grid_dim_z]) * 8 * grids[0].dx
    assert plan.spacing == h and plan.axes == (1, 2)
    assert plan.dims == tuple(int(np.floor(e / h)) + 1 for e in ext)
    assert plan.origin.tolist() == [29.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="outside the domain"):
        sl.plan_slice(pp.SlicePlane("o", 0, 50.0), grids)
    with pytest.raises(ValueError, match="miss the domain"):
        sl.plan_slice(pp.SlicePlane("o", 2, 5.0, ((50.0, 60.0), (0.0, 5.0)), 1.0), grids)
    with pytest.raises(ValueError, match="more than"):
        sl.plan_slice(pp.SlicePlane("o", 2, 5.0, None, 0.004), grids)


# ---- restatement ----
def _fields(grids, t):
    from _gradient_ref import gradient_fields

    def f(li):
        g = grids[li]
        vel = getattr(g, "vel_temp" if t_sub_after(li, t) % 2 == 0 else "vel")
        w, q = gradient_fields(vel, g.neighbor_table, g.obstacle, F32(1.0 / g.dx))
        return g.rho, vel, w, q
    return f


def test_restatement_equals_probes_and_the_gradient_fields_at_the_stencil():
    grids, _ = _tunnel3()
    rng = np.random.default_rng(3)
    for g in grids:
        g.rho[...] = 1 + 0.01 * rng.standard_normal(g.rho.shape).astype(F32)
        g.vel[...] = 0.05 * rng.standard_normal(g.vel.shape).astype(F32)
    spec = pp.SlicePlane("s", 1, 16.3, ((8.0, 30.0), (9.0, 23.0)), 0.31, pp.SLICE_FIELDS)
    plan = sl.plan_slice(spec, grids)
    t = 1                                                               # odd: `vel` on every level
    got = sl.sample_slice(plan, _fields(grids, t))
    assert got.shape == (9, plan.n) and not got[:, ~plan.valid].any()
    idx = np.flatnonzero(plan.valid)
    probe = pm.sample_fields(pm.plan_probes(plan.points[idx], grids), lambda li: (grids[li].rho, grids[li].vel))
    assert np.array_equal(got[0:4, idx].T.view(np.uint32), probe.view(np.uint32))
    u = probe[:, 1:4]
    assert np.array_equal(got[4, idx], np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]))
    # a point with weights 0 is its base cell's gradient value
    f = _fields(grids, t)
    p = idx[0]
    li = int(plan.level[p])
    _, _, w, q = f(li)
    c, b = int(plan.cells[p, 0]), int(plan.blocks[p, 0])
    zero = sl.SlicePlan(**{**plan.__dict__, "weights": np.zeros_like(plan.weights)})
    got0 = sl.sample_slice(zero, f)
    assert got0[5:8, p].tolist() == w[c % 8, (c // 8) % 8, c // 64, b].tolist() and got0[8, p] == q[c % 8, (c // 8) % 8, c // 64, b]
    assert np.abs(got[5:9, idx]).max() > 0


# ---- files ----
def test_vti_and_pvd_read_back(tmp_path):
    grids, _ = _tunnel3()
    spec = pp.SlicePlane("wake", 1, 16.3, ((8.0, 30.0), (9.0, 23.0)), 0.5, ("density", "velocity", "velocity_magnitude", "q_criterion"))
    plan = sl.plan_slice(spec, grids, (1.0, 2.0, 3.0))
    vals = np.random.default_rng(1).standard_normal((9, plan.n)).astype(F32)
    vals[:, ~plan.valid] = 0
    w = sl.SliceWriter(str(tmp_path), [plan], 0.25)
    w.write(4, [vals])
    w.write(8, [vals * 2])
    attrs, arr = sl.read_vti(os.path.join(tmp_path, "slice_wake_000008.vti"))
    na, nb = plan.dims
    assert attrs["WholeExtent"] == f"0 {na - 1} 0 0 0 {nb - 1}"
    assert [float(v) for v in attrs["Origin"].split()] == [9.0, 16.3 + 2.0, 12.0]
    assert [float(v) for v in attrs["Spacing"].split()] == [0.5] * 3
    assert list(arr) == ["Density", "Velocity", "VelocityMagnitude", "QCriterion", "Valid"]
    assert arr["Velocity"].dtype == np.float32 and arr["Velocity"].shape == (plan.n, 3) and arr["Valid"].dtype == np.uint8
    assert np.array_equal(arr["Density"], vals[0] * 2) and np.array_equal(arr["Velocity"], (vals[1:4] * 2).T)
    assert np.array_equal(arr["VelocityMagnitude"], vals[4] * 2) and np.array_equal(arr["QCriterion"], vals[8] * 2)
    assert np.array_equal(arr["Valid"], plan.valid.astype(np.uint8))
    assert sl.read_pvd(os.path.join(tmp_path, "slice_wake.pvd")) == [(1.0, "slice_wake_000004.vti"), (2.0, "slice_wake_000008.vti")]
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".part")]


# ---- C entry points ----
def test_create_refuses_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    h = C.c_void_p()
    one = np.zeros(8, np.int32)
    w = np.zeros(3, np.float32)
    v = np.ones(1, np.uint8)
    s = np.ones(1, np.float32)
    assert lib.ludwig_slices_create(None, 1, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, w.ctypes.data, v.ctypes.data,
                                    s.ctypes.data, 0, C.byref(h)) != 0
    arr = (C.c_void_p * 1)(None)
    assert lib.ludwig_slices_create(arr, 1, 0, one.ctypes.data, one.ctypes.data, one.ctypes.data, w.ctypes.data, v.ctypes.data,
                                    s.ctypes.data, 0, C.byref(h)) != 0
    assert lib.ludwig_slices_create(arr, 1, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, w.ctypes.data, v.ctypes.data,
                                    s.ctypes.data, 4, C.byref(h)) != 0
    assert b"flags" in lib.ludwig_last_error()
    assert lib.ludwig_slices_create(arr, 1, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, w.ctypes.data, v.ctypes.data,
                                    s.ctypes.data, 0, C.byref(h)) != 0
    assert b"null" in lib.ludwig_last_error() and not h.value
    assert lib.ludwig_slices_sample(None, 1) != 0 and lib.ludwig_slices_download(None, None, 0) != 0
    lib.ludwig_slices_destroy(None)


# ---- run_case with the CPU oracle ----
CUBE = {"basic": {"num_levels": 1, "surface_resolution": 7, "simulation": {"steps": 10, "output_freq": 8}},
        "advanced": {"boundary": {"method": "bounce_back"}, "high_re": {"wall_model": {"enabled": False}},
                     "numerics": {"c_wale": 0.0, "nu_sgs_background": 0.0}, "diagnostics": {"freq": 4}}}


class GradOracleStepper:
    """the CPU oracle plus the velocity-gradient fields of the tests' float32 restatement: what run_case's slice fallback reads"""

    def __init__(self, grids):
        from _steppers import OracleStepper
        self.inner = OracleStepper(grids)
        self.grids = grids
        self.field = self.inner.field
        self.plans = None
        self.after = {}                   # step -> host_sample right after a batch that ended on a sampled step

    def batch(self, t_start, n, u_curr, params):
        self.inner.batch(t_start, n, u_curr, params)
        end = t_start + n - 1
        if self.plans is not None and end in (2, 5, 8):
            self.after[end] = sl.host_sample(self, self.plans, self.grids, end)

    def gradient_fields(self, level, vel_name, scale):
        from _gradient_ref import gradient_fields
        g = self.grids[level]
        return gradient_fields(getattr(g, vel_name), g.neighbor_table, g.obstacle, scale)

    def close(self):
        pass


def test_run_case_writes_slice_files_at_the_sampled_steps_and_leaves_the_rest_unchanged(tmp_path):
    from oracle import oracle
    oracle.set_num_threads(min(8, os.cpu_count() or 1))
    stl = os.path.join(G, "cube1m.stl")
    planes = [{"name": "mid", "normal": "y", "position": 0.02, "fields": ["density", "velocity", "vorticity", "q_criterion"]},
              {"name": "cross", "normal": "x", "position": 0.9, "bounds": [[-0.6, 0.6], [-0.5, 0.5]], "spacing": 0.05}]
    runs = {}
    for on in (False, True):
        over = {**CUBE, "advanced": {**CUBE["advanced"], "slices": {"enabled": on, "start_step": 2, "interval": 3, "planes": planes}}}
        cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), over)
        setup = pp.setup_multilevel_domain(cfg, stl)
        out = os.path.join(tmp_path, "on" if on else "off")
        holder = {}

        def factory(grids):
            holder["st"] = GradOracleStepper(grids)
            if on:
                holder["st"].plans = [sl.plan_slice(s, grids, setup[2].mesh_offset) for s in cfg.slices_planes]
            return holder["st"]
        case.run_case(cfg, factory, setup=setup, out_dir=out)
        runs[on] = (out, cfg, setup, holder["st"])
    off, on = runs[False][0], runs[True][0]
    steps = [2, 5, 8]
    new = [f"slice_{n}_{s:06d}.vti" for n in ("mid", "cross") for s in steps] + ["slice_mid.pvd", "slice_cross.pvd"]
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + new)
    for name in os.listdir(off):
        if name != "convergence.csv":                                       # wall time and MLUPS columns
            assert filecmp.cmp(os.path.join(off, name), os.path.join(on, name), shallow=False), name
    st, cfg, (grids, _, params, _) = runs[True][3], runs[True][1], runs[True][2]
    assert [t for t, _ in sl.read_pvd(os.path.join(on, "slice_mid.pvd"))] == [s * params.time_scale for s in steps]
    plans = [sl.plan_slice(s, grids, params.mesh_offset) for s in cfg.slices_planes]
    assert sorted(st.after) == steps                                      # batches end at every sampled step
    for s_step in steps:
        for plan, v in zip(plans, st.after[s_step]):
            attrs, arr = sl.read_vti(os.path.join(on, f"slice_{plan.spec.name}_{s_step:06d}.vti"))
            assert np.array_equal(arr["Valid"], plan.valid.astype(np.uint8)) and plan.valid.any()
            assert np.array_equal(arr["Density"].view(np.uint32), v[0].view(np.uint32))
            if "velocity" in plan.spec.fields:
                assert np.array_equal(arr["Velocity"], v[1:4].T)
            if "vorticity" in plan.spec.fields:
                assert np.array_equal(arr["Vorticity"], v[5:8].T) and np.array_equal(arr["QCriterion"], v[8])
                assert np.abs(v[5:9]).max() > 0
