"""Flux planes on the host (flux_planes.py, preprocess._flux_planes_config, run_case's host fallback): configuration, the cell-centred
grid, the numpy restatement of the device reduction against analytic integrals and forces.tree_sum_f64, the ABI's declarations."""
import copy
import filecmp
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from open_ludwig_amd import _lib, case, cases, flux_planes as fp, forces, preprocess as pp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(G, "cube1m_config.yaml")
F32 = np.float32
NEW_CALLS = ("ludwig_flux_planes_create", "ludwig_flux_planes_destroy", "ludwig_flux_planes_sample", "ludwig_flux_planes_download")
PLANE = {"name": "wake", "normal": "x", "position": 1.0}
BOX = {"name": "cv", "bounds": [[-1.0, 1.0], [-1.0, 1.0], [-1.0, 1.0]]}


def _config(flux_cfg):
    return pp.load_case_configuration(CFG, {"advanced": {"flux_planes": flux_cfg}})


def test_configuration_defaults_parsing_and_refusals():
    cfg = pp.load_case_configuration(CFG)
    assert not cfg.flux_planes_enabled and cfg.flux_planes_planes == () and cfg.flux_planes_boxes == ()
    assert not _config({"enabled": False, "planes": "nonsense"}).flux_planes_enabled
    cfg = _config({"enabled": True, "start_step": 3, "interval": 2, "planes": [dict(PLANE, direction=-1, spacing=0.5,
                                                                                  bounds=[[-1, 1], [0, 2]])], "boxes": [BOX]})
    assert (cfg.flux_planes_enabled, cfg.flux_planes_start_step, cfg.flux_planes_interval) == (True, 3, 2)
    assert cfg.flux_planes_planes[0] == pp.FluxPlane("wake", 0, 1.0, ((-1.0, 1.0), (0.0, 2.0)), 0.5, -1, None)
    faces = cfg.flux_planes_planes[1:]
    assert [f.name for f in faces] == ["cv_xmin", "cv_xmax", "cv_ymin", "cv_ymax", "cv_zmin", "cv_zmax"]
    assert [(f.normal, f.position, f.direction) for f in faces] == [(0, -1.0, -1), (0, 1.0, 1), (1, -1.0, -1), (1, 1.0, 1), (2, -1.0, -1),
                                                                     (2, 1.0, 1)]                       # outward
    assert all(f.box == "cv" and f.bounds == ((-1.0, 1.0), (-1.0, 1.0)) for f in faces)
    assert cfg.flux_planes_boxes == (pp.FluxBox("cv", ((-1.0, 1.0),) * 3, None),)
    bad = [("nonsense", "must be a mapping"),
           ({"enabled": True, "interval": 0, "planes": [PLANE]}, "interval must be >= 1"),
           ({"enabled": True}, "at least one plane or box"),
           ({"enabled": True, "planes": [PLANE, PLANE]}, "not unique"),
           ({"enabled": True, "planes": [PLANE], "boxes": [dict(BOX, name="wake")]}, "not unique"),
           ({"enabled": True, "planes": [dict(PLANE, name="cv_xmin")], "boxes": [BOX]}, "not unique"),
           ({"enabled": True, "planes": [dict(PLANE, name="a/b")]}, "plain file-name stem"),
           ({"enabled": True, "planes": [dict(PLANE, name=".hidden")]}, "plain file-name stem"),
           ({"enabled": True, "planes": [dict(PLANE, direction=0)]}, "direction 0 is not 1 or -1"),
           ({"enabled": True, "planes": [dict(PLANE, direction=2)]}, "is not 1 or -1"),
           ({"enabled": True, "planes": [dict(PLANE, direction="up")]}, "is not 1 or -1"),
           ({"enabled": True, "planes": [dict(PLANE, bounds=[[0, 1]])]}, "bounds must be"),
           ({"enabled": True, "planes": [dict(PLANE, bounds=[[1, 0], [0, 1]])]}, "lower < upper"),
           ({"enabled": True, "planes": [dict(PLANE, spacing=0)]}, "spacing"),
           ({"enabled": True, "planes": [dict(PLANE, normal="w")]}, "is not x, y or z"),
           ({"enabled": True, "boxes": [dict(BOX, bounds=[[0, 1], [0, 1]])]}, "bounds must be"),
           ({"enabled": True, "boxes": [{"name": "cv"}]}, "bounds must be")]
    for flux_cfg, msg in bad:
        with pytest.raises(ValueError, match=re.escape(msg)):
            _config(flux_cfg)


def test_flux_grid_counts_cell_centred_coordinates_and_refusals():
    grids, _ = cases.periodic_box((3, 3, 3))                                   # 24^3 cells of dx 1
    dx = float(grids[0].dx)
    L = 24.0 * dx
    axes, h, dims, pts = fp.flux_grid(pp.FluxPlane("p", 1, 0.5 * L), grids)    # the defaults: the whole domain at the finest dx
    assert axes == (0, 2) and h == dx and dims == (24, 24) and pts.shape == (576, 3) and pts.dtype == np.float64
    assert np.array_equal(pts[:24, 0], (np.arange(24) + 0.5) * dx) and np.all(pts[:24, 2] == 0.5 * dx) and np.all(pts[:, 1] == 0.5 * L)
    assert np.array_equal(pts[24], [0.5 * dx, 0.5 * L, 1.5 * dx])              # point index i + n_a j
    # floor((hi - lo) / h) cells, at least one; the midpoints cover the bounds
    _, _, dims, pts = fp.flux_grid(pp.FluxPlane("p", 0, 1.0, ((2.0, 9.9), (3.0, 3.4)), 2.0), grids)
    assert dims == (3, 1) and np.array_equal(pts[:, 1], [3.0, 5.0, 7.0]) and np.array_equal(pts[:, 2], [4.0, 4.0, 4.0])
    # the STL frame: the domain starts at -offset
    _, _, dims, pts = fp.flux_grid(pp.FluxPlane("p", 2, -1.0), grids, offset=(2.0, 2.0, 2.0))
    assert dims == (24, 24) and pts[0, 0] == -2.0 + 0.5 * dx
    with pytest.raises(ValueError, match=r"flux plane 'p': position 25.0 lies outside the domain"):
        fp.flux_grid(pp.FluxPlane("p", 0, 25.0), grids)
    with pytest.raises(ValueError, match=r"flux plane 'p': bounds \[30.0, 31.0\] along y miss the domain"):
        fp.flux_grid(pp.FluxPlane("p", 0, 1.0, ((30.0, 31.0), (0.0, 1.0))), grids)
    with pytest.raises(ValueError, match=rf"more than {pp.SLICE_MAX_POINTS} per plane"):
        fp.flux_grid(pp.FluxPlane("p", 0, 1.0, None, 24.0 / 4097), grids)      # 4097^2 > 2^24
    assert fp.flux_grid(pp.FluxPlane("p", 0, 1.0, None, 24.0 / 4096.5), grids)[2] == (4096, 4096)       # the cap itself is allowed


def _fields(grids):
    return lambda li: (grids[li].rho, grids[li].vel)


def test_uniform_state_gives_count_times_the_integrand_and_a_closed_box():
    grids, params = cases.periodic_box((3, 3, 3))
    U, V, W = F32(0.04), F32(-0.02), F32(0.01)
    cases.set_state(grids[0], F32(1.0), U, V, W)
    u = np.array([U, V, W], dtype=np.float64)
    q = float(u @ u)
    for normal in range(3):
        plan = fp.plan_flux_plane(pp.FluxPlane("p", normal, 11.3, ((2.0, 21.0), (3.0, 20.0))), grids)
        sums, count = fp.host_record(plan, _fields(grids))
        assert count == 19 * 17 == plan.valid.sum()
        un = u[normal]
        want = np.array([1.0, un, un, un * u[0], un * u[1], un * u[2], q, un * q]) * count
        assert np.all(np.abs(sums - want) <= 1e-6 * np.abs(want)), (normal, sums / want - 1)
    box = pp.FluxBox("cv", ((4.0, 15.0), (5.0, 19.0), (6.0, 12.0)))
    faces = [fp.plan_flux_plane(f, grids) for f in pp.flux_box_faces(box)]

    class P:                                                                   # the scales a plane's quantities read
        rho_physical, velocity_scale, u_physical, reference_area, time_scale = 1.2, 250.0, 10.0, 2.0, 1.0e-3
    qs = [fp.plane_quantities(f, *fp.host_record(f, _fields(grids)), P) for f in faces]
    b = fp.box_quantities(list(zip(faces, qs)), P)
    assert all(abs(x.mass_flow) > 0 for x in qs)
    assert abs(b.mass_imbalance) <= 1e-6 * min(abs(x.mass_flow) for x in qs)
    assert qs[0].mass_flow < 0 < qs[1].mass_flow and qs[0].area == 14 * 6 and qs[0].count == 84      # x faces: outward signs
    assert all(abs(f) <= 1e-6 * abs(qs[1].momentum[0]) for f in b.force)       # nothing inside: no force


def test_linear_shear_gives_the_analytic_mass_and_momentum_flux():
    """u = (a + b y, 0, c), rho = 1: trilinear interpolation is exact for a linear field and the midpoint rule for a linear integrand,
    so only float32 rounding remains (a few 6e-8) in the mass flux through an x-normal plane, int (a + b y), and in the x-momentum
    flux through a z-normal plane, int c (a + b y). The x-momentum flux through the x-normal plane, int (a + b y)^2, is quadratic:
    the midpoint rule misses its integral by b^2 h^2 / 12 per unit area, here (1e-4)^2 / 12 / 9e-4 = 1e-6 of it. All to 1e-5."""
    grids, _ = cases.periodic_box((3, 3, 3))
    g = grids[0]
    _, gy, _ = cases.global_cell_coords(g)
    a, b, c = 0.03, 0.0002, 0.01
    ux = (a + b * (gy - 0.5)).astype(F32)                                      # at the cell centre's y
    cases.set_state(g, F32(1.0), ux, F32(0.0), F32(c))
    cf = float(F32(c))
    y0, y1, z0, z1, h = 3.0, 19.0, 4.0, 12.0, 0.5
    A = h * h
    plan = fp.plan_flux_plane(pp.FluxPlane("p", 0, 10.25, ((y0, y1), (z0, z1)), h), grids)
    sums, count = fp.host_record(plan, _fields(grids))
    assert count == 32 * 16 and not plan.replaced.any()
    mass = (a * (y1 - y0) + 0.5 * b * (y1 ** 2 - y0 ** 2)) * (z1 - z0)
    assert abs(sums[2] * A - mass) <= 1e-5 * mass and abs(sums[1] * A - mass) <= 1e-5 * mass
    mom = ((a + b * y1) ** 3 - (a + b * y0) ** 3) / (3 * b) * (z1 - z0)
    assert abs(sums[3] * A - mom) <= 1e-5 * mom
    assert sums[4] == 0.0 and abs(sums[5] * A - cf * mass) <= 1e-5 * cf * mass
    x0, x1 = 2.0, 14.0
    plan = fp.plan_flux_plane(pp.FluxPlane("q", 2, 9.75, ((x0, x1), (y0, y1)), h), grids)
    sums, count = fp.host_record(plan, _fields(grids))
    assert count == 24 * 32
    mom_x = cf * (a * (y1 - y0) + 0.5 * b * (y1 ** 2 - y0 ** 2)) * (x1 - x0)       # int c (a + b y) dx dy
    assert abs(sums[3] * A - mom_x) <= 1e-5 * mom_x
    assert abs(sums[2] * A - cf * (x1 - x0) * (y1 - y0)) <= 1e-5 * cf * (x1 - x0) * (y1 - y0)


def test_a_record_is_the_tree_sum_of_its_contributions_per_level_coarse_first():
    grids, _ = cases.tunnel_with_sphere(levels=2, wall_model=True)
    fields = _fields(grids)
    # 33 x 32 = 1056 points of spacing 0.25 inside the fine level, of which the first n form the list
    full = fp.plan_flux_plane(pp.FluxPlane("p", 0, 28.0, ((12.0, 20.25), (20.0, 28.0)), 0.25), grids)
    assert full.n == 1056 and full.valid.all() and (full.level == 1).all()
    c_all = fp.contributions(full, np.arange(full.n), *fields(1))
    assert c_all.dtype == F32 and c_all.shape == (1056, 8)
    for n in (1, 2, 3, 511, 512, 513, 1025):
        plan = copy.copy(full)
        plan.valid = np.arange(full.n) < n
        sums, count = fp.host_record(plan, fields)
        want = np.array([forces.tree_sum_f64(c_all[:n, k].astype(np.float64)) for k in range(8)])
        assert count == n and np.array_equal(sums.view(np.uint64), want.view(np.uint64)), n
    # two levels: coarse + fine, in that order
    plan = fp.plan_flux_plane(pp.FluxPlane("p", 0, 28.0, None, 0.5), grids)
    lists = plan.lists()
    assert [li for li, _ in lists] == [0, 1] and all(idx.size > 1 for _, idx in lists)
    recs = [fp.list_record(fp.contributions(plan, idx, *fields(li))) for li, idx in lists]
    sums, count = fp.host_record(plan, fields)
    assert np.array_equal(sums.view(np.uint64), (recs[0] + recs[1]).view(np.uint64)) and count == sum(idx.size for _, idx in lists)
    # a one-level plane is that level's record itself (no 0.0 + x: -0.0 survives)
    one = fp.plan_flux_plane(pp.FluxPlane("p", 0, 40.0, ((4.0, 27.0), (4.0, 27.0)), 1.0), grids)
    (li, idx), = one.lists()
    assert li == 0 and idx.size == 529
    assert np.array_equal(fp.host_record(one, fields)[0].view(np.uint64), fp.list_record(fp.contributions(one, idx, *fields(0))).view(np.uint64))
    assert np.signbit(fp.list_record(np.full((1, 8), -0.0, dtype=F32))).all()
    # no valid point: +0.0 and 0
    none = copy.copy(one)
    none.valid = np.zeros(one.n, bool)
    sums, count = fp.host_record(none, fields)
    assert count == 0 and np.array_equal(sums.view(np.uint64), np.zeros(8, np.uint64))


def test_series_and_segment_logic_are_the_force_series_own():
    from open_ludwig_amd import force_series as fs
    assert fp.segment_end is fs.segment_end and issubclass(fp.Series, fs.Series)
    s = fp.Series(3)
    s.append(np.array([2, 5]), np.arange(48.0).reshape(2, 3, 8), np.arange(6).reshape(2, 3))
    s.append(np.zeros(0, np.int64), np.zeros((0, 3, 8)), np.zeros((0, 3), np.int64))
    steps, sums, counts = s.take_new()
    assert steps.tolist() == [2, 5] and sums.shape == (2, 3, 8) and counts.tolist() == [[0, 1, 2], [3, 4, 5]] and sums[1, 2, 7] == 47.0
    assert s.take_new()[0].size == 0 and s.arrays()[0].tolist() == [2, 5]
    f = fs.Series()                                                            # the force series' own shape is the default
    f.append(np.array([1]), np.arange(9.0), np.array([4]))
    assert f.arrays()[1].shape == (1, 9) and f.arrays()[2].tolist() == [4]


def test_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.ludwig_abi_version() == 1 and _lib.OBSERVE_FLUXES == 4
    header = open(os.path.join(ROOT, "include", "ludwig_hip.h")).read()
    assert "#define LUDWIG_ABI_VERSION 1" in header.replace("  ", " ")
    assert re.search(r"LUDWIG_OBSERVE_FLUXES\s*=\s*4\b", header) and "typedef struct LudwigFluxPlanes LudwigFluxPlanes;" in header
    for name in NEW_CALLS:
        assert name in _lib.EXPORTED_SYMBOLS and name + "(" in header and getattr(lib, name) is not None
    declared = sorted(set(re.findall(r"\b(ludwig_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\bT (ludwig_[a-z_0-9]+)", out))) == declared == sorted(_lib.EXPORTED_SYMBOLS)
    jl = open(os.path.join(ROOT, "julia", "LudwigHIP.jl")).read()
    assert re.search(r"const OBSERVE_PROBES, OBSERVE_SURFACE, OBSERVE_FORCES, OBSERVE_TRACERS, OBSERVE_FLUXES = Int32\.\(0:4\)", jl)
    called = set(re.findall(r"ccall\(\(:(\w+), LIB\)", jl))
    assert set(NEW_CALLS) <= called <= set(declared)


def test_entry_points_reject_bad_arguments_without_a_device():
    import ctypes as C
    lib = _lib.load()
    h = C.c_void_p(1)
    assert lib.ludwig_flux_planes_create(None, 1, 0, None, None, None, None, None, None, None, 4, C.byref(h)) == -1 and not h.value
    assert b"null" in lib.ludwig_last_error()
    levels = (C.c_void_p * 1)(None)
    assert lib.ludwig_flux_planes_create(levels, 1, 0, None, None, None, None, None, None, None, 0, C.byref(h)) == -1
    assert b"capacity" in lib.ludwig_last_error()
    assert lib.ludwig_flux_planes_create(levels, 1, 0, None, None, None, None, None, None, None, 4, None) == -1
    assert lib.ludwig_flux_planes_sample(None, 0) == -1
    n = C.c_int32(7)
    assert lib.ludwig_flux_planes_download(None, None, None, None, 0, C.byref(n)) == -1
    lib.ludwig_flux_planes_destroy(None)                                       # destroying nothing is a no-op
    # a set without planes needs no device: it samples into its ring of steps and downloads nothing but them
    assert lib.ludwig_flux_planes_create(levels, 1, 0, None, None, None, None, None, None, None, 2, C.byref(h)) == 0 and h.value
    try:
        assert lib.ludwig_flux_planes_sample(h, 3) == 0 and lib.ludwig_flux_planes_sample(h, 4) == 0
        assert lib.ludwig_flux_planes_sample(h, 5) == -5 and b"ring full" in lib.ludwig_last_error()      # LUDWIG_ERR_STATE
        steps = np.zeros(2, np.int64)
        assert lib.ludwig_flux_planes_download(h, None, None, steps.ctypes.data, 2, C.byref(n)) == 0
        assert n.value == 2 and steps.tolist() == [3, 4]
        assert lib.ludwig_flux_planes_download(h, None, None, steps.ctypes.data, 2, C.byref(n)) == 0 and n.value == 0
    finally:
        lib.ludwig_flux_planes_destroy(h)


FLUX_CFG = {"enabled": True, "start_step": 2, "interval": 3,
            "planes": [{"name": "wake", "normal": "x", "position": 1.5, "direction": -1}],
            "boxes": [{"name": "cv", "bounds": [[-1.0, 1.2], [-0.9, 0.9], [-0.8, 0.8]]}]}


def test_run_case_with_a_stepper_without_a_device_set_integrates_on_the_host(tmp_path):
    """the CPU oracle behind run_case: flux_planes.host_sample on downloaded fields, batches cut at every sampled step; without the
    key neither file is written and every other file is what a run that never enters the feature's code path writes"""
    from _steppers import OracleStepper
    from oracle import oracle
    oracle.set_num_threads(min(8, os.cpu_count() or 1))
    base = {"basic": {"num_levels": 1, "surface_resolution": 7, "simulation": {"steps": 6, "output_freq": 8, "ramp_steps": 4}},
            "advanced": {"boundary": {"method": "bounce_back"}, "high_re": {"wall_model": {"enabled": False}},
                         "numerics": {"c_wale": 0.0, "nu_sgs_background": 0.0}, "diagnostics": {"freq": 4}}}
    outs, batches = {}, {}
    for which in ("on", "off", "never"):
        over = copy.deepcopy(base)
        if which == "on":
            over["advanced"]["flux_planes"] = FLUX_CFG
        cfg = pp.load_case_configuration(CFG, over)
        outs[which], batches[which] = str(tmp_path / which), []

        class Recording(OracleStepper):
            def batch(self, t_start, n, u_curr, params, _log=batches[which]):
                _log.append((t_start, n))
                super().batch(t_start, n, u_curr, params)
        if which == "never":                                                   # the feature's planning and sampling must not even be entered
            saved = fp.plan_flux_plane, fp.host_sample, fp.csv_rows
            fp.plan_flux_plane = fp.host_sample = fp.csv_rows = None
        try:
            case.run_case(cfg, Recording, stl_path=os.path.join(G, "cube1m.stl"), out_dir=outs[which], log=lambda s: None)
        finally:
            if which == "never":
                fp.plan_flux_plane, fp.host_sample, fp.csv_rows = saved
    assert [b[0] + b[1] - 1 for b in batches["on"]] == [2, 5, 6] and batches["off"] == batches["never"] and len(batches["off"]) == 1
    assert sorted(os.listdir(outs["on"])) == sorted(os.listdir(outs["off"]) + ["fluxes.csv", "flux_boxes.csv"])
    assert sorted(os.listdir(outs["off"])) == sorted(os.listdir(outs["never"]))
    for name in os.listdir(outs["off"]):
        if name != "convergence.csv":                                          # (it holds wall-clock times)
            assert filecmp.cmp(os.path.join(outs["off"], name), os.path.join(outs["never"], name), shallow=False), name
            assert filecmp.cmp(os.path.join(outs["off"], name), os.path.join(outs["on"], name), shallow=False), name
    lines = open(os.path.join(outs["on"], "fluxes.csv")).read().splitlines()
    assert lines[0] == fp.FLUXES_CSV_HEADER and lines[0].split(",")[:4] == ["Step", "Time_phys_s", "Plane", "MassFlow_kg_s"]
    rows = [l.split(",") for l in lines[1:]]
    names = ["wake", "cv_xmin", "cv_xmax", "cv_ymin", "cv_ymax", "cv_zmin", "cv_zmax"]
    assert [(int(r[0]), r[2]) for r in rows] == [(s, n) for s in (2, 5) for n in names] and all(len(r) == 13 for r in rows)
    assert all(int(r[12]) > 0 and float(r[11]) > 0 for r in rows)
    blines = open(os.path.join(outs["on"], "flux_boxes.csv")).read().splitlines()
    assert blines[0] == fp.BOXES_CSV_COMMENT and "without the viscous, subgrid and unsteady terms" in blines[0]
    assert blines[1] == fp.BOXES_CSV_HEADER == "Step,Time_phys_s,Box,MassImbalance_kg_s,Fx_N,Fy_N,Fz_N,Cd,Cl"
    assert [(int(l.split(",")[0]), l.split(",")[2]) for l in blines[2:]] == [(2, "cv"), (5, "cv")]
    # a box's rows are its faces' rows combined: the mass imbalance is the sum of the six outward mass flows
    for k, step in enumerate((2, 5)):
        faces = [float(r[3]) for r in rows if int(r[0]) == step and r[2].startswith("cv_")]
        assert abs(float(blines[2 + k].split(",")[3]) - sum(faces)) <= 1e-9 * max(abs(f) for f in faces)


def test_distributed_stepper_refuses_and_names_the_key():
    st = object.__new__(case.DistributedStepper)                               # the refusal needs no device and no process group
    with pytest.raises(RuntimeError, match=r"advanced\.flux_planes"):
        st.flux_planes_setup(None)
    cfg = pp.load_case_configuration(CFG, {"basic": {"num_levels": 1, "surface_resolution": 7}, "advanced": {"flux_planes": FLUX_CFG}})
    closed = []

    class Refusing:
        def __init__(self, grids):
            pass

        flux_planes_setup = case.DistributedStepper.flux_planes_setup

        def close(self):
            closed.append(True)
    with pytest.raises(RuntimeError, match=r"advanced\.flux_planes"):
        case.run_case(cfg, Refusing, stl_path=os.path.join(G, "cube1m.stl"), steps=1)
    assert closed == [True]
