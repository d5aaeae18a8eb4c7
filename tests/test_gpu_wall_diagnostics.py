"""Wall diagnostics on the device (ludwig_level_wall_census, ludwig_wall_surface_*, run_case's wall_model.csv / wall_forces.csv and the
extra arrays of surface_%06d.vtu). wall_model_state evaluates the float32 expressions of tests/_wall_ref.py with the same jl_pow /
jl_log and -ffp-contract=off, the census is integers and the per-triangle values are one fixed float32 expression: every comparison is
bit equality."""
import ctypes as C
import os

import numpy as np
import pytest

import _edge_states as es
import _surface_common as common
import _wall_cases as wc
import _wall_ref as ref
from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, preprocess as pp
from open_ludwig_amd import surface_stats as ss, wall_diagnostics as wd
from open_ludwig_amd.statistics import t_sub_after

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


def _reference_census(d, g, lvl, steps):
    return ref.census(d.download("rho"), d.download(wc.vel_name(lvl, steps)), g.obstacle, g.wall_dist, g.tau)


def _check_stepped(name, grids, params, steps, u):
    dev = [adapt(g, 0) for g in grids]                                  # the default rho policy: the census call replays an elided rho
    try:
        execute_timestep_batch(dev, 1, steps, u, params)
        out = []
        for lvl, (d, g) in enumerate(zip(dev, grids)):
            got = wd.census(d, t_sub_after(lvl, steps))                 # before any download: the call itself has to produce rho
            want = _reference_census(d, g, lvl, steps)
            assert got == want, f"{name} level {lvl + 1}\n{got}\n{want}"
            assert got.near_cells > 0 and int(got.hist.sum()) == got.evaluated
            out.append(got)
        return out
    finally:
        for d in dev:
            d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [3, 4])
def test_census_of_the_16_block_tunnel_equals_the_restatement(gpu, steps):
    (rec,) = _check_stepped(*wc.tunnel(steps))
    assert rec.log_law > 0 and rec.evaluated - rec.log_law > 0 and rec.forced > 0 and rec.non_finite == 0


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(5))
def test_census_of_the_edge_state_entries_equals_the_restatement(gpu, index):
    c = wc.edge_entries()[index]
    (rec,) = _check_stepped(*c)
    if c[0] == "wall_umag_edges_1step":                                 # |u| = 1e-6 exactly is skipped, one ulp more is evaluated
        assert rec.near_cells - rec.evaluated == 1
    if c[0] == "wall_model_tau_half":
        assert rec.evaluated == 0 and rec.min_bits == wd.NO_MIN and rec.max_bits == wd.NO_MAX


@pytest.mark.gpu
def test_census_of_both_levels_of_the_2_level_tunnel_equals_the_restatement(gpu):
    recs = _check_stepped(*wc.tunnel_two_levels())
    assert len(recs) == 2 and all(r.evaluated > 0 for r in recs) and recs[0] != recs[1]


@pytest.mark.gpu
def test_planted_non_finite_states_are_counted_and_kept_out_of_the_rest(gpu):
    """uploads only: nothing is stepped"""
    name, grids, params, _, _ = wc.tunnel(0)
    g = grids[0]
    near = np.argwhere((g.wall_dist > 0) & (g.wall_dist < 10) & ~g.obstacle)
    d = adapt(g, 0)
    try:
        clean = wd.census(d, 1)
        assert clean == ref.census(g.rho, g.vel, g.obstacle, g.wall_dist, g.tau) and clean.non_finite == 0 and clean.evaluated > 0
        assert wd.census(d, 0) == ref.census(g.rho, g.vel_temp, g.obstacle, g.wall_dist, g.tau) != clean
        rho, vel = g.rho.copy(order="F"), g.vel.copy(order="F")
        a, b, c, e = (tuple(int(v) for v in near[i]) for i in (0, 7, 100, len(near) - 1))
        rho[a] = np.nan                                                 # y+ stays finite, the wall shear rho u_tau^2 does not
        rho[b] = np.inf
        vel[c + (1,)] = np.inf                                          # |u| = Inf: u_tau and y+ are not finite
        vel[e + (0,)] = np.nan                                          # |u| = NaN fails `u_mag > 1e-6`: the model is skipped, not evaluated
        far = tuple(int(v) for v in np.argwhere(~((g.wall_dist > 0) & (g.wall_dist < 10)) & ~g.obstacle)[0])
        rho[far] = np.nan                                               # not near the wall: not this observer's business
        d.upload("rho", rho)
        d.upload("vel", vel)
        got = wd.census(d, 1)
        assert got == ref.census(rho, vel, g.obstacle, g.wall_dist, g.tau)
        assert got.non_finite == 3 and got.near_cells == clean.near_cells and got.evaluated == clean.evaluated - 4
        assert int(got.hist.sum()) == got.evaluated and np.isfinite(got.y_plus_min) and np.isfinite(got.y_plus_max)
        assert got.min_bits >= clean.min_bits and got.max_bits <= clean.max_bits and got.max_bits < 0x7F800000
    finally:
        d.close()


def _assert_bits(got, want, what):
    es.assert_nan_aware_equal(got, want, what)


@pytest.mark.gpu
def test_surface_values_on_the_tunnel_sphere_for_both_velocity_buffers(gpu):
    name, grids, params, _, u = wc.tunnel(0)
    g = grids[0]
    mesh, center, radius = common.tunnel_sphere_mesh(grids)
    sparams = common.tunnel_params(center, radius)
    plan = ss.plan_surface(mesh, g, sparams)
    assert plan.found.all()                                             # (a triangle without a cell: the ball1m test below)
    d = adapt(g, 0)
    S = wd.DeviceWallSurface(plan, d, sparams)
    try:
        with pytest.raises(_lib.LudwigError):
            S.download()                                                # nothing computed yet
        seen = set()
        for t in (1, 2, 3, 4):
            execute_timestep_batch([d], t, 1, u, params)
            S.compute(t_sub_after(0, t))                                # before any download: the call itself has to produce rho
            got = S.download()
            want = ref.surface_values(plan, d.download("rho"), d.download(wc.vel_name(0, t)), g.obstacle, g.wall_dist, g.tau, sparams)
            for k, row in enumerate(wd.ROWS):
                _assert_bits(got[k], want[k], f"step {t} {row}")
            seen |= set(np.unique(got[6]).astype(int))
            assert np.abs(got[1:4]).max() > 0 and (got[5] > 0).any()
        assert {3, 7} <= seen and seen & {2, 6}, seen                   # log law with and without a force, and the power law
    finally:
        S.close()
        d.close()


RE266K = {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}, "simulation": {"steps": 8, "output_freq": 8}},
          "advanced": {"diagnostics": {"freq": 4}}}


def _cfg(name="ball1m", wall=None, **basic):
    over = {"basic": {**RE266K["basic"], **basic}, "advanced": dict(RE266K["advanced"])}
    if wall is not None:
        over["advanced"]["wall_diagnostics"] = wall
    return pp.load_case_configuration(os.path.join(G, f"{name}_config.yaml"), over)


@pytest.fixture(scope="module")
def ball_setup():
    return pp.setup_multilevel_domain(_cfg(), os.path.join(G, "ball1m.stl"))


@pytest.mark.gpu
def test_surface_values_on_ball1m_after_an_odd_and_an_even_coarse_step(gpu, ball_setup):
    grids, mesh, params, _ = ball_setup
    sp = pp.solver_params(_cfg(), params)
    fin = len(grids) - 1
    for i, g in enumerate(grids):
        cases.init_perturbed(g, 31 + i)                                 # a moving state: from rest the model is skipped everywhere
    plan = ss.plan_surface(mesh, grids[fin], params)
    lost = plan.subset(np.arange(plan.n))                               # the same plan with two triangles that found no cell
    lost.found[[0, 5]] = False
    lost.blocks[[0, 5]] = -1
    dev = [adapt(g, 0) for g in grids]
    S, S_lost = wd.DeviceWallSurface(plan, dev[fin], params), wd.DeviceWallSurface(lost, dev[fin], params)
    g = grids[fin]
    try:
        for t in (1, 2):
            execute_timestep_batch(dev, t, 1, F32(0.05), sp)
            S.compute(t_sub_after(fin, t))
            got = S.download()
            rho, vel = dev[fin].download("rho"), dev[fin].download(wc.vel_name(fin, t))
            want = ref.surface_values(plan, rho, vel, g.obstacle, g.wall_dist, g.tau, params)
            for k, row in enumerate(wd.ROWS):
                _assert_bits(got[k], want[k], f"step {t} {row}")
            assert ((got[6].astype(int) & 3) >= 2).sum() > plan.n // 2
            # the pressure is ludwig_map_surface_stresses' for the same cells
            h = grids[fin]
            p_map = case.forces_mod.map_surface_stresses_device(mesh, dev[fin], h.dx, h.tau, params, 5, "vel")[0]
            assert np.array_equal(got[0].view(np.uint32), np.asarray(p_map, F32).view(np.uint32))
            S_lost.compute(t_sub_after(fin, t))
            gl = S_lost.download()
            assert not gl[:, [0, 5]].any() and np.array_equal(np.delete(gl, [0, 5], axis=1).view(np.uint32), np.delete(got, [0, 5], axis=1).view(np.uint32))
    finally:
        S.close()
        S_lost.close()
        for d in dev:
            d.close()


@pytest.mark.gpu
def test_error_paths(gpu, hip_lib):
    grids, _ = cases.periodic_box((2, 1, 1))
    d = adapt(grids[0], 0)
    try:
        rec = _lib.WallCensus()
        assert hip_lib.ludwig_level_wall_census(d.handle, -1, C.byref(rec)) == -1 and b"t_sub" in hip_lib.ludwig_last_error()
        assert hip_lib.ludwig_level_wall_census(d.handle, 0, None) == -1
        assert wd.census(d, 0) == wd.Census()                           # wall_dist 100 everywhere: no block is flagged
        sp = _lib.SurfaceParams()
        out = C.c_void_p()
        bl, ce, nr = np.array([5], np.int32), np.array([0], np.int32), np.zeros(3, F32)
        assert hip_lib.ludwig_wall_surface_create(d.handle, 1, bl.ctypes.data, ce.ctypes.data, nr.ctypes.data, C.byref(sp), C.byref(out)) == -1
        assert b"block" in hip_lib.ludwig_last_error() and out.value is None
        bl[0], ce[0] = 1, 512
        assert hip_lib.ludwig_wall_surface_create(d.handle, 1, bl.ctypes.data, ce.ctypes.data, nr.ctypes.data, C.byref(sp), C.byref(out)) == -1
        ce[0] = 3
        assert hip_lib.ludwig_wall_surface_create(d.handle, 1, bl.ctypes.data, ce.ctypes.data, nr.ctypes.data, C.byref(sp), C.byref(out)) == 0
        vals = np.zeros(7, F32)
        assert hip_lib.ludwig_wall_surface_download(out, vals.ctypes.data, 28) == -5      # LUDWIG_ERR_STATE: nothing computed
        assert hip_lib.ludwig_wall_surface_compute(out, -1) == -1
        assert hip_lib.ludwig_wall_surface_compute(out, 0) == 0
        assert hip_lib.ludwig_wall_surface_download(out, vals.ctypes.data, 24) == -1
        assert hip_lib.ludwig_wall_surface_download(out, vals.ctypes.data, 28) == 0 and vals[6] == 0
        hip_lib.ludwig_wall_surface_destroy(out)
    finally:
        d.close()


# ---- run_case ----
def _strip_conv(raw):
    return [[c for i, c in enumerate(l.split(",")) if i not in (1, 5)] for l in raw.decode().splitlines()]


@pytest.mark.gpu
def test_run_case_off_means_off_and_on_writes_rows_and_surface_arrays(gpu, tmp_path):
    kept = []

    class Kept(case.HipStepper):
        def __init__(self, grids):
            super().__init__(grids)
            kept.append(self)

        def close(self):
            pass
    setup = pp.setup_multilevel_domain(_cfg("cube1m"), os.path.join(G, "cube1m.stl"))
    grids, mesh, params, _ = setup
    out = {}
    for key, wall in (("absent", None), ("off", {"enabled": False}), ("on", {"enabled": True, "band": [1.0, 300.0]})):
        out[key] = os.path.join(tmp_path, key)
        case.run_case(_cfg("cube1m", wall), Kept, setup=setup, out_dir=out[key])
    try:
        names = sorted(os.listdir(out["absent"]))
        assert names == sorted(os.listdir(out["off"])) and "wall_model.csv" not in names
        assert sorted(os.listdir(out["on"])) == sorted(names + ["wall_model.csv", "wall_forces.csv"])
        assert kept[0].wall_surface is None and kept[1].wall_surface is None
        for n in names:
            a, b, c = (open(os.path.join(out[k], n), "rb").read() for k in ("absent", "off", "on"))
            if n == "convergence.csv":                                  # wall time and MLUPS columns
                a, b, c = _strip_conv(a), _strip_conv(b), _strip_conv(c)
            assert a == b, n
            if not n.startswith("surface_"):
                assert a == c, n
        st = kept[2]
        lines = open(os.path.join(out["on"], "wall_model.csv")).read().splitlines()
        assert lines[0].startswith("# y_plus_target = 100") and lines[1] == wd.WALL_MODEL_CSV_HEADER
        rows = [l.split(",") for l in lines[2:]]
        assert [(r[0], r[1]) for r in rows] == [(s, str(g.level_id)) for s in ("8",) for g in grids]          # one batch of 8: one diagnostics step
        for lvl, g in enumerate(grids):                                 # the kept stepper still holds the state after step 8
            rec = st.wall_census(lvl, 8)
            assert ",".join(rows[lvl]) == wd.wall_model_csv_row(8, g.level_id, rec, (1.0, 300.0))
        forces = open(os.path.join(out["on"], "wall_forces.csv")).read().splitlines()
        assert forces[0] == wd.WALL_FORCES_CSV_HEADER and [l.split(",")[0] for l in forces[1:]] == ["8"]
        vals = st.wall_surface_values(8)
        assert forces[1] == wd.wall_forces_csv_row(8, mesh, vals, wd.model_forces(mesh, vals, params, _cfg("cube1m").symmetric_analysis))
        # the surface file: today's arrays with today's bytes, then the finalised wall arrays
        old = common.read_vtu(os.path.join(out["off"], "surface_000008.vtu"))
        new = common.read_vtu(os.path.join(out["on"], "surface_000008.vtu"))
        fin = wd.finalize(vals, params)
        assert list(new["cells"]) == list(old["cells"]) + list(fin)
        for k, a in old["cells"].items():
            assert np.array_equal(new["cells"][k], a), k
        for k, a in fin.items():
            es.assert_nan_aware_equal(new["cells"][k], a, k)
    finally:
        for st in kept:
            case.HipStepper.close(st)
