"""Surface statistics without a GPU: the advanced.surface_statistics keys, the numpy restatement of k_accumulate_surface_stats
(HostSurfaceStats), finalize, the surface_mean VTU, the C entry points' declarations and argument checks, and run_case's
surface_mean_*.vtu / forces_mean.csv with the CPU oracle stepping (the host fallback)."""
import ctypes as C
import filecmp
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from open_ludwig_amd import _lib, case, cases, forces, preprocess as pp, surface_stats as ss
from open_ludwig_amd.statistics import sample_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _surface_common as common  # noqa: E402

F32 = np.float32
NEW_CALLS = ("ludwig_surface_stats_create", "ludwig_surface_stats_destroy", "ludwig_surface_stats_reset",
             "ludwig_surface_stats_accumulate", "ludwig_surface_stats_download", "ludwig_execute_timestep_batch_sampled")


# ---- configuration ----
def test_shipped_configs_parse_with_surface_statistics_off():
    for name in ("ball1m_config.yaml", "cube1m_config.yaml", "bunny_config.yaml"):
        cfg = pp.load_case_configuration(os.path.join(G, name))
        assert not cfg.surface_statistics_enabled
        assert cfg.surface_statistics_start_step == max(cfg.ramp_steps, 1) and cfg.surface_statistics_interval == 1


def test_surface_statistics_keys_parse_and_validate():
    p = os.path.join(G, "ball1m_config.yaml")
    on = pp.load_case_configuration(p, {"advanced": {"surface_statistics": {"enabled": True, "start_step": 7, "interval": 4}}})
    assert on.surface_statistics_enabled and (on.surface_statistics_start_step, on.surface_statistics_interval) == (7, 4)
    d = pp.load_case_configuration(p, {"advanced": {"surface_statistics": {"enabled": True}}})
    assert (d.surface_statistics_start_step, d.surface_statistics_interval) == (d.ramp_steps, 1)
    for start in (0, -5):
        c = pp.load_case_configuration(p, {"advanced": {"surface_statistics": {"enabled": True, "start_step": start}}})
        assert c.surface_statistics_start_step == 1
    for bad in (0, -1):
        with pytest.raises(ValueError, match="surface_statistics.interval"):
            pp.load_case_configuration(p, {"advanced": {"surface_statistics": {"enabled": True, "interval": bad}}})


# ---- the restatement ----
def _tunnel(levels=2):
    grids, _ = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    mesh, center, radius = common.tunnel_sphere_mesh(grids)
    return grids, mesh, common.tunnel_params(center, radius)


def _fields(g, seed):
    rng = np.random.default_rng(seed)
    rho = (1.0 + 0.02 * rng.standard_normal(g.rho.shape)).astype(F32)
    vel = (0.05 * rng.standard_normal(g.vel.shape)).astype(F32)
    return np.asfortranarray(rho), np.asfortranarray(vel)


def test_plan_and_sample_values_equal_the_instantaneous_mapping():
    grids, mesh, params = _tunnel()
    g = grids[-1]
    plan = ss.plan_surface(mesh, g, params)
    assert plan.n == mesh.centers.shape[0] and (~plan.found).sum() == 2 and plan.found[:-2].all()
    assert (plan.blocks[~plan.found] == -1).all()
    for seed in (1, 2):
        rho, vel = _fields(g, seed)
        p, tx, ty, tz, mag = ss.sample_values(plan, rho, vel, g.tau, params)
        want = forces.map_surface_stresses(mesh, rho, vel, g.obstacle, g.block_pointer, g.dx, g.tau, params)
        for a, b in zip((p, tx, ty, tz), want):
            assert a.dtype == F32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(mag, np.sqrt((tx * tx + ty * ty) + tz * tz))
        assert np.abs(tx).max() > 0 and not p[~plan.found].any() and not mag[~plan.found].any()


def test_host_sums_equal_a_direct_float64_loop():
    grids, mesh, params = _tunnel(levels=1)
    g = grids[0]
    plan = ss.plan_surface(mesh, g, params)
    h = ss.HostSurfaceStats(plan, g.tau, params)
    want = [[0.0] * plan.n for _ in range(7)]
    for seed in range(4):
        rho, vel = _fields(g, 10 + seed)
        h.accumulate(rho, vel)
        vals = ss.sample_values(plan, rho, vel, g.tau, params)
        for i in range(plan.n):
            p, tx, ty, tz, m = (float(v[i]) for v in vals)
            for k, x in enumerate((p, p * p, tx, ty, tz, m, m * m)):
                want[k][i] += x
    sums, n = h.download()
    assert n == 4 and sums.dtype == np.float64 and sums.shape == (7, plan.n)
    assert np.array_equal(sums, np.array(want))
    h.reset()
    assert h.download()[1] == 0 and not h.download()[0].any()
    with pytest.raises(ValueError):
        ss.HostSurfaceStats(plan, g.tau, params, 1, 0)


def test_finalize_against_direct_numpy():
    params = common.tunnel_params((0, 0, 0), 1.0)
    q = 0.5 * params.rho_physical * params.u_physical ** 2
    rng = np.random.default_rng(3)
    series = rng.standard_normal((9, 5, 50)).astype(F32)        # sample, quantity (p, tx, ty, tz, |tau|), triangle
    series[:, 4] = np.abs(series[:, 4])
    series[:, :, 0] = F32(0.1)                                    # a constant series: <v^2> - <v>^2 rounds to a tiny value
    sums = np.zeros((7, 50))
    for s in series:
        ss.add_sample(sums, s)
    f = ss.finalize(sums, 9, params)
    x = series.astype(np.float64)
    mean = x.mean(axis=0)
    assert np.allclose(f["mean_p"], mean[0], rtol=1e-13, atol=1e-15)
    assert np.allclose(f["mean_tau"], mean[1:4].T, rtol=1e-13, atol=1e-15)
    assert np.allclose(f["mean_tau_mag"], mean[4], rtol=1e-13)
    assert np.allclose(f["p_rms"][1:], x[:, 0, 1:].std(axis=0), rtol=1e-9)
    assert np.allclose(f["tau_mag_rms"][1:], x[:, 4, 1:].std(axis=0), rtol=1e-9)
    assert f["p_rms"][0] >= 0.0 and f["p_rms"][0] < 1e-7 and f["tau_mag_rms"][0] >= 0.0
    assert np.array_equal(f["Cp_mean"], f["mean_p"] / q) and np.array_equal(f["Cp_rms"], f["p_rms"] / q)
    assert np.array_equal(f["Cf_mean"], f["mean_tau_mag"] / q)
    const = np.zeros((7, 3))
    for _ in range(7):
        ss.add_sample(const, [np.full(3, F32(0.3))] * 5)          # sum/7 of 0.3 seven times: <p^2> < <p>^2 by rounding
    fc = ss.finalize(const, 7, params)
    assert (fc["p_rms"] >= 0).all() and (fc["Cp_rms"] >= 0).all() and np.isfinite(fc["p_rms"]).all()
    empty = ss.finalize(np.zeros((7, 4)), 0, params)
    for k, v in empty.items():
        assert np.isnan(v).all(), k


def test_surface_mean_vtu_round_trip(tmp_path):
    grids, mesh, params = _tunnel(levels=1)
    n = mesh.centers.shape[0]
    rng = np.random.default_rng(4)
    sums = np.zeros((7, n))
    for _ in range(3):
        ss.add_sample(sums, [rng.standard_normal(n).astype(F32) for _ in range(4)] + [rng.random(n).astype(F32)])
    fin = ss.finalize(sums, 3, params)
    found = np.arange(n) % 5 != 0
    path = ss.save_surface_mean_vtk(os.path.join(tmp_path, "surface_mean_000040"), mesh, fin, found, (3, 20, 40))
    assert path.endswith("surface_mean_000040.vtu")
    v = common.read_vtu(path)
    names = ["Pressure_Pa_mean", "Pressure_Pa_rms", "ShearX_Pa_mean", "ShearY_Pa_mean", "ShearZ_Pa_mean", "ShearMagnitude_Pa_mean",
             "ShearMagnitude_Pa_rms", "Cp_mean", "Cp_rms", "Cf_mean", "Normal", "Area_m2", "MappingQuality"]
    assert list(v["cells"]) == names and v["n_cells"] == n
    assert all(v["types"][k] == "Float32" for k in names)
    want = {"Pressure_Pa_mean": fin["mean_p"], "Pressure_Pa_rms": fin["p_rms"], "ShearX_Pa_mean": fin["mean_tau"][:, 0],
            "ShearY_Pa_mean": fin["mean_tau"][:, 1], "ShearZ_Pa_mean": fin["mean_tau"][:, 2], "ShearMagnitude_Pa_mean": fin["mean_tau_mag"],
            "ShearMagnitude_Pa_rms": fin["tau_mag_rms"], "Cp_mean": fin["Cp_mean"], "Cp_rms": fin["Cp_rms"], "Cf_mean": fin["Cf_mean"],
            "Normal": mesh.normals, "Area_m2": mesh.areas, "MappingQuality": found}
    for k, a in want.items():
        assert np.array_equal(v["cells"][k], np.asarray(a).astype(F32)), k
    assert {k: (v["types"][k], v["fields"][k].tolist()) for k in v["fields"]} == {
        "StatisticsSamples": ("Int64", [3]), "StatisticsFirstStep": ("Int64", [20]), "StatisticsLastStep": ("Int64", [40])}


def test_mean_forces_row_is_the_forces_of_the_mean_loads():
    grids, mesh, params = _tunnel(levels=1)
    g = grids[0]
    plan = ss.plan_surface(mesh, g, params)
    h = ss.HostSurfaceStats(plan, g.tau, params)
    for seed in range(2):
        h.accumulate(*_fields(g, 20 + seed))
    fin = ss.finalize(*h.download(), params)
    fr = ss.mean_forces(mesh, fin, params, symmetric=False)
    want = forces.integrate_surface_forces(mesh, fin["mean_p"].astype(F32), *(fin["mean_tau"][:, k].astype(F32) for k in range(3)), params)
    assert (fr.Cd, fr.Cl, fr.Fx, fr.My) == (want.Cd, want.Cl, want.Fx, want.My)
    row = ss.forces_mean_csv_row(12, (2, 4, 12), fr).split(",")
    assert len(row) == len(ss.FORCES_MEAN_CSV_HEADER.split(",")) and row[:4] == ["12", "2", "4", "12"]
    assert float(row[10]) == pytest.approx(fr.Cd, rel=1e-9, abs=1e-300) and float(row[11]) == pytest.approx(fr.Cl, rel=1e-9, abs=1e-300)
    assert ss.window_of(0, 5, 3) == (0, 0, 0) and ss.window_of(4, 5, 3) == (4, 5, 14)


# ---- the C interface ----
def test_header_bindings_and_julia_list_the_new_calls():
    header = open(os.path.join(ROOT, "include", "ludwig_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "LudwigHIP.jl")).read()
    for name in NEW_CALLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        # the binding reaches an in-batch observer through the observed batch call, as an entry of the observer's kind
        called = "ludwig_execute_timestep_batch_observed" if name.startswith("ludwig_execute_timestep_batch_") else name
        assert re.search(r"ccall\(\(:%s, LIB\)" % called, jl), name
    assert "entry(OBSERVE_SURFACE, s.surface, s.surface_start_step, s.surface_interval)" in jl
    assert "typedef struct LudwigBatchSamplers" in header and "struct BatchSamplers" in jl
    lib = _lib.load()
    assert lib.ludwig_abi_version() == 1
    for name in NEW_CALLS:
        assert getattr(lib, name) is not None


def test_batch_samplers_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ludwig_hip.h"\n'
                   "#define F(f) printf(\"%s %zu %zu\\n\", #f, offsetof(LudwigBatchSamplers, f), sizeof(((LudwigBatchSamplers *)0)->f))\n"
                   "int main(void) { printf(\"size %zu\\n\", sizeof(LudwigBatchSamplers)); F(probes); F(probes_start_step); "
                   "F(probes_interval); F(surface); F(surface_start_step); F(surface_interval); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    S = _lib.BatchSamplers
    assert int(got["size"]) == C.sizeof(S)
    for name, _ in S._fields_:
        off, size = (int(x) for x in got[name].split())
        assert (off, size) == (getattr(S, name).offset, getattr(S, name).size), name


def test_new_calls_reject_null_and_invalid_arguments_without_a_device():
    lib = _lib.load()
    h = C.c_void_p()
    sp = _lib.SurfaceParams(0.0, 0.5006, 0.0, 0.0, 0.0, 1.0, 1.0, 0)
    one = np.zeros(3, np.int32)
    f = np.zeros(3, np.float32)
    assert lib.ludwig_surface_stats_create(None, 0, None, None, None, None, C.byref(sp), C.byref(h)) == -1 and not h.value
    assert lib.ludwig_surface_stats_create(None, 1, one.ctypes.data, one.ctypes.data, f.ctypes.data, f.ctypes.data, C.byref(sp), None) == -1
    assert "null" in lib.ludwig_last_error().decode()
    assert lib.ludwig_surface_stats_reset(None) == -1
    assert lib.ludwig_surface_stats_accumulate(None, 3) == -1
    n = C.c_int64(0)
    assert lib.ludwig_surface_stats_download(None, None, 0, C.byref(n)) == -1
    lib.ludwig_surface_stats_destroy(None)
    fl = _lib.StepFlags()
    smp = _lib.BatchSamplers(None, 1, 1, None, 1, 0)
    assert lib.ludwig_execute_timestep_batch_sampled(None, 1, 1, 1, 0.05, C.byref(fl), C.byref(smp)) == -1
    arr = (C.c_void_p * 1)(None)
    assert lib.ludwig_execute_timestep_batch_sampled(arr, 1, 1, 1, 0.05, C.byref(fl), None) == -1      # null level
    assert lib.ludwig_execute_timestep_batch_sampled(arr, 0, 1, 1, 0.05, C.byref(fl), C.byref(smp)) == -1


# ---- run_case with the CPU oracle (the host fallback) ----
CUBE = {"basic": {"num_levels": 1, "surface_resolution": 7, "simulation": {"steps": 10, "output_freq": 4}},
        "advanced": {"boundary": {"method": "bounce_back"}, "high_re": {"wall_model": {"enabled": False}},
                     "numerics": {"c_wale": 0.0, "nu_sgs_background": 0.0}, "diagnostics": {"freq": 4},
                     "gpu": {"async_depth": 3}}}


def test_run_case_writes_surface_mean_files_and_leaves_the_rest_unchanged(tmp_path):
    from oracle import oracle
    from _steppers import OracleStepper
    oracle.set_num_threads(min(8, os.cpu_count() or 1))
    stl = os.path.join(G, "cube1m.stl")
    runs = {}
    for on in (False, True):
        over = {**CUBE, "advanced": {**CUBE["advanced"], "surface_statistics": {"enabled": on, "start_step": 2, "interval": 3}}}
        cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), over)
        assert not hasattr(OracleStepper, "surface_stats_setup")
        setup = pp.setup_multilevel_domain(cfg, stl)
        out = os.path.join(tmp_path, "on" if on else "off")
        case.run_case(cfg, OracleStepper, setup=setup, out_dir=out)
        runs[on] = (out, setup, cfg)
    off, on = runs[False][0], runs[True][0]
    means = ["surface_mean_000004.vtu", "surface_mean_000008.vtu"]
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + means + ["forces_mean.csv"])
    for name in os.listdir(off):
        if name != "convergence.csv":                                       # wall time and MLUPS columns
            assert filecmp.cmp(os.path.join(off, name), os.path.join(on, name), shallow=False), name
    _, (grids, mesh, params, _), cfg = runs[True]
    rows = [l.strip().split(",") for l in open(os.path.join(on, "forces_mean.csv"))]
    assert rows[0] == ss.FORCES_MEAN_CSV_HEADER.split(",")
    # batches of 3: the files of steps 4 and 8 hold the state at the end of batches 4-6 and 7-9, like every output file
    assert [r[:4] for r in rows[1:]] == [["4", "2", "2", "5"], ["8", "3", "2", "8"]]
    assert sample_steps(1, 9, 2, 3) == [2, 5, 8]
    for name, (n, last) in zip(means, ((2, 5), (3, 8))):
        v = common.read_vtu(os.path.join(on, name))
        assert [int(v["fields"][k][0]) for k in ("StatisticsSamples", "StatisticsFirstStep", "StatisticsLastStep")] == [n, 2, last]
        assert v["n_cells"] == mesh.centers.shape[0]
        assert np.isfinite(v["cells"]["Cp_mean"]).all() and (v["cells"]["Cp_rms"] >= 0).all()
        assert (v["cells"]["Cp_rms"] > 0).any() == (n > 1)
        assert v["cells"]["MappingQuality"].sum() > 0
