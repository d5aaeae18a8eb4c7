"""Force series without a GPU: the halving tree, the per-triangle contributions against forces.partial_force_sums, the CSV row, the
advanced.forces.series keys, and the C entry points' declarations and argument checks."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from open_ludwig_amd import _lib, case, cases, force_series as fs, forces, output, preprocess as pp, surface_stats as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _surface_common as common  # noqa: E402

F32 = np.float32
NEW_CALLS = ("ludwig_force_series_create", "ludwig_force_series_destroy", "ludwig_force_series_sample", "ludwig_force_series_download",
             "ludwig_execute_timestep_batch_loads")


# ---- the tree ----
def _padded_tree(x):
    """the explicit recursive tree over x zero-padded to the next power of two"""
    n = 1
    while n < len(x):
        n *= 2
    x = np.concatenate([np.asarray(x, np.float64), np.zeros(n - len(x), np.float64)])

    def rec(lo, hi):
        if hi - lo == 1:
            return np.float64(x[lo])
        mid = (lo + hi) // 2
        return np.float64(rec(lo, mid) + rec(mid, hi))
    return rec(0, n)


@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513, 1025])
def test_tree_sum_is_the_zero_padded_power_of_two_tree(n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(F32).astype(np.float64)
    got, want = forces.tree_sum_f64(x), _padded_tree(x)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    if n >= 511:                                                     # the order matters: a plain sequential sum gives other bits
        assert np.cumsum(x)[-1].tobytes() != want.tobytes()
    neg = -np.zeros(n)                                               # a total of -0.0 keeps its sign only where nothing is appended
    assert forces.tree_sum_f64(neg).tobytes() == _padded_tree(neg).tobytes()


def test_tree_sum_is_the_monitors():
    from open_ludwig_amd import monitor
    assert forces.tree_sum_f64 is monitor.tree_sum
    assert forces.tree_sum_f64(np.zeros(0)).tobytes() == np.float64(0.0).tobytes()


# ---- the contributions ----
def _tunnel(levels=2):
    grids, _ = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    mesh, center, radius = common.tunnel_sphere_mesh(grids)
    return grids, mesh, common.tunnel_params(center, radius)


def _loads(g, mesh, params, seed):
    rng = np.random.default_rng(seed)
    rho = np.asfortranarray((1.0 + 0.02 * rng.standard_normal(g.rho.shape)).astype(F32))
    vel = np.asfortranarray((0.05 * rng.standard_normal(g.vel.shape)).astype(F32))
    plan = ss.plan_surface(mesh, g, params)
    return plan, ss.sample_values(plan, rho, vel, g.tau, params)[:4], (rho, vel)


def test_contributions_are_the_terms_of_partial_force_sums():
    grids, mesh, params = _tunnel(3)
    plan, (p, tx, ty, tz), _ = _loads(grids[2], mesh, params, 1)
    params.mesh_offset = np.array([0.37, -1.2, 2.5])                 # a real offset: the arm is (c + off) - mc in two float32 steps
    assert plan.found.sum() > 100 and (~plan.found).any()
    contrib, covered = forces.force_series_contributions(mesh, p, tx, ty, tz, params)
    n = mesh.centers.shape[0]
    assert contrib.shape == (n, 9) and contrib.dtype == np.float32
    want = forces.partial_force_sums(mesh, p, tx, ty, tz, params)
    got = np.array([np.sum(contrib[:, k], dtype=np.float32) for k in range(9)], dtype=np.float32)
    assert got.tobytes() == want.tobytes()
    assert covered == forces.integrate_surface_forces(mesh, p, tx, ty, tz, params).coverage == int(plan.found.sum())
    assert np.abs(want).min() > 0.0
    # a rank's share: the same rows
    sel = np.arange(5, n, 3)
    part, cov = forces.force_series_contributions(mesh, p[sel], tx[sel], ty[sel], tz[sel], params, select=sel)
    assert part.tobytes() == contrib[sel].tobytes() and cov == int(plan.found[sel].sum())
    arm = forces.moment_arms(mesh, params)
    off, mc = params.mesh_offset.astype(F32), np.asarray(params.moment_center, F32)
    assert arm.dtype == np.float32 and arm.tobytes() == np.stack([(mesh.centers.astype(F32)[:, k] + off[k]) - mc[k] for k in range(3)]).tobytes()


def test_tree_record_agrees_with_float32_sums_within_the_first_order_bound():
    """any float32 summation order of n terms is within n 2^-23 sum|x_i| of the exact sum to first order (2^-24 per addition, at most
    n - 1 of them on a term's path, for the pairwise float32 sum; the float64 tree adds 2^-53 log2 n): the two differ by less"""
    grids, mesh, params = _tunnel(3)
    plan, (p, tx, ty, tz), _ = _loads(grids[2], mesh, params, 2)
    contrib, _ = forces.force_series_contributions(mesh, p, tx, ty, tz, params)
    rec = forces.record_of(contrib)
    want = forces.partial_force_sums(mesh, p, tx, ty, tz, params).astype(np.float64)
    n = contrib.shape[0]
    bound = n * 2.0 ** -23 * np.abs(contrib.astype(np.float64)).sum(axis=0)
    assert rec.dtype == np.float64 and (bound > 0).all()
    assert (np.abs(rec - want) <= bound).all(), (np.abs(rec - want) / bound).max()
    assert (rec != want).any()                                       # and they ARE different orders


def test_host_record_restates_one_sample():
    grids, mesh, params = _tunnel(2)
    plan, (p, tx, ty, tz), (rho, vel) = _loads(grids[1], mesh, params, 3)
    sums, cov = fs.host_record(mesh, plan, rho, vel, grids[1].tau, params)
    contrib, cov2 = forces.force_series_contributions(mesh, p, tx, ty, tz, params)
    assert sums.tobytes() == forces.record_of(contrib).tobytes() and cov == cov2
    assert forces.record_of(np.zeros((0, 9), F32)).tobytes() == np.zeros(9).tobytes()


# ---- the result file ----
def test_csv_row_has_the_columns_and_formats_of_forces_csv_plus_coverage():
    assert fs.csv_header() == output.FORCE_CSV_HEADER + ",Coverage"
    params = SimpleNamespace(rho_physical=1.225, u_physical=2.0, reference_area=3.0, reference_chord=0.5)
    sums = np.array([1.5, -2.0, 0.25, 0.125, 3.0, -0.5, 7.0, 8.0, -9.0])
    fr = forces.finish_forces(sums, 1234, params, symmetric=True)
    row = fs.csv_row(40, 0.4, fr, F32(0.03))
    assert row == output.force_csv_row(40, 0.4, fr, F32(0.03)) + ",1234"
    assert len(row.split(",")) == len(fs.csv_header().split(","))
    assert fr.Fx == 2.0 * (1.5 + 0.125) and fr.Fy == 0.0 and fr.My == 16.0          # the doubling stays finish_forces'
    m, r = fs.mean_rms([1.0, 3.0])
    assert (m, r) == (2.0, 1.0) and all(np.isnan(v) for v in fs.mean_rms([]))


def test_series_accumulator_and_segment_end():
    s = fs.Series()
    assert [a.shape for a in s.arrays()] == [(0,), (0, 9), (0,)]
    s.append(np.array([1, 2]), np.ones((2, 9)), np.array([5, 6]))
    s.append(np.zeros(0, np.int64), np.zeros((0, 9)), np.zeros(0, np.int64))
    s.append(np.array([3]), np.full((1, 9), 2.0), np.array([7]))
    steps, sums, cov = s.arrays()
    assert steps.tolist() == [1, 2, 3] and cov.tolist() == [5, 6, 7] and sums.shape == (3, 9) and sums[2, 0] == 2.0
    new = s.take_new()
    assert new[0].tolist() == [1, 2, 3] and s.take_new()[0].size == 0            # only what came since the last take
    s.append(np.array([4, 5]), np.full((2, 9), 3.0), np.array([8, 9]))
    new = s.take_new()
    assert new[0].tolist() == [4, 5] and new[1].shape == (2, 9) and new[2].tolist() == [8, 9] and s.arrays()[0].tolist() == [1, 2, 3, 4, 5]
    assert fs.segment_end(1, 8, 1, 1, 2) == 2 and fs.segment_end(3, 8, 1, 1, 64) == 8 and fs.segment_end(1, 8, 2, 3, 1) == 2
    assert fs.segment_end(1, 8, 9, 1, 1) == 8


def test_series_appends_stay_cheap_over_a_long_run():
    """12 500 batches of 8 records (a 100 000-step run at interval 1): the buffers are reallocated a dozen times, not once per batch,
    and a batch's take_new() copies that batch's records only"""
    s = fs.Series()
    buffers = set()
    one = np.ones((8, 9))
    for b in range(12500):
        steps = np.arange(8 * b + 1, 8 * b + 9)
        s.append(steps, one * b, steps)
        buffers.add(id(s._sums))
        new = s.take_new()
        assert new[0][0] == 8 * b + 1 and new[0].size == 8 and new[1].base is None
    assert len(buffers) <= 12
    steps, sums, cov = s.arrays()
    assert np.array_equal(steps, np.arange(1, 100001)) and np.array_equal(cov, steps) and sums[-1, 0] == 12499.0 and sums[8, 3] == 1.0


# ---- configuration ----
def test_series_key_defaults_off_and_validates():
    p = os.path.join(G, "ball1m_config.yaml")
    for name in ("ball1m_config.yaml", "cube1m_config.yaml", "bunny_config.yaml", "wing5deg_config.yaml"):
        cfg = pp.load_case_configuration(os.path.join(G, name))
        assert not cfg.forces_series_enabled and (cfg.forces_series_start_step, cfg.forces_series_interval) == (1, 1)
    off = pp.load_case_configuration(p, {"advanced": {"forces": {"series": {"enabled": False, "interval": 5}}}})
    assert not off.forces_series_enabled and off.forces_series_interval == 1
    on = pp.load_case_configuration(p, {"advanced": {"forces": {"series": {"enabled": True, "start_step": 7, "interval": 4}}}})
    assert on.forces_series_enabled and (on.forces_series_start_step, on.forces_series_interval) == (7, 4)
    d = pp.load_case_configuration(p, {"advanced": {"forces": {"series": {"enabled": True, "start_step": -3}}}})
    assert (d.forces_series_start_step, d.forces_series_interval) == (1, 1)
    with pytest.raises(ValueError, match=r"advanced\.forces\.series\.enabled.*advanced\.forces\.enabled"):
        pp.load_case_configuration(p, {"advanced": {"forces": {"enabled": False, "series": {"enabled": True}}}})
    with pytest.raises(ValueError, match=r"advanced\.forces\.series\.interval"):
        pp.load_case_configuration(p, {"advanced": {"forces": {"series": {"enabled": True, "interval": 0}}}})
    with pytest.raises(ValueError, match=r"advanced\.forces\.series must be a mapping"):
        pp.load_case_configuration(p, {"advanced": {"forces": {"series": True}}})


def test_a_stepper_without_the_device_set_is_refused_by_key_name():
    class NoSeries:
        def __init__(self, grids):
            self.closed = False

        def close(self):
            self.closed = True
    over = {"basic": {"num_levels": 1, "surface_resolution": 7, "simulation": {"steps": 2}},
            "advanced": {"forces": {"series": {"enabled": True}}}}
    cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), over)
    setup = pp.setup_multilevel_domain(cfg, os.path.join(G, "cube1m.stl"))
    made = []

    def factory(g):
        made.append(NoSeries(g))
        return made[-1]
    with pytest.raises(RuntimeError, match=r"advanced\.forces\.series.*NoSeries"):
        case.run_case(cfg, factory, setup=setup)
    assert made[0].closed


# ---- the C interface ----
def test_new_symbols_are_declared_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ludwig_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "ludwig_hip.h")).read()
    assert "#define LUDWIG_ABI_VERSION 1" in header.replace("  ", " ")
    for name in NEW_CALLS:
        assert name in _lib.EXPORTED_SYMBOLS and name + "(" in header and getattr(lib, name) is not None
    assert [n for n, _ in _lib.BatchSamplers._fields_] == ["probes", "probes_start_step", "probes_interval", "surface",
                                                          "surface_start_step", "surface_interval"]


def test_entry_points_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    h = C.c_void_p(1)
    sp = _lib.SurfaceParams(0.0, 0.5, 0.0, 0.0, 0.0, 1.0, 1.0, 0)
    assert lib.ludwig_force_series_create(None, 0, None, None, None, None, None, None, C.byref(sp), 4, C.byref(h)) == -1 and not h.value
    assert b"null" in lib.ludwig_last_error()
    assert lib.ludwig_force_series_create(None, 0, None, None, None, None, None, None, C.byref(sp), 4, None) == -1
    assert lib.ludwig_force_series_sample(None, 0, 0) == -1
    n = C.c_int32(7)
    assert lib.ludwig_force_series_download(None, None, None, None, 0, C.byref(n)) == -1
    lib.ludwig_force_series_destroy(None)                            # destroying nothing is a no-op
    fl = _lib.StepFlags()
    assert lib.ludwig_execute_timestep_batch_loads(None, 0, 1, 1, 0.0, C.byref(fl), None, None, 1, 1) == -1
    assert lib.ludwig_execute_timestep_batch_loads(None, 0, 1, 1, 0.0, C.byref(fl), None, C.c_void_p(8), 1, 1) == -1
