"""The surface-force path on the host against tests/_force_ref.py, the restatement written from src/forces/surface.jl alone, and against
the hand-written cells of tests/_force_cases.py: forces.nearest_fluid_cells (the SurfacePlan every device set reads), stress_from_cells
/ map_surface_stresses, the nine sums, the per-triangle contributions, finish_forces, and the coverage count. No GPU."""
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import forces, preprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _edge_states as edge  # noqa: E402
import _force_cases as fc  # noqa: E402
import _force_ref as ref  # noqa: E402
import _step_ref  # noqa: E402
import _surface_common as common  # noqa: E402

F32 = np.float32
LEVELS = ("full", "boxes", "holes")
TAUS = (None, 0.5, 0.500001)                   # the level's own; nu = 0; the smallest tau the step allows


def _cell(found, block, lx, ly, lz, i):
    return (int(block[i]), int(lx[i]), int(ly[i]), int(lz[i])) if found[i] else None


def _host_cells(nc):
    return [_cell(nc.found, nc.block, nc.lx, nc.ly, nc.lz, i) for i in range(nc.found.size)]


def _ref_cells(c):
    return [_cell(c.found, c.block, c.local[:, 0], c.local[:, 1], c.local[:, 2], i) for i in range(c.found.size)]


@pytest.fixture(scope="module")
def levels():
    """the table's host levels with their random fields; shared, never changed"""
    out = {}
    for name in LEVELS:
        g = fc.build_level(name)
        out[name] = (g, fc.random_fields(g))
    return out


@pytest.fixture(scope="module")
def sphere():
    grids, sparams, mesh, params = fc.sphere_case()
    g = grids[1]
    return g, fc.random_fields(g), mesh, params


# ---- the table itself ----
def test_force_table_holds_every_situation(levels):
    names = [r.name for r in fc.ROWS]
    assert len(set(names)) == len(names)
    tags = {t for r in fc.ROWS for t in r.tags}
    assert tags == set(fc.SITUATIONS), (tags ^ set(fc.SITUATIONS))
    assert {r.level for r in fc.ROWS} == set(LEVELS)
    assert {r.radius for r in fc.ROWS} == {0, 1, 5, 16}
    assert any(r.offset != fc.NO_OFFSET for r in fc.ROWS)
    for r in fc.ROWS:
        g = levels[r.level][0]
        assert g.dx in (0.5, 1.0)
        t = [c + o for c, o in zip(r.centre, r.offset)]
        assert all(float(v * 8).is_integer() for v in t), r.name                    # dyadic: exact in float32 and float64
        assert ("equidistant" in r.tags) == r.tie, r.name
        if r.expect is None:
            continue
        b, lx, ly, lz = r.expect
        assert 0 <= b < g.n_blocks and not g.obstacle[lx, ly, lz, b], r.name
        # the typed cell lies within the search radius of the base cell and in the block the id names
        cell = [(int(m[b]) - 1) * 8 + l + 1 for m, l in zip((g.map_x, g.map_y, g.map_z), (lx, ly, lz))]
        base = [int(np.floor(v / g.dx)) + 1 for v in t]
        assert max(abs(c - q) for c, q in zip(cell, base)) <= max(r.radius, 0), (r.name, cell, base)
    g = levels["holes"][0]
    assert (np.asarray(g.block_pointer) == 0).sum() == 5 and not g.obstacle.any()
    g = levels["full"][0]
    assert len({g.grid_dim_x, g.grid_dim_y, g.grid_dim_z}) == 3 and g.obstacle.sum() == len(fc.FULL_SOLID) + 26
    assert levels["boxes"][0].obstacle.sum() == 11 ** 3 - 1 + 11 ** 3 + 7 ** 3 - 1 + 5 ** 3 - 1
    far = [r for r in fc.ROWS if "far" in r.tags]
    assert all(900 <= max(abs(c) for c in r.centre) / levels[r.level][0].dx <= 1100 for r in far)


# ---- the search ----
@pytest.mark.parametrize("name", LEVELS)
def test_nearest_fluid_cells_gives_the_hand_written_cells_and_the_restatement(levels, name):
    g, _ = levels[name]
    for (radius, offset), rows in fc.groups(name).items():
        mesh = fc.mesh_of([r.centre for r in rows], fc.row_normals(len(rows)))
        params = fc.params(offset)
        nc = forces.nearest_fluid_cells(mesh, g.obstacle, g.block_pointer, g.dx, params, radius)
        want = [r.expect for r in rows]
        assert _host_cells(nc) == want, [(r.name, a, b) for r, a, b in zip(rows, _host_cells(nc), want) if a != b]
        for ft in (np.float32, np.float64):
            c = ref.search(mesh.centers, offset, g.dx, g.obstacle, g.block_pointer, radius, ft)
            assert _ref_cells(c) == want, (ft.__name__, [(r.name, a, b) for r, a, b in zip(rows, _ref_cells(c), want) if a != b])
            if ft is np.float32:
                assert nc.wall_dist.dtype == np.float32 and nc.wall_dist.tobytes() == c.wall_dist.tobytes()
        miss = ~nc.found
        assert not nc.block[miss].any() and not nc.lx[miss].any() and (nc.wall_dist[miss] == F32(0.5)).all()


def test_a_base_cell_that_is_not_the_nearest_in_float32():
    """dx = float32(0.1) on the `full` level: 0.5 / dx and 1.5 / dx round UP to the integers 5 and 15 in float32, so the base cell is
    (6,16,3) although the point lies (by 1.5e-9) in cell (5,15,3) - and the float32 distances say so: 0.0024999983 < 0.002500001 in
    x, 0.0024999953 < 0.0025000072 in y. The only situation in which shell 1 after a hit at radius 0 changes the winner; the dyadic
    rows cannot have it. (5,15,3) is block (1,2,1) = id 2, local (4,6,2), typed by hand. Float64 puts the base there directly."""
    g = fc.build_level("full")
    mesh = fc.mesh_of([fc.NON_DYADIC_CENTRE], fc.row_normals(1))
    dx = float(F32(0.1))
    nc = forces.nearest_fluid_cells(mesh, g.obstacle, g.block_pointer, dx, fc.params(), 5)
    assert _host_cells(nc) == [fc.NON_DYADIC_EXPECT]
    c32 = ref.search(mesh.centers, fc.NO_OFFSET, dx, g.obstacle, g.block_pointer, 5, np.float32)
    c64 = ref.search(mesh.centers, fc.NO_OFFSET, dx, g.obstacle, g.block_pointer, 5, np.float64)
    assert _ref_cells(c32) == _ref_cells(c64) == [fc.NON_DYADIC_EXPECT]
    assert c32.base[0].tolist() == [6, 16, 3] and c64.base[0].tolist() == [5, 15, 3]
    assert nc.wall_dist.tobytes() == c32.wall_dist.tobytes()
    r0 = forces.nearest_fluid_cells(mesh, g.obstacle, g.block_pointer, dx, fc.params(), 0)
    assert _host_cells(r0) == [(2, 5, 7, 2)]                                       # radius 0 stays on the base cell


def test_sphere_cells_equal_the_restatement(sphere):
    g, _, mesh, params = sphere
    assert mesh.centers.shape[0] == 322 and g.dx == 0.5
    for radius in (0, 1, 5):
        nc = forces.nearest_fluid_cells(mesh, g.obstacle, g.block_pointer, g.dx, params, radius)
        for ft in (np.float32, np.float64):
            c = ref.search(mesh.centers, params.mesh_offset, g.dx, g.obstacle, g.block_pointer, radius, ft)
            assert _ref_cells(c) == _host_cells(nc), (radius, ft.__name__)
        if radius == 5:
            assert nc.found.all()                                                  # also the two tiny triangles at the centre (wd 9)
            assert nc.wall_dist.tobytes() == ref.search(mesh.centers, params.mesh_offset, g.dx, g.obstacle, g.block_pointer, 5,
                                                        np.float32).wall_dist.tobytes()


# ---- the stress ----
def _assert_equals_ref32(got, r32, what):
    """bit for bit (so -0 != +0); NaN meets NaN"""
    for name, a, b in zip(("p", "tau_x", "tau_y", "tau_z"), got, (r32.p, r32.tau[:, 0], r32.tau[:, 1], r32.tau[:, 2])):
        assert a.dtype == np.float32 and b.dtype == np.float32
        edge.assert_nan_aware_equal(a, b, f"{what} {name}")


def _evaluate(g, fields, vel_name, mesh, params, radius, tau):
    tau = g.tau if tau is None else tau
    r32, r64 = fc.ref_pair(g, fields, vel_name, mesh, params, radius, tau)
    got = forces.map_surface_stresses(mesh, fields["rho"], fields[vel_name], g.obstacle, g.block_pointer, g.dx, tau, params, radius)
    return got, r32, r64


@pytest.mark.parametrize("tau", TAUS)
def test_map_surface_stresses_equals_ref32_bit_for_bit_and_ref64_within_the_bound(levels, sphere, tau):
    calls = list(fc.table_calls(levels))
    g, fields, mesh, params = sphere
    calls.append(("sphere", g, fields, mesh, params, 5, np.ones(322, bool)))
    for what, g, fields, mesh, params, radius, compare in calls:
        for vel_name in ("vel", "vel_temp"):
            with np.errstate(all="ignore"):
                got, r32, r64 = _evaluate(g, fields, vel_name, mesh, params, radius, tau)
            _assert_equals_ref32(got, r32, f"{what} {vel_name}")
            _, _, err_p, err_t, excluded = fc.e_ref_and_errors(got, r32, r64, compare)
            assert excluded <= _step_ref.MAX_EXCLUDED_SHARE * compare.sum(), (what, excluded)
            assert err_p <= ref.bound("p") and err_t <= ref.bound("tau"), (what, vel_name, err_p, err_t)
            miss = ~r32.cells.found
            for a in got:
                assert a[miss].tobytes() == np.zeros(int(miss.sum()), F32).tobytes()          # four exact +0.0 without a cell


def test_planted_states_take_the_branch_they_are_planted_for(levels):
    g, fields = levels["full"]
    states = fc.planted_states()
    planted, mesh = fc.plant(g, fields, states)
    with np.errstate(all="ignore"):
        got, r32, r64 = _evaluate(g, planted, "vel", mesh, fc.params(), 5, None)
    by = {s.name: i for i, s in enumerate(states)}
    gate = r32.gates[:, 0]
    assert r32.cells.found.all() and r32.gates[:, 1].all()                         # every state triangle sits below wd = 0.5
    for name in ("parallel_dyadic_x", "parallel_dyadic_minus_z", "ut_below_gate", "ut_at_gate"):
        assert not gate[by[name]] and not r32.tau[by[name]].any(), name
    assert gate[by["ut_above_gate"]] and r32.tau[by["ut_above_gate"], 0] > 0
    # u parallel to a non-dyadic normal: u_t is pure rounding residue (1e-9 against |u| = 0.05) and still above the gate, so the shear is
    # that residue's direction - ref32 and ref64 do not even agree on its sign, which is why this state is held to ref32 only
    i = by["parallel_non_dyadic"]
    assert gate[i] and r64.gates[i, 0] and 0 < np.abs(r32.tau[i]).max() < 1e-8 and (np.sign(r32.tau[i]) != np.sign(r64.tau[i])).any()
    assert r32.p[by["rho_one"]] == 0 and r32.p[by["rho_below_one_ny0"]] < 0 < r32.p[by["rho_above_one_ny0"]]
    assert np.isnan(r32.p[by["rho_nan"]]) and np.isinf(r32.p[by["rho_inf"]]) and np.isfinite(r32.p[by["u_nan"]])
    assert not gate[by["u_nan"]] and not r32.tau[by["u_nan"]].any()                # NaN > 1e-10 is false: zeros, not NaN
    contrib = ref.contributions(r32.p, r32.tau, mesh.centers, mesh.normals, mesh.areas, (0, 0, 0), (0, 0, 0), np.float32)
    lo, hi = contrib[by["rho_below_one_ny0"], 1], contrib[by["rho_above_one_ny0"], 1]
    assert lo == 0 and hi == 0 and not np.signbit(lo) and np.signbit(hi)           # -p n_y A with n_y = 0: +0.0 and -0.0
    # the clamp and the two sides of 0.5 in the table rows
    g2, f2 = levels["full"]
    rows = fc.groups("full")[(5, fc.NO_OFFSET)]
    mesh2 = fc.mesh_of([r.centre for r in rows], fc.row_normals(len(rows)))
    c = ref.search(mesh2.centers, fc.NO_OFFSET, g2.dx, g2.obstacle, g2.block_pointer, 5, np.float32)
    wd = {r.name: float(c.wall_dist[i]) for i, r in enumerate(rows)}
    assert wd["cell_centre"] == 0.0 and wd["generic"] < 0.5 and wd["face_centred"] == 0.5 and wd["on_face"] > 0.5


# ---- sums, contributions, coefficients ----
def _finish_ref(nine, params, symmetric):
    return ref.finish(nine, symmetric, params.rho_physical, params.u_physical, params.reference_area, params.reference_chord)


def _assert_finish_equal(fr, want):
    for k, v in want.items():
        assert getattr(fr, k) == v and np.signbit(getattr(fr, k)) == np.signbit(v), (k, getattr(fr, k), v)


def test_sums_contributions_and_finish_against_the_restatement(levels, sphere):
    g, fields, mesh, params = sphere
    params.mesh_offset = np.array([0.375, -1.25, 2.5])                              # moves the arms, not the plan
    try:
        _, r32, _ = _evaluate(g, fields, "vel", mesh, fc.params(), 5, None)
        p, tx, ty, tz = r32.p, r32.tau[:, 0], r32.tau[:, 1], r32.tau[:, 2]
        want32 = ref.contributions(p, r32.tau, mesh.centers, mesh.normals, mesh.areas, params.mesh_offset, params.moment_center, np.float32)
        got, cov = forces.force_series_contributions(mesh, p, tx, ty, tz, params)
        assert got.dtype == np.float32 and got.tobytes() == want32.tobytes()
        assert cov == ref.coverage(p) == 322
        nine64 = ref.sums(want32)
        bound = fc.first_order_bound(want32)
        sums32 = forces.partial_force_sums(mesh, p, tx, ty, tz, params)
        assert (bound > 0).all() and (np.abs(sums32.astype(np.float64) - nine64) <= bound).all()
        assert (np.abs(forces.record_of(got) - nine64) <= bound).all()
        for symmetric in (False, True):
            fr = forces.integrate_surface_forces(mesh, p, tx, ty, tz, params, symmetric)
            _assert_finish_equal(fr, _finish_ref(sums32, params, symmetric))
            assert fr.coverage == 322
            _assert_finish_equal(forces.finish_forces(nine64, 7, params, symmetric), _finish_ref(nine64, params, symmetric))
    finally:
        params.mesh_offset = np.zeros(3)


def test_finish_symmetric_table_and_reference_guards():
    """src/forces/surface.jl:518-526 as a literal table, and F_ref / M_ref <= 1e-10 leaving the coefficients at 0"""
    nine = np.array([1.5, -2.0, 0.25, 0.125, 3.0, -0.5, 7.0, 8.0, -9.0])
    p = fc.params()                                                                # rho 1.225, U 2: q = 2.45; A 10: F_ref 24.5; L 3: M_ref 73.5
    plain = forces.finish_forces(nine, 3, p, False)
    assert (plain.Fx, plain.Fy, plain.Fz) == (1.625, 1.0, -0.25) and (plain.Mx, plain.My, plain.Mz) == (7.0, 8.0, -9.0)
    assert (plain.Cd, plain.Cl, plain.Cs) == (1.625 / 24.5, -0.25 / 24.5, 1.0 / 24.5)          # Cl from Fz, Cs from Fy
    assert (plain.Cmx, plain.Cmy, plain.Cmz) == (7.0 / 73.5, 8.0 / 73.5, -9.0 / 73.5)
    sym = forces.finish_forces(nine, 3, p, True)
    assert (sym.Fx_pressure, sym.Fy_pressure, sym.Fz_pressure) == (3.0, 0.0, 0.5)
    assert (sym.Fx_viscous, sym.Fy_viscous, sym.Fz_viscous) == (0.25, 0.0, -1.0)
    assert (sym.Fx, sym.Fy, sym.Fz) == (3.25, 0.0, -0.5) and (sym.Mx, sym.My, sym.Mz) == (0.0, 16.0, 0.0)
    assert (sym.Cd, sym.Cl, sym.Cs, sym.Cmx, sym.Cmy, sym.Cmz) == (3.25 / 24.5, -0.5 / 24.5, 0.0, 0.0, 16.0 / 73.5, 0.0)
    _assert_finish_equal(sym, _finish_ref(nine, p, True))
    p.reference_area = 0.0
    zero = forces.finish_forces(nine, 3, p, False)
    assert (zero.Cd, zero.Cl, zero.Cs, zero.Cmx, zero.Cmy, zero.Cmz) == (0.0,) * 6 and zero.Fx == 1.625
    _assert_finish_equal(zero, _finish_ref(nine, p, False))
    p.reference_area, p.reference_chord = 10.0, 0.0
    no_chord = forces.finish_forces(nine, 3, p, False)
    assert no_chord.Cd == 1.625 / 24.5 and (no_chord.Cmx, no_chord.Cmy, no_chord.Cmz) == (0.0, 0.0, 0.0)
    p.reference_area, p.reference_chord = 1e-10 / 2.45, 1.0                          # F_ref == 1e-10 exactly is NOT above the guard
    assert 2.45 * p.reference_area == 1e-10 and forces.finish_forces(nine, 3, p, False).Cd == 0.0


# ---- integration on closed meshes: no restatement needed ----
def _closed_meshes():
    cube = pp.load_mesh(os.path.join(G, "cube1m.stl"))
    ball = common.sphere_mesh((1.5, -0.5, 2.0), 1.25, 2, inside=False)
    return (("cube1m", cube, 1.0), ("icosphere", ball, 4.0 / 3.0 * np.pi * 1.25 ** 3))


@pytest.mark.parametrize("which", [0, 1])
def test_integration_on_a_closed_mesh(which):
    """uniform p: zero net force; p = a z: F = (0, 0, -a V) with V the mesh's own volume from the divergence theorem at the centroids
    (exact for flat triangles), which fixes the sign convention and the outward normals; uniform tau: F_v = tau A_total"""
    name, mesh, v_analytic = _closed_meshes()[which]
    n = mesh.centers.shape[0]
    params = fc.params(moment_center=(0.0, 0.0, 0.0))
    zero = np.zeros(n, F32)
    vol = float((mesh.centers[:, 2] * mesh.normals[:, 2] * mesh.areas).sum())
    assert 0.9 * v_analytic < vol <= v_analytic * (1 + 1e-12), (name, vol)          # positive: the normals point outward
    p = np.full(n, F32(3.5))
    s = forces.partial_force_sums(mesh, p, zero, zero, zero, params).astype(np.float64)
    mag = np.abs(forces.force_series_contributions(mesh, p, zero, zero, zero, params)[0].astype(np.float64)).sum(axis=0)
    tol = n * 2.0 ** -23 * mag + 2.0 ** -23 * mag                                   # the sum's order, and each term's own rounding
    assert (mag[:3] > 0).all() and (np.abs(s[:3]) <= tol[:3]).all(), (name, s[:3], tol[:3])
    a = 0.75
    pz = (a * mesh.centers[:, 2]).astype(F32)
    s = forces.partial_force_sums(mesh, pz, zero, zero, zero, params).astype(np.float64)
    mag = np.abs(forces.force_series_contributions(mesh, pz, zero, zero, zero, params)[0].astype(np.float64)).sum(axis=0)
    tol = (n + 4) * 2.0 ** -23 * mag                                                # + the rounding of p, n, A and the two products
    assert abs(s[0]) <= tol[0] and abs(s[1]) <= tol[1] and abs(s[2] + a * vol) <= tol[2], (name, s[:3], a * vol, tol[:3])
    assert s[2] < 0
    t = F32(0.125)
    s = forces.partial_force_sums(mesh, zero, np.full(n, t), np.full(n, -t), np.full(n, 2 * t), params).astype(np.float64)
    area = float(mesh.areas.sum())
    assert np.allclose(s[3:6], [0.125 * area, -0.125 * area, 0.25 * area], rtol=(n + 2) * 2.0 ** -23, atol=0) and not s[:3].any()


def test_moment_of_one_loaded_triangle_by_hand():
    """centre (2, 3, 5) + offset (1, -1, 0.5) - moment centre (0.5, 1, 1.5) = arm (2.5, 1, 4); normal (0, 0, 1), area 2, p = 4, tau =
    (0.5, 0, 0): dF = (1, 0, -8); M = r x dF = (1 * -8 - 4 * 0, 4 * 1 - 2.5 * -8, 2.5 * 0 - 1 * 1) = (-8, 24, -1)"""
    mesh = fc.mesh_of([(2.0, 3.0, 5.0)], [(0.0, 0.0, 1.0)], areas=[2.0])
    params = fc.params((1.0, -1.0, 0.5), moment_center=(0.5, 1.0, 1.5))
    one = lambda v: np.array([v], F32)
    s = forces.partial_force_sums(mesh, one(4.0), one(0.5), one(0.0), one(0.0), params)
    assert s.tolist() == [0.0, 0.0, -8.0, 1.0, 0.0, 0.0, -8.0, 24.0, -1.0]
    c, cov = forces.force_series_contributions(mesh, one(4.0), one(0.5), one(0.0), one(0.0), params)
    assert c[0].tolist() == s.tolist() and cov == 1 and np.signbit(c[0, 0]) and np.signbit(c[0, 1])      # (-p) * 0 is -0.0
    want = ref.contributions(one(4.0), np.array([[0.5, 0.0, 0.0]], F32), mesh.centers, mesh.normals, mesh.areas, params.mesh_offset,
                             params.moment_center, np.float32)
    assert want.tobytes() == c.tobytes()
    fr = forces.finish_forces(s, cov, params, True)
    assert (fr.Fx, fr.Fz, fr.My, fr.Mx, fr.Mz) == (2.0, -16.0, 48.0, 0.0, 0.0)


# ---- the coverage threshold ----
def test_coverage_counts_the_float32_nearest_to_1e_10_as_the_reference_does():
    """pressure_scale = 0.0025165824 (float32) and rho = 1 + 2^-23 give |p| == float32(1e-10) = 1.00000001335e-10 exactly. The
    reference compares the Float32 pressure with the Float64 literal 1e-10 (src/forces/surface.jl:430): counted. A float32 comparison
    with 1e-10f does not count it. Every count of this package goes through forces.coverage_count."""
    ps = fc.threshold_pressure_scale()
    assert ps is not None and abs(float(ps) - 2.5e-3) < 1e-4
    params = fc.params(pressure_scale=ps)
    assert fc.pressure_scale_of(params) == ps
    rho = np.array([1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23, 1.0, 1.0 + 2.0 ** -22], F32)
    p, _, _ = ref.stress(rho, np.zeros((4, 3), F32), np.tile([0.0, 0.0, 1.0], (4, 1)), np.full(4, 0.5, F32), np.ones(4, bool), 0.6, ps,
                         np.float32)
    assert p[0] == F32(1e-10) and p[1] == -F32(1e-10) and p[2] == 0 and p[3] > F32(1e-10)
    assert float(p[0]) > 1e-10 and not (p[0] > F32(1e-10))
    got = forces.stress_from_cells(rho, np.zeros((4, 3), F32), np.full(4, 0.5, F32), np.ones(4, bool), np.tile([0.0, 0.0, 1.0], (4, 1)),
                                   0.6, params)
    assert got[0].tobytes() == p.tobytes()
    assert ref.coverage(p) == 3 == forces.coverage_count(p)
    mesh = fc.mesh_of([(1.0, 1.0, 1.0)] * 4, [(0.0, 0.0, 1.0)] * 4)
    z = np.zeros(4, F32)
    assert forces.force_series_contributions(mesh, p, z, z, z, params)[1] == 3
    assert forces.integrate_surface_forces(mesh, p, z, z, z, params).coverage == 3


# ---- calibration ----
def test_e_ref_census(levels, sphere, capsys):
    """prints the measured e_ref = |ref32 - ref64| / scale over every non-planted triangle and asserts that the constants recorded in
    tests/_force_ref.py are this measurement with under 10 % on top"""
    worst = {"p": 0.0, "tau": 0.0}
    excluded = total = 0
    calls = [c for c in fc.table_calls(levels) if c[0] != "planted states"]
    g, fields, mesh, params = sphere
    calls.append(("sphere", g, fields, mesh, params, 5, np.ones(322, bool)))
    for what, g, fields, mesh, params, radius, compare in calls:
        for vel_name in ("vel", "vel_temp"):
            got, r32, r64 = _evaluate(g, fields, vel_name, mesh, params, radius, None)
            e_p, e_t, _, _, ex = fc.e_ref_and_errors(got, r32, r64, compare)
            worst["p"], worst["tau"] = max(worst["p"], e_p), max(worst["tau"], e_t)
            excluded += ex
            total += int(compare.sum())
    with capsys.disabled():
        print(f"\nforce e_ref census: p {worst['p']:.3e} tau {worst['tau']:.3e} over {total} triangle evaluations, {excluded} excluded; "
              f"recorded {ref.MAX_E_REF}, margin {ref.MARGIN}")
    for k in worst:
        assert worst[k] <= ref.MAX_E_REF[k] <= 1.1 * worst[k], (k, worst[k], ref.MAX_E_REF[k])
    assert excluded == 0
