"""The surface-force path on the device against tests/_force_ref.py, the restatement written from src/forces/surface.jl alone, on the
geometry of tests/_force_cases.py: k_map_stresses (ludwig_map_surface_stresses: the device search and wall_stress),
k_accumulate_surface_stats and k_force_chunks on plans made by forces.nearest_fluid_cells of the same cases, and case._aerodynamics.
float32 in the reference's operand order is compared bit for bit (NaN meets NaN), float64 within MARGIN * MAX_E_REF; the hand-written
cells of the table are asserted against the same restatement by tests/test_force_reference_host.py."""
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import adapt, case, force_series as fs, forces, surface_stats as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _edge_states as edge  # noqa: E402
import _force_cases as fc  # noqa: E402
import _force_ref as ref  # noqa: E402
import _step_ref  # noqa: E402

F32 = np.float32
U = F32(0.05)
ORDER_SWITCH = "LUDWIG_REFERENCE_BLOCK_ORDER"


def _device(g, fields):
    d = adapt(g, 0)
    try:
        for k, v in fields.items():
            d.upload(k, v)
    except Exception:
        d.close()
        raise
    return d


def _check_call(d, what, g, fields, mesh, params, radius, compare, tau=None, dx=None):
    """ludwig_map_surface_stresses on both velocity buffers: ref32 bit for bit, ref64 within the bound, exact +0.0 without a cell"""
    tau = g.tau if tau is None else tau
    dx = g.dx if dx is None else dx
    for vel_name in ("vel", "vel_temp"):
        r32, r64 = fc.ref_pair(g, fields, vel_name, mesh, params, radius, tau, dx)
        got = forces.map_surface_stresses_device(mesh, d, dx, tau, params, radius, vel_name)
        for name, a, b in zip(("p", "tau_x", "tau_y", "tau_z"), got, (r32.p, r32.tau[:, 0], r32.tau[:, 1], r32.tau[:, 2])):
            edge.assert_nan_aware_equal(a, b, f"{what} radius {radius} {vel_name} {name}")
        _, _, err_p, err_t, excluded = fc.e_ref_and_errors(got, r32, r64, compare)
        assert excluded <= _step_ref.MAX_EXCLUDED_SHARE * compare.sum(), (what, excluded)
        assert err_p <= ref.bound("p") and err_t <= ref.bound("tau"), (what, vel_name, err_p, err_t)
        miss = ~r32.cells.found
        for a in got:
            assert a[miss].tobytes() == np.zeros(int(miss.sum()), F32).tobytes(), what
    return r32


# ---- ludwig_map_surface_stresses on the table ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.LEVELS)
def test_device_mapping_equals_the_restatement_on_the_table(gpu, name):
    """every row of the table on its level: radii 0, 1, 5, 16, the mesh offset, centres outside the domain, in absent blocks, about
    1000 cells away, on faces and at equal distances; and every row again at the radii it does not name"""
    g = fc.build_level(name)
    fields = fc.random_fields(g)
    d = _device(g, fields)
    try:
        for (radius, offset), rows in fc.groups(name).items():
            mesh = fc.mesh_of([r.centre for r in rows], fc.row_normals(len(rows)))
            r32 = _check_call(d, name, g, fields, mesh, fc.params(offset), radius, np.array([not r.tie for r in rows]))
            want = [r.expect for r in rows]
            got = [(int(r32.cells.block[i]), *map(int, r32.cells.local[i])) if r32.cells.found[i] else None for i in range(len(rows))]
            assert got == want                                       # what was compared bit for bit read the hand-written cells
        rows = [r for r in fc.ROWS if r.level == name and r.offset == fc.NO_OFFSET]
        mesh = fc.mesh_of([r.centre for r in rows], fc.row_normals(len(rows)))
        for radius in (0, 1, 5, 16):
            _check_call(d, name + " all rows", g, fields, mesh, fc.params(), radius, np.array([not r.tie for r in rows]))
    finally:
        d.close()


@pytest.mark.gpu
def test_device_mapping_of_the_planted_states_and_the_non_dyadic_spacing(gpu):
    """u parallel to the normal, |u_t| below / at / above 1.0f-10, rho = 1 and its float32 neighbours, NaN and Inf, at the level's tau,
    tau = 0.5 (nu = 0) and tau = 0.500001; and the base cell that is not the nearest at dx = float32(0.1)"""
    g = fc.build_level("full")
    states = fc.planted_states()
    fields, mesh = fc.plant(g, fc.random_fields(g), states)
    compare = np.array([s.ref64 for s in states])
    d = _device(g, fields)
    try:
        for tau in (None, 0.5, 0.500001):
            r32 = _check_call(d, f"planted states tau {tau}", g, fields, mesh, fc.params(), 5, compare, tau=tau)
            assert r32.cells.found.all() and (np.nan_to_num(r32.tau).any() == (tau != 0.5))      # nu = 0: zeros, or NaN where rho is not finite
        one = fc.mesh_of([fc.NON_DYADIC_CENTRE], fc.row_normals(1))
        dx = float(F32(fc.NON_DYADIC_DX))
        r32 = _check_call(d, "non-dyadic", g, fields, one, fc.params(), 5, np.zeros(1, bool), dx=dx)
        assert (int(r32.cells.block[0]), *map(int, r32.cells.local[0])) == fc.NON_DYADIC_EXPECT
        r0 = _check_call(d, "non-dyadic", g, fields, one, fc.params(), 0, np.zeros(1, bool), dx=dx)
        assert r0.cells.base[0].tolist() == [6, 16, 3] and r0.p[0] != r32.p[0]
    finally:
        d.close()


# ---- stepped levels, block orders ----
def _sphere_devices(monkeypatch, reference_order):
    if reference_order:
        monkeypatch.setenv(ORDER_SWITCH, "1")
    else:
        monkeypatch.delenv(ORDER_SWITCH, raising=False)
    grids, sparams, mesh, params = fc.sphere_case()
    st = case.HipStepper(grids, upload_state=True)
    return grids, sparams, mesh, params, st


@pytest.mark.gpu
def test_device_mapping_after_odd_and_even_coarse_steps(gpu, monkeypatch):
    """the 2-level tunnel after 3 and after 4 coarse steps (rho as the step left it, possibly elided until read): the mapping comes
    first, the fields it is compared on are downloaded afterwards"""
    grids, sparams, mesh, params, st = _sphere_devices(monkeypatch, False)
    g = grids[1]
    try:
        t = 1
        for n in (3, 1):
            st.batch(t, n, U, sparams)
            t += n
            got = {v: forces.map_surface_stresses_device(mesh, st.dev[1], g.dx, g.tau, params, 5, v) for v in ("vel", "vel_temp")}
            fields = {k: st.field(1, k) for k in ("rho", "vel", "vel_temp")}
            assert not np.array_equal(fields["vel"], fields["vel_temp"])
            for v in ("vel", "vel_temp"):
                r32, r64 = fc.ref_pair(g, fields, v, mesh, params, 5, g.tau)
                for name, a, b in zip(("p", "tau_x", "tau_y", "tau_z"), got[v], (r32.p, r32.tau[:, 0], r32.tau[:, 1], r32.tau[:, 2])):
                    edge.assert_nan_aware_equal(a, b, f"after {t - 1} steps {v} {name}")
                _, _, err_p, err_t, excluded = fc.e_ref_and_errors(got[v], r32, r64, np.ones(322, bool))
                assert excluded <= _step_ref.MAX_EXCLUDED_SHARE * 322 and err_p <= ref.bound("p") and err_t <= ref.bound("tau")
                assert np.count_nonzero(got[v][0]) == 322 and np.abs(got[v][1]).max() > 0
    finally:
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["reference_order", "shuffled"])
def test_the_block_order_is_invisible_to_the_mapping(gpu, monkeypatch, how):
    g = fc.build_level("holes")
    fields = fc.random_fields(g)
    if how == "reference_order":
        monkeypatch.setenv(ORDER_SWITCH, "1")
    else:
        monkeypatch.delenv(ORDER_SWITCH, raising=False)
    d = _device(g, fields)
    try:
        if how == "shuffled":
            d.set_order(np.random.default_rng(3).permutation(8 * g.n_blocks).astype(np.int32))
        rows = [r for r in fc.ROWS if r.level == "holes"]
        mesh = fc.mesh_of([r.centre for r in rows], fc.row_normals(len(rows)))
        _check_call(d, how, g, fields, mesh, fc.params(), 16, np.array([not r.tie for r in rows]))
    finally:
        d.close()


# ---- surface statistics and force series on real plans ----
def _plan_cases():
    """(what, level, fields, mesh, params): the radius-5 rows of every level, the planted states, and the coverage threshold"""
    for name in fc.LEVELS:
        g = fc.build_level(name)
        rows = [r for r in fc.ROWS if r.level == name and r.offset == fc.NO_OFFSET]
        yield name, g, fc.random_fields(g), fc.mesh_of([r.centre for r in rows], fc.row_normals(len(rows)),
                                                       areas=[0.125 * (1 + i) for i in range(len(rows))]), fc.params()
    g = fc.build_level("full")
    states = fc.planted_states()
    fields, mesh = fc.plant(g, fc.random_fields(g), states)
    yield "planted states", g, fields, mesh, fc.params()
    ps = fc.threshold_pressure_scale()
    assert ps is not None
    fields, mesh = fc.plant(g, fc.random_fields(g), states[6:9])                   # rho = 1, 1 - 2^-23, 1 + 2^-23
    yield "coverage threshold", g, fields, mesh, fc.params(pressure_scale=ps)


def _expected_samples(g, fields, mesh, params, plan):
    """per velocity buffer: the restatement's float32 (p, tau) on the plan's cells, |tau| in the statistics' float32 order, the nine
    contributions and the coverage count"""
    out = {}
    for v in ("vel", "vel_temp"):
        r32, _ = fc.ref_pair(g, fields, v, mesh, params, 5, g.tau)
        assert np.array_equal(r32.cells.found, plan.found) and np.array_equal(np.where(r32.cells.found, r32.cells.block, -1), plan.blocks)
        assert np.array_equal(r32.cells.local[:, 0] + 8 * r32.cells.local[:, 1] + 64 * r32.cells.local[:, 2], plan.cells)
        assert r32.cells.wall_dist.tobytes() == plan.wall_dist.tobytes()
        with np.errstate(all="ignore"):
            t = r32.tau
            mag = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]).astype(F32)
            contrib = ref.contributions(r32.p, r32.tau, mesh.centers, mesh.normals, mesh.areas, params.mesh_offset, params.moment_center,
                                        np.float32)
        out[v] = (r32.p, t, mag, contrib, ref.coverage(r32.p))
    return out


@pytest.mark.gpu
def test_surface_statistics_and_force_series_on_plans_of_the_table(gpu):
    """DeviceSurfaceStats and DeviceForceSeries built from forces.nearest_fluid_cells of the table's cases, one sample on vel (odd
    sub-step) and one on vel_temp (even): the restatement's float32 values pushed through the documented float64 orders - sequential
    per triangle for the statistics, forces.tree_sum_f64 over the triangles for the series - and the reference's coverage count.
    In the "coverage threshold" case |p| of one triangle is float32(1e-10) exactly: the reference's Float64 comparison counts it."""
    for what, g, fields, mesh, params in _plan_cases():
        plan = ss.plan_surface(mesh, g, params)
        want = _expected_samples(g, fields, mesh, params, plan)
        d = _device(g, fields)
        S = F = None
        try:
            S = ss.DeviceSurfaceStats(plan, d, 0, g.tau, params)
            F = fs.from_mesh(mesh, plan, d, 0, g.tau, params, capacity=2)
            for t_sub in (3, 4):
                S.accumulate(t_sub)
                F.sample(t_sub, t_sub)
            sums, n = S.download()
            steps, rec, cov = F.download()
        finally:
            for h in (S, F):
                if h is not None:
                    h.close()
            d.close()
        assert n == 2 and steps.tolist() == [3, 4]
        acc = np.zeros((7, plan.n))
        with np.errstate(all="ignore"):
            for v in ("vel", "vel_temp"):
                p, t, mag, _, _ = want[v]
                p, t, mag = p.astype(np.float64), t.astype(np.float64), mag.astype(np.float64)
                for k, term in enumerate((p, p * p, t[:, 0], t[:, 1], t[:, 2], mag, mag * mag)):
                    acc[k] = acc[k] + term
        edge.assert_nan_aware_equal(sums, acc, f"{what}: surface statistics")
        for i, v in enumerate(("vel", "vel_temp")):
            contrib, covered = want[v][3], want[v][4]
            with np.errstate(all="ignore"):
                tree = np.array([forces.tree_sum_f64(contrib[:, k].astype(np.float64)) for k in range(9)])
            edge.assert_nan_aware_equal(rec[i], tree, f"{what}: force series record on {v}")
            assert int(cov[i]) == covered, (what, v, int(cov[i]), covered)
        if what == "coverage threshold":
            p = want["vel"][0]
            assert p[2] == F32(1e-10) and p[1] == -F32(1e-10) and p[0] == 0 and want["vel"][4] == 2
        if what == "planted states":
            assert np.isnan(rec).any() and want["vel"][4] < plan.n


# ---- case._aerodynamics ----
@pytest.mark.gpu
@pytest.mark.parametrize("symmetric", [False, True])
def test_aerodynamics_against_the_float64_finish_of_the_restatement(gpu, monkeypatch, symmetric):
    """Cd, Cl, Cs, Cmx, Cmy, Cmz, the forces, moments and the pressure / viscous split of case._aerodynamics after 3 coarse steps of the
    2-level tunnel, against the restatement's finish of the float64 sums of its float32 contributions: within the first-order bound
    of a float32 sum of n terms (doubled where the symmetry table doubles)"""
    grids, sparams, mesh, params, st = _sphere_devices(monkeypatch, False)
    g = grids[1]
    try:
        st.batch(1, 3, U, sparams)
        fr = case._aerodynamics(st, grids, mesh, params, symmetric)
        fields = {k: st.field(1, k) for k in ("rho", "vel")}
    finally:
        st.close()
    r32, _ = fc.ref_pair(g, fields, "vel", mesh, params, 5, g.tau)
    contrib = ref.contributions(r32.p, r32.tau, mesh.centers, mesh.normals, mesh.areas, params.mesh_offset, params.moment_center, np.float32)
    want = ref.finish(ref.sums(contrib), symmetric, params.rho_physical, params.u_physical, params.reference_area, params.reference_chord)
    b = fc.first_order_bound(contrib)
    k = 2.0 if symmetric else 1.0
    f_ref = 0.5 * params.rho_physical * params.u_physical ** 2 * params.reference_area
    m_ref = f_ref * params.reference_chord
    tol = {"Fx_pressure": k * b[0], "Fy_pressure": b[1], "Fz_pressure": k * b[2], "Fx_viscous": k * b[3], "Fy_viscous": b[4],
           "Fz_viscous": k * b[5], "Fx": k * (b[0] + b[3]), "Fy": b[1] + b[4], "Fz": k * (b[2] + b[5]), "Mx": b[6], "My": k * b[7], "Mz": b[8]}
    tol.update(Cd=tol["Fx"] / f_ref, Cl=tol["Fz"] / f_ref, Cs=tol["Fy"] / f_ref, Cmx=tol["Mx"] / m_ref, Cmy=tol["My"] / m_ref,
               Cmz=tol["Mz"] / m_ref)
    assert f_ref > 1e-10 and m_ref > 1e-10 and set(tol) == set(want)
    for name, t in tol.items():
        got = getattr(fr, name)
        print(f"{name}: got {got!r} want {want[name]!r} |diff| {abs(got - want[name]):.3e} bound {t:.3e}")
        assert abs(got - want[name]) <= t, (name, got, want[name], t)
    if symmetric:
        assert fr.Fy == 0.0 and fr.Mx == 0.0 and fr.Mz == 0.0 and fr.Cs == 0.0
    else:
        assert min(abs(want[n]) for n in ("Cd", "Cl", "Cs", "Cmx", "Cmy", "Cmz", "Fx_viscous")) > 0
    assert fr.coverage == ref.coverage(r32.p) == 322
