"""Warm start, host side: the state file, the map between two runs' frames and init_host, the numpy restatement of
ludwig_level_init_from_source that the device tests compare against (open_ludwig_amd/warm_start.py states the definition)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _iso_cases as ic                                    # noqa: E402
import _warm_start_cases as wc                             # noqa: E402
from open_ludwig_amd import cases, preprocess as pp, streamlines as sl, warm_start as ws      # noqa: E402
from open_ludwig_amd.blocks import build_lattice_arrays    # noqa: E402

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
IDENTITY = np.array([1, 1, 1, 0, 0, 0], F32)


@pytest.fixture(scope="module")
def tunnel():
    grids, _ = wc.small_tunnel(levels=2)
    return grids, wc.state_of(grids, offset=(1.5, -0.25, 3.0))


def test_state_file_round_trip(tunnel, tmp_path):
    _, state = tunnel
    path = os.path.join(tmp_path, ws.state_file_name(12))
    ws.save_state(path, state)
    assert os.path.basename(path) == "state_000012.npz" and os.listdir(tmp_path) == ["state_000012.npz"]
    back = ws.load_state(path)
    assert back.n_levels == state.n_levels == 2 and back.step == state.step and back.case == state.case == "test"
    assert back.u_lattice == state.u_lattice and np.array_equal(back.mesh_offset, state.mesh_offset)
    for a, b in zip(state.levels, back.levels):
        assert a["dx"] == b["dx"]
        for key, dt in (("block_pointer", np.int32), ("obstacle", np.bool_), ("rho", F32), ("vel", F32)):
            assert b[key].dtype == a[key].dtype == dt and b[key].shape == a[key].shape and np.array_equal(a[key], b[key]), key
    with np.load(path, allow_pickle=False) as z:             # numpy arrays only: nothing in the file needs pickle
        assert all(z[k].dtype != object for k in z.files)


def test_affine_map_of_an_identical_hierarchy_is_dyadic_and_unshifted(tunnel):
    grids, state = tunnel
    for li, g in enumerate(grids):
        m = ws.affine_map(state, g.dx, state.mesh_offset)
        assert m.dtype == F32 and np.array_equal(m, np.array([2.0 ** -li] * 3 + [0.0] * 3, F32))
    # two frames: a point of the STL sits at (p + off) / dx in each run
    m = ws.affine_map(state, 0.25, (0.5, 0.75, 1.0))
    assert np.array_equal(m, np.array([0.25, 0.25, 0.25, 1.0, -1.0, 2.0], F32))


def test_identity_map_copies_uncovered_cells_and_restarts_at_equilibrium(tunnel):
    grids, state = tunnel
    src = state.host_levels()
    fine_bp = grids[1].block_pointer
    for li, g in enumerate(grids):
        res = ws.init_host(g, src, ws.affine_map(state, g.dx, state.mesh_offset), 1.0, (1.0, 0.0, 0.0, 0.0))
        fluid = ~g.obstacle
        assert (res["outcome"][~fluid] == -1).all()
        if li == 0:                                          # covered: the fine level holds a block at the cell's position
            x = ic.cell_centres(g.active_block_coords).astype(np.int64)
            inside = (x[..., 0] // 4 < fine_bp.shape[0]) & (x[..., 1] // 4 < fine_bp.shape[1]) & (x[..., 2] // 4 < fine_bp.shape[2])
            covered = np.zeros(g.rho.shape, bool)
            covered[inside] = fine_bp[x[..., 0][inside] // 4, x[..., 1][inside] // 4, x[..., 2][inside] // 4] > 0
        else:
            covered = np.zeros(g.rho.shape, bool)
        own = fluid & ~covered
        assert own.any() and (res["outcome"][own] == ws.FOUND).all() and (res["source_level"][own] == li).all()
        # weights exactly 0: (1 - 0) a + 0 b = a, bit for bit
        assert np.array_equal(res["rho"][own], g.rho[own]) and np.array_equal(res["vel"][own], g.vel[own])
        n_solid = 0
        if li == 0:
            # a covered cell takes the fine level's trilinear value at its centre - the average of the fine cells around it - or, where
            # the fine cell that holds the centre is solid, the fallback: sample_host itself, asked directly
            cov = fluid & covered
            P = ((ic.cell_centres(g.active_block_coords) + 0.5)[cov]).astype(F32)
            code, q, lvl, _ = sl.sample_host(P, src)
            assert cov.any() and (lvl == 1).all() and set(code.tolist()) <= {0, 2} and (code == 0).sum() > 100
            assert np.array_equal(res["outcome"][cov], code)
            ok = code == 0
            n_solid = int((~ok).sum())
            assert np.array_equal(res["rho"][cov][ok], q[ok, 0]) and np.array_equal(res["vel"][cov][ok], q[ok, 1:4])
            assert np.array_equal(res["rho"][cov][~ok], np.ones(n_solid, F32)) and not res["vel"][cov][~ok].any()
            assert not np.array_equal(res["rho"][cov][ok], g.rho[cov][ok])
        assert np.array_equal(res["rho"][~fluid], np.ones(int((~fluid).sum()), F32)) and not res["vel"][~fluid].any()
        assert np.array_equal(res["f"], ws.equilibrium_host(res["rho"], res["vel"]))
        n_cov = int((fluid & covered).sum())
        assert res["counts"].tolist() == [int(fluid.sum()) - n_solid, 0, n_solid, 0, int(own.sum()) if li == 0 else 0,
                                          n_cov - n_solid if li == 0 else int(fluid.sum())]


def test_equilibrium_restatement_matches_the_reference_formula():
    """the float32 restatement against the formula in float64, and against cases.equilibrium (the package's own f_eq)"""
    rng = np.random.default_rng(5)
    rho = (1.0 + 0.02 * rng.standard_normal((8, 8, 8, 2))).astype(F32)
    u = (0.05 * rng.standard_normal((8, 8, 8, 2, 3))).astype(F32)
    got = ws.equilibrium_host(rho, u)
    cx, cy, cz, w, *_ = build_lattice_arrays()
    r, v = rho.astype(np.float64), u.astype(np.float64)
    cu = cx[None, None, None, None, :] * v[..., 0:1] + cy * v[..., 1:2] + cz * v[..., 2:3]
    want = r[..., None] * w.astype(np.float64) * (1.0 + 3.0 * cu + 4.5 * cu * cu - 1.5 * (v * v).sum(axis=-1)[..., None])
    assert got.dtype == F32 and np.abs(got - want).max() <= 8 * 2.0 ** -24 * np.abs(want).max()
    assert np.array_equal(got, cases.equilibrium(rho, u[..., 0], u[..., 1], u[..., 2]))
    rest = ws.equilibrium_host(np.ones(3, F32), np.zeros((3, 3), F32))
    assert np.array_equal(rest, np.broadcast_to(w, (3, 27)))


def test_linear_field_on_a_grid_one_and_a_half_times_finer():
    """a one-level source with rho and u linear in x, resampled with a = 2/3: trilinear interpolation reproduces a linear field, up to
    rounding. The bound, with u = 2^-24 the unit roundoff and M the field's largest magnitude: the stored source values carry u M; a
    lerp (1 - w) a + w b rounds 1 - w (u M), its two products (u M together, the weights summing to 1) and its sum (u M): 3 u M, three
    lerps 9 u M; the position P = a (gc + 0.5) + b is rounded twice and g = P - 0.5 once, 3 u P_max cells, times the slope."""
    coords, _ = ic.block_grid(3, 3, 3)
    g = cases.make_level(1, coords, (3, 3, 3), 0.6)
    x = ic.cell_centres(coords)[..., 0] + 0.5
    slopes = {"rho": (1.0, 0.002), "ux": (0.03, 0.0015), "uy": (-0.01, 0.0004), "uz": (0.002, -0.0001)}
    rho = np.asfortranarray((slopes["rho"][0] + slopes["rho"][1] * x).astype(F32))
    vel = np.asfortranarray(np.stack([(slopes[k][0] + slopes[k][1] * x) for k in ("ux", "uy", "uz")], axis=-1).astype(F32))
    src = sl.host_levels([g], lambda li: (rho, vel))
    dcoords, _ = ic.block_grid(4, 4, 4)
    dst = cases.make_level(1, dcoords, (4, 4, 4), 0.6)
    m = np.array([1.0 / 1.5] * 3 + [1.0] * 3, F32)
    res = ws.init_host(dst, src, m, 1.0, (1.0, 0.0, 0.0, 0.0))
    assert res["counts"].tolist() == [32 ** 3, 0, 0, 0, 32 ** 3]
    P = ws.cell_positions(dst, m).astype(np.float64)
    assert P.min() > 1.0 and P.max() < 23.0                  # every stencil inside the source: no corner is replaced
    u = 2.0 ** -24
    for k, name in enumerate(("rho", "ux", "uy", "uz")):
        c0, c1 = slopes[name]
        got = res["rho"] if k == 0 else res["vel"][..., k - 1]
        want = c0 + c1 * P[..., 0]
        M = np.abs(want).max()
        bound = 10 * u * M + 3 * u * 24.0 * abs(c1)
        err = np.abs(got - want).max()
        print(f"{name}: max error {err:.3e}, bound {bound:.3e} ({err / (u * M):.2f} u M)")
        assert err <= bound, (name, err, bound)


def test_shifted_map_counts_every_outcome_cell_by_cell():
    src = wc.planted_nest()
    coords = [(1, 1, 1), (2, 1, 1), (3, 1, 1), (2, 2, 2)]
    dst = cases.make_level(1, coords, (3, 2, 2), 0.6)
    dst.obstacle[2:4, 3, 4, 1] = True
    m = np.array([0.75, 0.75, 0.75, -3.1, 2.3, 1.7], F32)
    res = ws.init_host(dst, src, m, 0.5, wc.NEST_FALLBACK)
    c = res["counts"]
    fluid = ~dst.obstacle
    assert c[:4].sum() == fluid.sum() == 4 * 512 - 2 and (c[:4] > 0).all() and (c[4:] > 0).all() and c[4:].sum() == c[0]
    # cell by cell: every point on its own through sample_host
    P = ws.cell_positions(dst, m)
    n = np.zeros(4, np.int64)
    per_level = np.zeros(2, np.int64)
    for idx in np.ndindex(*dst.rho.shape):
        if dst.obstacle[idx]:
            assert res["rho"][idx] == 1.0 and not res["vel"][idx].any()
            continue
        code, q, li, _ = sl.sample_host(P[idx][None, :], src)
        k = int(code[0]) if code[0] != 0 else (ws.FOUND if np.isfinite(q[0]).all() else ws.NON_FINITE)
        n[k] += 1
        assert res["outcome"][idx] == k
        if k == ws.FOUND:
            per_level[li[0]] += 1
        else:
            assert res["rho"][idx] == F32(wc.NEST_FALLBACK[0]) and np.array_equal(res["vel"][idx], np.array(wc.NEST_FALLBACK[1:], F32))
    assert n.tolist() == c[:4].tolist() and per_level.tolist() == c[4:].tolist()
    assert np.isfinite(res["f"]).all() and np.array_equal(res["f"], ws.equilibrium_host(res["rho"], res["vel"]))


def test_velocity_scale_halves_u_and_quarters_the_density_fluctuation():
    g = cases.make_level(1, [(1, 1, 1)], (1, 1, 1), 0.6)
    rng = np.random.default_rng(3)
    rho = np.asfortranarray((1.0 + rng.integers(-64, 65, (8, 8, 8, 1)) * 2.0 ** -10).astype(F32))
    vel = np.asfortranarray((rng.integers(-256, 257, (8, 8, 8, 1, 3)) * 2.0 ** -12).astype(F32))
    res = ws.init_host(g, sl.host_levels([g], lambda li: (rho, vel)), IDENTITY, 0.5, (1.0, 0.0, 0.0, 0.0))
    assert res["counts"].tolist() == [512, 0, 0, 0, 512]
    assert np.array_equal(res["vel"], vel / F32(2.0)) and np.array_equal(res["rho"] - F32(1.0), (rho - F32(1.0)) / F32(4.0))


def test_config_keys_default_to_nothing_and_are_checked():
    base = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"))
    assert not base.state_files_enabled and base.initial_condition_state == "" and base.initial_condition_first_step == 1
    cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), {"advanced": {
        "state_files": {"enabled": True, "interval": 8},
        "initial_condition": {"state": "out/state_000016.npz", "first_step": 17, "velocity_scale": 0.5}}})
    assert cfg.state_files_enabled and cfg.state_files_interval == 8
    assert (cfg.initial_condition_state, cfg.initial_condition_first_step, cfg.initial_condition_velocity_scale) == ("out/state_000016.npz", 17, 0.5)
    assert ws.resolve_state_path(cfg.initial_condition_state, cfg.case_dir) == os.path.join(G, "out", "state_000016.npz")
    auto = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), {"advanced": {"initial_condition": {"state": "s.npz"}}})
    assert auto.initial_condition_velocity_scale is None
    for bad in ({"state_files": {"enabled": True, "interval": -1}}, {"initial_condition": {"first_step": 3}},
                {"initial_condition": {"state": "s.npz", "first_step": 0}}, {"initial_condition": {"state": "s.npz", "velocity_scale": 0.0}},
                {"initial_condition": {"state": "s.npz", "velocity_scale": "fast"}}):
        with pytest.raises(ValueError, match="advanced\\.(state_files|initial_condition)"):
            pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), {"advanced": bad})


def test_steppers_without_the_device_path_name_the_key(tmp_path):
    """the oracle stepper offers no init_from and the distributed one refuses: both errors name the YAML key"""
    from _steppers import OracleStepper
    from open_ludwig_amd import case
    over = {"basic": {"num_levels": 1, "surface_resolution": 7, "simulation": {"steps": 2}},
            "advanced": {"initial_condition": {"state": "nowhere.npz"}}}
    cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), over)
    setup = pp.setup_multilevel_domain(cfg, os.path.join(G, "cube1m.stl"))
    with pytest.raises(RuntimeError, match="advanced.initial_condition"):
        case.run_case(cfg, OracleStepper, setup=setup)
    for name, key in (("init_from", "advanced.initial_condition"), ("state_files_setup", "advanced.state_files"), ("flow_source", "distributed")):
        with pytest.raises(RuntimeError, match=key):
            getattr(case.DistributedStepper, name)(None)


def test_julia_mirror_and_documents_carry_the_entry_points():
    jl = open(os.path.join(ROOT, "julia", "LudwigHIP.jl")).read()
    header = open(os.path.join(ROOT, "include", "ludwig_hip.h")).read()
    for name in ("ludwig_flow_source_create", "ludwig_flow_source_from_levels", "ludwig_flow_source_destroy", "ludwig_level_init_from_source"):
        assert name in jl and name in header, name
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert "restart at equilibrium" in text and "not bit-identical" in text and "finer source level" in text, doc
