"""The subgrid observer on the host: the restatement the device is checked against (tests/_subgrid_ref.py) is tied to the step's own
WALE branch (tests/_step_ref.py), the GPU test's inputs reach every branch code, subgrid.finalize and the configuration keys."""
import os

import numpy as np
import pytest

import _step_ref as sr
import _step_ref_cases as src_cases
import _subgrid_cases as sc
import _subgrid_ref as ref
from oracle import oracle
from open_ludwig_amd import case, preprocess as pp, subgrid
from _steppers import OracleStepper

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


# ---- 1. the restatement reports the step's nu_t ----
@pytest.mark.parametrize("name", ["box3_rough", "tunnel_L2_t1_b1_s1_w1_n0_z0"])
def test_codes_are_the_branches_the_next_sub_step_takes(name):
    """The velocity a level holds after coarse step t is what its first sub-step of coarse step t + 1 reads as vel_in. The code
    the restatement gives on that buffer must be the WALE branch the step reference (float32 run) records for that sub-step: code >= 1
    where it flags OP1, code >= 2 where it flags denom, code 3 where it flags the eddy viscosity above the background - cell for cell,
    after an odd and after an even coarse step, over the fluid cells."""
    c = src_cases.CASES[name]
    grids, params = c.build()
    seen = np.zeros(4, dtype=np.int64)
    for t in (1, 2, 3):
        if t > 1:
            oracle.execute_timestep_batch(grids, t - 1, 1, F32(c.u), params)       # the state after coarse step t - 1
        res = sr.coarse_step(grids, params, t, c.u, np.float32)
        for lv, g in enumerate(grids):
            vel_in = sr._buffers((1 << lv) * t)[2]                                 # what the level's first sub-step of step t reads
            _, _, code = ref.state(getattr(g, vel_in), g.neighbor_table, params.c_wale, params.nu_sgs_bg)
            br = res[lv].branches[0]
            fluid = ~np.asarray(g.obstacle).astype(bool)       # the step records no branch in a solid cell, the observer reports none
            for least, bit in ((1, sr.WALE_OP1), (2, sr.WALE_DENOM), (3, sr.WALE_EDDY)):
                assert np.array_equal((code >= least)[fluid], ((br & bit) != 0)[fluid]), f"{name} step {t} level {lv + 1}: code >= {least}"
            seen += np.bincount(code[fluid].ravel(), minlength=4)
    assert seen[3] > 0 and seen[:3].sum() > 0, seen


def test_restatement_agrees_with_a_literal_single_cell_evaluation():
    """the vectorised restatement against the formula written out once more for single cells in Python float32 scalars"""
    grids, params, vel = sc.uploaded_box("box27")
    g = grids[0]
    nu, s2, code = ref.state(vel, g.neighbor_table, params.c_wale, params.nu_sgs_bg)
    import _gradient_ref as gref
    rng = np.random.default_rng(3)
    for _ in range(60):
        x, y, z, b = (int(v) for v in rng.integers(0, (8, 8, 8, g.n_blocks)))
        gm = np.empty((3, 3), dtype=F32)
        for j, d in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
            hi = gref.neighbor_value(vel, g.neighbor_table, x, y, z, b, *d)
            lo = gref.neighbor_value(vel, g.neighbor_table, x, y, z, b, *(-k for k in d))
            gm[:, j] = F32(0.5) * (hi - lo)
        with np.errstate(all="ignore"):
            one = ref.wale_state([[gm[i, j].reshape(1) for j in range(3)] for i in range(3)], params.c_wale, params.nu_sgs_bg)
        for got, want in zip((nu, s2, code), one):
            a, w = np.asarray(got[x, y, z, b]), np.asarray(want[0])
            assert (np.isnan(a) and np.isnan(w)) or a.tobytes() == w.tobytes(), (x, y, z, b)


# ---- 2. the GPU test's inputs reach every code ----
def test_uploaded_boxes_reach_every_code():
    total = np.zeros(4, dtype=np.int64)
    for name, want in (("one_block", (0, 1, 2, 3)), ("three_in_an_L", (0, 1, 2)), ("box27", (0, 1, 2, 3))):
        grids, params, vel = sc.uploaded_box(name)
        g = grids[0]
        nu, s2, code = ref.state(vel, g.neighbor_table, params.c_wale, params.nu_sgs_bg)
        fluid = ~g.obstacle
        counts = np.bincount(code[fluid].ravel(), minlength=4)
        for k in want:
            assert counts[k] > 0, (name, k, counts)
        total += counts
        assert g.obstacle.any() and np.isnan(vel).sum() == 1 and np.isinf(vel).sum() == 2
        # the step's rule at a non-finite velocity: OP1 is NaN, the model is not evaluated, nu_t is the background value
        bad = ~np.isfinite(s2)
        assert bad.any() and np.isfinite(nu).all()
        assert (nu[bad] == F32(params.nu_sgs_bg)).all() and (code[bad] == ref.NO_OP1).all()
        # the floor: code 2 holds exactly nu_bg, code 3 is above it
        assert (nu[code == ref.FLOOR] == F32(params.nu_sgs_bg)).all() and (nu[code == ref.MODEL] > F32(params.nu_sgs_bg)).all()
    assert (total > 0).all(), total
    grids, params, vel = sc.uploaded_box("three_in_an_L")
    assert params.nu_sgs_bg == 0.05                            # the background value above the model's: where code 2 comes from
    _, _, low = ref.state(vel, grids[0].neighbor_table, params.c_wale, 0.0005)
    assert (low == ref.MODEL).any()


def test_restated_sums_are_sequential_float64():
    grids, params, vel = sc.uploaded_box("one_block")
    g = grids[0]
    sums = ref.zero_sums(1)
    for scale in (1.0, 0.5, 2.0):
        ref.accumulate(sums, vel * F32(scale), g.neighbor_table, g.obstacle, params.c_wale, params.nu_sgs_bg)
    want = np.zeros(3)
    cell = (1, 3, 4, 0)
    assert not g.obstacle[cell]
    for scale in (1.0, 0.5, 2.0):
        nu, s2, _ = ref.state(vel * F32(scale), g.neighbor_table, params.c_wale, params.nu_sgs_bg)
        n, e = float(nu[cell]), float(s2[cell])
        want += (n, n * n, n * e)
    assert [s[cell] for s in sums] == list(want)
    assert all((s[g.obstacle] == 0).all() for s in sums)


# ---- 3. finalize ----
def test_finalize_formulas():
    nu = 0.002
    s_nu, s_nunu, s_eps = np.array([0.04, 0.0, 0.03]), np.array([0.0005, 0.0, 0.0003]), np.array([8e-6, 0.0, 4e-6])
    tke = np.array([3e-4, 0.0, 0.0])
    out = subgrid.finalize(s_nu, s_nunu, s_eps, 4, nu, c_k=0.1, resolved_tke=tke)
    mean, mean2 = s_nu / 4, s_nunu / 4
    assert np.array_equal(out["nu_ratio_mean"], mean / nu)
    assert np.array_equal(out["nu_ratio_rms"], np.sqrt(np.maximum(mean2 - mean * mean, 0.0)) / nu)
    assert np.array_equal(out["k_sgs"], mean2 / 0.1 ** 2) and out["k_sgs"][0] == 0.000125 / 0.1 ** 2
    assert np.array_equal(out["eps_sgs"], s_eps / 4)
    assert out["resolved_share"][0] == tke[0] / (tke[0] + out["k_sgs"][0])
    assert out["resolved_share"][1] == 1.0                     # k = k_sgs = 0
    assert out["resolved_share"][2] == 0.0                     # nothing resolved
    assert all(v.dtype == np.float64 for v in out.values())
    # <nu^2> - <nu>^2 = 0.00999997 - 0.01 < 0 (sums that rounding left inconsistent): the rms clamps at 0
    neg = subgrid.finalize(np.array([0.3]), np.array([0.0299999]), np.array([0.0]), 3, nu)
    assert neg["nu_ratio_rms"][0] == 0.0 and "resolved_share" not in neg
    assert subgrid.finalize(s_nu, s_nunu, s_eps, 4, nu)["k_sgs"][0] == 0.000125 / subgrid.DEFAULT_CK ** 2 and subgrid.DEFAULT_CK == 0.094


def test_finalize_without_samples_is_nan():
    z = np.zeros((2, 2))
    out = subgrid.finalize(z, z, z, 0, 0.002, resolved_tke=np.full((2, 2), np.nan))
    assert all(np.isnan(v).all() for v in out.values()) and set(out) == {k for _, k in subgrid.MEAN_ARRAYS}


def test_level_viscosity_is_the_wall_shear_expression():
    from open_ludwig_amd import forces
    for tau in (0.5006, 0.5003, 0.50015):
        assert subgrid.level_viscosity(tau) == (F32(tau) - F32(0.5)) / F32(3.0) == forces.lattice_viscosity(tau)
    assert subgrid.level_viscosity(0.5006).dtype == F32
    nu_t = np.array([0.0005, 0.002], dtype=F32)
    r = subgrid.ratio_field(nu_t, 0.5006)
    assert r.dtype == F32 and np.array_equal(r, nu_t / subgrid.level_viscosity(0.5006))


# ---- 4. configuration ----
def _load(over):
    return pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), over)


def test_configuration_keys_and_defaults():
    base = _load(None)
    assert "EddyViscosityRatio" not in base.output_fields and base.statistics_subgrid is False and base.statistics_subgrid_ck == 0.094
    off = _load({"basic": {"simulation": {"output_fields": {"eddy_viscosity": False}}},
                 "advanced": {"statistics": {"enabled": True, "subgrid": False}}})
    assert off.output_fields == base.output_fields and off.statistics_subgrid is False
    on = _load({"basic": {"simulation": {"output_fields": {"eddy_viscosity": True, "vorticity": True}}},
                "advanced": {"statistics": {"enabled": True, "subgrid": True, "subgrid_ck": 0.1}}})
    assert on.output_fields == base.output_fields + ("Vorticity", "EddyViscosityRatio")
    assert on.statistics_subgrid is True and on.statistics_subgrid_ck == 0.1 and on.statistics_enabled


def test_subgrid_without_statistics_is_refused_by_key_name():
    for stats in ({"subgrid": True}, {"subgrid": True, "enabled": False}):
        with pytest.raises(ValueError, match=r"advanced\.statistics\.subgrid"):
            _load({"advanced": {"statistics": stats}})
    with pytest.raises(ValueError, match=r"advanced\.statistics\.subgrid_ck"):
        _load({"advanced": {"statistics": {"enabled": True, "subgrid": True, "subgrid_ck": 0.0}}})


def test_a_stepper_without_the_device_entry_points_raises_and_names_the_feature():
    for over, key in (({"basic": {"simulation": {"output_fields": {"eddy_viscosity": True}}}}, "eddy_viscosity"),
                      ({"advanced": {"statistics": {"enabled": True, "subgrid": True}}}, "advanced.statistics.subgrid")):
        cfg = _load(dict(over, basic=dict(over.get("basic", {}), surface_resolution=25)))
        setup = pp.setup_multilevel_domain(cfg, os.path.join(G, "ball1m.stl"))
        with pytest.raises(RuntimeError, match=key):
            case.run_case(cfg, OracleStepper, steps=1, setup=setup)
