"""The edge-state catalogue (tests/_edge_states.py) on the CPU oracle alone.

1. Census: after one step every entry shows the output signature of the branch it targets (counts of rho == 0.01f, subnormals, the
   NaN set, ...), so the GPU comparison in tests/test_gpu_edge_states.py cannot quietly turn into a smooth-state test.
2. The oracle against expectations derived from the reference's expressions, not from the oracle.
"""
import dataclasses

import numpy as np
import pytest

import _edge_states as es
from oracle import oracle

F32 = np.float32


def one_step(entry):
    entry.steps = 1
    es.run_oracle(entry)
    g = entry.grids[0]
    return g, g.f, g.vel, g.rho                    # t_sub = 1 is odd: level 1 writes f / vel


def test_density_clamp_reaches_both_sides():
    e = es.density_clamp()
    g, f, v, r = one_step(e)
    c = e.cells
    for name in ("below", "exact", "negative"):
        assert r[c[name]] == F32(0.01), name
    assert r[c["above"]] == np.nextafter(F32(0.01), F32(1.0))
    assert int((r == F32(0.01)).sum()) == 3
    # a rest state below 0.01: rho = 0.01f and +0.0 velocity (j = 0 exactly, times 1 / 0.01)
    for name in ("below", "exact"):
        assert (v[c[name]].view(np.uint32) == 0).all(), name


def test_subnormal_velocities_survive():
    g, f, v, r = one_step(es.subnormal_state())
    assert (r == F32(0.01)).all()
    sub = es.is_subnormal(v)
    assert sub.sum() > v.size // 2, int(sub.sum())


@pytest.mark.parametrize("kind,k", [("nan", 4), ("nan", es.REST), ("+inf", 4), ("-inf", 4)])
def test_nonfinite_population_reaches_exactly_the_puller(kind, k):
    """NaN / +-Inf in population k of cell x: after one step exactly cell x + c_k is not finite. Reference: only that cell pulls it,
    and f_k * c_k with c = 0 is NaN (physics_kernels.jl:144-148), so its momentum, velocity and all 27 populations are NaN."""
    e = es.nonfinite_population(kind, k)
    g, f, v, r = one_step(e)
    bad = ~np.isfinite(f).all(axis=4) | ~np.isfinite(v).all(axis=4)
    assert [tuple(int(i) for i in a) for a in np.argwhere(bad)] == [e.cells["puller"]]
    assert np.isnan(f[e.cells["puller"]]).all() and not np.isfinite(v[e.cells["puller"]]).any()
    if kind == "-inf":
        # max(-Inf, 0.01): the clamp does not hide the diverged cell, u = (NaN, NaN, j_z / 0.01 = +Inf)
        assert r[e.cells["puller"]] == F32(0.01) and v[e.cells["puller"]][2] == np.inf


def test_nan_in_velocity_only_leaves_everything_finite():
    g, f, v, r = one_step(es.nan_velocity_only())
    assert np.isfinite(f).all() and np.isfinite(v).all() and np.isfinite(r).all()


@pytest.mark.parametrize("tau", [1.2, 0.8])
def test_overflowed_density_gives_nan_populations(tau):
    """rho = +Inf with zero momentum: u = 0 * (1 / Inf) = 0, f_neq = f - Inf = -Inf for every k, and the reference's Pi sums
    hold -Inf * 0 = NaN, so every population is NaN - the rest population included, whatever the sign of 1 - omega."""
    e = es.overflowed_rho(tau)
    g, f, v, r = one_step(e)
    c = e.cells["cell"]
    assert r[c] == np.inf and np.isfinite(v[c]).all()
    assert np.isnan(f[c]).all()
    bad = ~np.isfinite(f).all(axis=4)
    assert int(bad.sum()) == 1


def _wale(vel, c):
    """OP1 and denom of reference physics_kernels.jl:251-291 in float64 for an interior cell of one block."""
    x, y, z, b = c
    V = vel.astype(np.float64)
    g = np.empty((3, 3))
    for i, d in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        hi = V[x + d[0], y + d[1], z + d[2], b]
        lo = V[x - d[0], y - d[1], z - d[2], b]
        g[:, i] = 0.5 * (hi - lo)
    gsq = g @ g
    Sd = 0.5 * (gsq + gsq.T) - np.eye(3) * np.trace(gsq) / 3
    S = 0.5 * (g + g.T)
    op1, op2 = float((Sd * Sd).sum()), float((S * S).sum())
    return op1, op2 ** 2.5 + op1 ** 1.25


def _one_step_variant(build, **params):
    """f after one oracle step of a fresh entry, with solver params replaced"""
    e = build()
    e.params = dataclasses.replace(e.params, **params)
    return one_step(e)[1]


def test_wale_branches_are_reached():
    """Both OP1 <= 1e-12 and OP1 > 1e-12 with denom <= 1e-12 leave nu_eddy = 0: the output equals a run with c_wale = 0. The cell with
    larger gradients takes the eddy viscosity and differs (so the comparison can see the branch)."""
    e = es.wale_branches()
    vel_in = e.grids[0].vel_temp.copy()
    op1, den = _wale(vel_in, e.cells["small_gradient"])
    assert op1 > 1e-12 and den <= 1e-12, (op1, den)
    assert _wale(vel_in, e.cells["uniform"])[0] <= 1e-12
    op1, den = _wale(vel_in, e.cells["large_gradient"])
    assert op1 > 1e-12 and den > 1e-12
    f = one_step(e)[1]
    f0 = _one_step_variant(es.wale_branches, c_wale=0.0)
    for name in ("small_gradient", "uniform"):
        assert not es.nan_aware_diff(f[e.cells[name]], f0[e.cells[name]]).any(), name
    assert es.nan_aware_diff(f[e.cells["large_gradient"]], f0[e.cells["large_gradient"]]).any()


@pytest.mark.parametrize("tau", [0.5, 0.4999])
def test_omega_floor_is_taken(tau):
    """tau_turb = tau < 0.500001 with c_wale = nu_sgs_bg = 0: omega = 1 / 0.500001. On the off-equilibrium state the output equals,
    bit for bit, a run at tau = 0.500001 (the floor itself) and differs from a run at tau 0.5001, above the floor."""
    def run(t):
        e = es.omega_clamp(t)
        es.run_oracle(e)
        return getattr(e.grids[0], oracle.newest_buffers(0, e.steps)[0])
    f = run(tau)
    assert np.isfinite(f).all()
    assert not es.nan_aware_diff(f, run(es.OMEGA_FLOOR)).any()
    assert es.nan_aware_diff(f, run(0.5001)).sum() > f.size // 2


def test_wall_distance_edges_are_placed_next_to_near_wall_cells():
    """Each edge value shares its block with ordinary near-wall cells (so the block flag is set). wall_dist 0, negative, NaN and 10
    take no force: one step equals a run without the wall model there. The float just below 10 takes it and differs."""
    e = es.wall_distance_edges()
    g = e.grids[0]
    wd = g.wall_dist
    for name, c in e.cells.items():
        blk = wd[..., c[3]]
        others = (blk > 0) & (blk < 10)
        others[c[:3]] = False
        assert others.any(), name
    assert np.isnan(wd[e.cells["nan"]]) and wd[e.cells["below_ten"]] == F32(es.BELOW_10)
    f = one_step(e)[1]
    assert np.isfinite(f).all()
    f0 = _one_step_variant(es.wall_distance_edges, wall_model_active=False)
    for name in ("zero", "negative", "nan", "ten"):
        assert not es.nan_aware_diff(f[e.cells[name]], f0[e.cells[name]]).any(), name
    assert es.nan_aware_diff(f[e.cells["below_ten"]], f0[e.cells["below_ten"]]).any()


def test_u_mag_threshold_is_straddled():
    """u = (1e-6, 0, 0) exactly gives u_mag = 1e-6; the other cell one ulp more. Both read back from the step's output. The force the
    second one takes is below every output bit (see es.wall_umag_edges), so both equal a run without the wall model."""
    e = es.wall_umag_edges()
    f, v, r = one_step(e)[1:]
    for name, want in (("at_1e-6", F32(1e-6)), ("above_1e-6", np.nextafter(F32(1e-6), F32(1.0)))):
        c = e.cells[name]
        assert r[c] == F32(1.0) and v[c][0] == want and not v[c][1] and not v[c][2], name
        assert np.sqrt(want * want) == want                    # u_mag = sqrtf(ux * ux) is ux itself
        assert 0 < e.grids[0].wall_dist[c] < 10
    f0 = _one_step_variant(es.wall_umag_edges, wall_model_active=False)
    for c in e.cells.values():
        assert not es.nan_aware_diff(f[c], f0[c]).any()


def test_y_plus_limit_is_straddled():
    """The two cells move at u = (0.05, 0, 0) exactly (read back from the step's output) and their wall distances are adjacent floats
    at which y_p, evaluated in float32 operation by operation with the shared pow, crosses 11.81. Below the limit the power law gives
    a wall force (differs from a run without the wall model); above it the log law's u_tau leaves tau_wall < tau_res (equal)."""
    e = es.wall_y_plus_edges()
    g = e.grids[0]
    d = {n: float(g.wall_dist[c]) for n, c in e.cells.items()}
    assert np.nextafter(F32(d["y_p_below"]), F32(1.0)) == F32(d["y_p_above"])
    assert es.wall_y_plus(d["y_p_below"], 0.05, 0.5003) <= es.YP_LIMIT < es.wall_y_plus(d["y_p_above"], 0.05, 0.5003)
    f, v, r = one_step(e)[1:]
    f0 = _one_step_variant(es.wall_y_plus_edges, wall_model_active=False)
    for c in e.cells.values():
        assert r[c] == F32(1.0) and v[c][0] == F32(0.05) and not v[c][1] and not v[c][2]
    assert es.nan_aware_diff(f[e.cells["y_p_below"]], f0[e.cells["y_p_below"]]).any()
    assert not es.nan_aware_diff(f[e.cells["y_p_above"]], f0[e.cells["y_p_above"]]).any()


def test_sponge_one_replaces_the_state():
    for blend in (True, False):
        e = es.sponge_edges(blend)
        g, f, v, r = one_step(e)
        for name in ("one", "one_b"):
            c = e.cells[name]
            assert r[c] == F32(1.0) and v[c][0] == F32(0.05) and not v[c][1] and not v[c][2]


@pytest.mark.parametrize("q_min", [0.001, -1.0])
def test_bouzidi_half_and_one(q_min):
    """q == 0.5: f_out[opp] = f_post[k] (inv_2q = 1, coeff2 = 0). q == 1.0: f_out[opp] = 0.5 f_k + 0.5 f_opp."""
    e = es.bouzidi_edges(q_min)
    g = e.grids[0]
    one_step(e)
    fp, f = g.f_post_collision, g.f
    x, y, z, b, k = e.cells["half"]
    opp = 26 - k
    assert f[x, y, z, b, opp] == fp[x, y, z, b, k]
    x, y, z, b, k = e.cells["one"]
    opp = 26 - k
    assert f[x, y, z, b, opp] == F32(0.5) * fp[x, y, z, b, k] + F32(0.5) * fp[x, y, z, b, opp]
    # above 1.0, +Inf, NaN, and q <= q_min (with q_min >= 0): no correction, f_out keeps the collided value
    skipped = ["above_one", "+inf", "nan"] + (["below_qmin", "tiny_subnormal"] if q_min >= 0 else [])
    for name in skipped:
        x, y, z, b, k = e.cells[name]
        assert f[x, y, z, b, 26 - k] == fp[x, y, z, b, 26 - k], name
    # q < 0.5: 2q f_k + (1 - 2q) f_ff with f_ff at x + c_opp(k) (all these cells lie inside their block or off the level)
    half_bits = dict(es.Q_EDGE_HALVES, behind_off_level=0x3266)
    below = ["below_half", "at_or_above_qmin", "behind_off_level"] + (["below_qmin", "tiny_subnormal"] if q_min < 0 else [])
    for name in below:
        x, y, z, b, k = e.cells[name]
        q = F32(np.array(half_bits[name], np.uint16).view(np.float16))
        nx, ny, nz = x - es.CX[k], y - es.CY[k], z - es.CZ[k]
        inside = all(0 <= c <= 7 for c in (nx, ny, nz))
        if name == "behind_off_level":
            assert not inside
        if not inside and name != "behind_off_level":
            continue
        f_k = fp[x, y, z, b, k]
        f_ff = fp[nx, ny, nz, b, k] if inside else f_k
        want = F32(2.0) * q * f_k + (F32(1.0) - F32(2.0) * q) * f_ff
        assert f[x, y, z, b, 26 - k] == want, name
    # q > 0.5: (1 / 2q) f_k + ((2q - 1) / 2q) f_opp
    x, y, z, b, k = e.cells["above_half"]
    q = F32(np.array(es.Q_EDGE_HALVES["above_half"], np.uint16).view(np.float16))
    inv = F32(1.0) / (F32(2.0) * q)
    want = inv * fp[x, y, z, b, k] + ((F32(2.0) * q - F32(1.0)) * inv) * fp[x, y, z, b, 26 - k]
    assert f[x, y, z, b, 26 - k] == want
    assert np.isfinite(f).all()


def test_bouzidi_qmin_neighbours_straddle_the_threshold():
    lo, hi = es.Q_EDGE_HALVES["below_qmin"], es.Q_EDGE_HALVES["at_or_above_qmin"]
    as_f = lambda bits: float(np.array(bits, np.uint16).view(np.float16))
    assert as_f(lo) <= float(F32(0.001)) < as_f(hi)


@pytest.mark.parametrize("kind", ["parent_half", "ratio_low", "ratio_high"])
def test_interface_rescaling_edges_stay_finite(kind):
    tp, tc = {"parent_half": (0.5, 0.5003), "ratio_low": (0.6, 0.500001), "ratio_high": (0.5001, 0.6)}[kind]
    tau_c, tau_f = F32(tp) - F32(0.5), F32(tc) - F32(0.5)
    if kind == "parent_half":
        assert not tau_c > F32(1e-6)
    else:
        ratio = tau_f / tau_c
        assert (ratio < F32(0.01)) if kind == "ratio_low" else (ratio > F32(100.0))
    e = es.interface_edges(kind, True)
    es.run_oracle(e)
    for i, g in enumerate(e.grids):
        assert np.isfinite(getattr(g, oracle.newest_buffers(i, e.steps)[0])).all()


def test_interface_nan_parent_reaches_the_child():
    for temporal in (True, False):
        e = es.interface_edges("nan_parent", temporal)
        es.run_oracle(e)
        child = e.grids[1]
        assert np.isnan(getattr(child, oracle.newest_buffers(1, e.steps)[0])).any()


def test_nan_aware_comparison():
    a = np.array([0.0, -0.0, np.nan, 1.0, es.TINY_SUBNORMAL], np.float32)
    b = np.array([0.0, 0.0, -np.nan, 1.0, 0.0], np.float32)
    assert es.nan_aware_diff(a, b).tolist() == [False, True, False, False, True]
    nan_gpu = np.array([0x7FC00000], np.uint32).view(np.float32)
    nan_x86 = np.array([0xFFC00000], np.uint32).view(np.float32)
    assert not es.nan_aware_diff(nan_gpu, nan_x86).any()
    assert es.nan_aware_diff(np.array([np.nan], np.float32), np.array([np.inf], np.float32)).all()
