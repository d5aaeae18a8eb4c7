"""Small levels that put chosen cells on either side of the thresholds of the step kernels, and a NaN-aware exact comparison.

Shared by tests/test_edge_states_host.py (the oracle alone: does every entry reach its branch, and does the oracle do what the
reference's expressions say) and tests/test_gpu_edge_states.py (HIP against the oracle on the same entries).

Every builder returns an `Entry`: host levels, solver params, the number of coarse steps, the inlet velocity, and the cells it
targets (0-based (x, y, z, block) of level 1 unless stated). Levels are at most 8 x 4 x 4 blocks.

Kernel lines cited below are in open_ludwig_amd/csrc/kernels.hpp; reference lines in the reference's src/ (restated line by line in
oracle/ludwig_oracle.c).
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from open_ludwig_amd import cases
from open_ludwig_amd.blocks import build_lattice_arrays
from oracle import oracle

CX, CY, CZ, W, OPP, _MY, _MZ = build_lattice_arrays()
F32 = np.float32
REST = 13                                       # the population with c = (0, 0, 0)
TINY_SUBNORMAL = np.array(1, np.uint32).view(np.float32).item()    # 1.4e-45
BELOW_10 = float(np.nextafter(F32(10.0), F32(0.0)))


# ---- comparison ----------------------------------------------------------------------------------------------------------------
def nan_aware_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Boolean mask of the elements where a and b differ. Non-NaN elements must be equal bit for bit (so -0 != +0, and subnormals
    count); NaN must meet NaN. The NaN payload and sign are NOT compared: x86 produces the default NaN 0xFFC00000 (sign set)
    where the GPU produces 0x7FC00000, and neither the reference nor the project gives them a meaning. Float64 arrays (the
    statistics sums) are compared as float64, everything else as float32."""
    wide = np.asarray(a).dtype == np.float64 and np.asarray(b).dtype == np.float64
    ft, it = (np.float64, np.uint64) if wide else (np.float32, np.uint32)
    a = np.asarray(a, dtype=ft)
    b = np.asarray(b, dtype=ft)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    bits_differ = a.view(it) != b.view(it)
    return (na != nb) | (~na & ~nb & bits_differ)


def assert_nan_aware_equal(a, b, what: str, mask: Optional[np.ndarray] = None) -> None:
    d = nan_aware_diff(a, b)
    if mask is not None:
        d &= mask if mask.ndim == d.ndim else mask[..., None]      # a cell mask applies to every component
    if d.any():
        i = tuple(np.argwhere(d)[0])
        raise AssertionError(f"{what}: {int(d.sum())} elements differ, first at {i}: got {np.asarray(a)[i]!r}, "
                             f"want {np.asarray(b)[i]!r}")


def is_subnormal(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a, dtype=np.float32)
    return (a != 0) & (np.abs(a) < np.finfo(np.float32).tiny)


# ---- entries -------------------------------------------------------------------------------------------------------------------
@dataclass
class Entry:
    name: str
    grids: list
    params: object
    steps: int
    u: float
    cells: Dict[str, Tuple[int, int, int, int]] = field(default_factory=dict)
    note: str = ""


def _both(level, name: str, idx, value) -> None:
    """Write into the A and the B buffer (the first step reads f_temp / vel_temp, later ones alternate)."""
    getattr(level, name)[idx] = value
    getattr(level, name + "_temp")[idx] = value


def put_pulled(level, cell, values) -> None:
    """Make the 27 populations cell (x, y, z, b) pulls on its next step equal `values`: population k is read from x - c_k, so
    that is where it is written. Cells must lie in 1..6 of their block, so every source is in the same block."""
    x, y, z, b = cell
    assert all(1 <= c <= 6 for c in (x, y, z))
    for k in range(27):
        _both(level, "f", (x - CX[k], y - CY[k], z - CZ[k], b, k), F32(values[k]))


def _rest_box(nb=(2, 2, 2), tau=0.5006):
    grids, params = cases.periodic_box(nb, tau=tau)
    g = grids[0]
    cases.set_state(g, F32(1.0), F32(0.0), F32(0.0), F32(0.0))
    return grids, params


def _perturbed_box(nb=(2, 2, 2), tau=0.5006, seed=11):
    grids, params = cases.periodic_box(nb, tau=tau)
    cases.init_perturbed(grids[0], seed)
    return grids, params


def density_clamp() -> Entry:
    """Kernel :357 `rho = jl_max(rho, 0.01f)` (finish_rho_only :497), reference physics_kernels.jl:172. Pulled sums below 0.01 at
    rest, exactly 0.01f (all mass in the rest population), negative, and 0.01f + 1 ulp (the side that is not clamped)."""
    grids, params = _perturbed_box()
    g = grids[0]
    w = np.asarray(W, dtype=np.float32)
    cells = {"below": (2, 2, 2, 0), "exact": (4, 4, 4, 1), "negative": (3, 5, 2, 2), "above": (5, 3, 4, 3)}
    below = np.zeros(27, np.float32); below[REST] = F32(0.005)
    put_pulled(g, cells["below"], below)
    exact = np.zeros(27, np.float32); exact[REST] = F32(0.01)
    put_pulled(g, cells["exact"], exact)
    neg = w * F32(0.5); neg[REST] = F32(-1.0)
    put_pulled(g, cells["negative"], neg)
    above = np.zeros(27, np.float32); above[REST] = np.nextafter(F32(0.01), F32(1.0))
    put_pulled(g, cells["above"], above)
    return Entry("density_clamp", grids, params, 3, 0.0, cells)


def subnormal_state() -> Entry:
    """A whole Taylor-Green box scaled by 1e-41: every population is subnormal, every cell clamps to rho = 0.01f (kernel :357) and
    the velocities j / 0.01 come out subnormal. A flush-to-zero build loses them. One step: the collided populations are those of
    rho = 0.01, normal numbers, so a second step would compare no subnormal output."""
    grids, params = cases.periodic_box((2, 2, 2), tau=0.5006)
    g = grids[0]
    for name in ("f", "f_temp"):
        getattr(g, name)[...] *= F32(1e-41)
    for name in ("vel", "vel_temp"):
        getattr(g, name)[...] *= F32(1e-41)
    return Entry("subnormal_state", grids, params, 1, 0.0)


def nonfinite_population(kind: str, k: int = 4) -> Entry:
    """One population of one cell NaN / +Inf / -Inf (a diverged value). Cell x + c_k pulls it on the next step. Reference
    physics_kernels.jl:144-148 sums f_k * c_k for every k, the kernel (:310-320) only the terms with c != 0. NaN runs 2 steps (the
    NaN spreads through the A/B swap, bit-exact); +-Inf runs 1 step, since the difference kept at the pulling cell (DESIGN.md section
    4) spreads to its neighbours on the next one."""
    grids, params = _perturbed_box(seed=13)
    g = grids[0]
    x, y, z, b = 3, 4, 2, 5
    v = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
    _both(g, "f", (x, y, z, b, k), F32(v))
    return Entry(f"nonfinite_{kind}_k{k}", grids, params, 2 if kind == "nan" else 1, 0.0,
                 {"source": (x, y, z, b), "puller": (x + CX[k], y + CY[k], z + CZ[k], b)})


def nan_velocity_only() -> Entry:
    """NaN only in the previous-step velocity (vel_in) of one cell: WALE's OP1 > 1e-12 (kernel :430, reference :283) is false for
    NaN, nu_eddy falls back to nu_bg and every output stays finite."""
    grids, params = _perturbed_box(seed=17)
    g = grids[0]
    c = (4, 4, 4, 3)
    g.vel_temp[c + (0,)] = np.nan
    g.vel[c + (0,)] = np.nan
    return Entry("nan_velocity_only", grids, params, 2, 0.0, {"cell": c})


def overflowed_rho(tau: float = 1.2) -> Entry:
    """Populations 10 and 16 (c = (0, -1, 0), (0, 1, 0)) of one cell 3e38: the density sum overflows to +Inf with zero momentum. The
    reference's Pi sums then hold f_neq * 0 = -Inf * 0 = NaN (physics_kernels.jl:308-322), the kernel's drop those terms. One step:
    the difference kept at this cell spreads to its neighbours on the next one."""
    grids, params = _rest_box(tau=tau)
    g = grids[0]
    c = (3, 3, 3, 2)
    vals = np.asarray(W, dtype=np.float32).copy()
    vals[10] = vals[16] = F32(3e38)
    put_pulled(g, c, vals)
    return Entry(f"overflowed_rho_tau{tau}", grids, params, 1, 0.0, {"cell": c})


def wale_branches() -> Entry:
    """WALE (kernel :429-436, reference :283-297). A uniform velocity gives OP1 = 0 (<= 1e-12). A few cells whose six neighbours
    carry gradients of about 3e-3 give OP1 > 1e-12 with denom <= 1e-12, so nu_eddy stays 0 there too; a cell with gradients of about
    3e-2 takes the eddy viscosity (census: the first two equal a run with c_wale = 0, the third differs)."""
    grids, params = _perturbed_box(seed=23)          # off equilibrium, so that nu_eddy shows in the output
    g = grids[0]
    for name in ("vel", "vel_temp"):
        getattr(g, name)[...] = F32(0.0)
    cells = {"small_gradient": (3, 3, 3, 0), "uniform": (3, 3, 3, 4), "large_gradient": (3, 3, 3, 6)}
    rng = np.random.default_rng(5)
    for name, amp in (("small_gradient", 3e-3), ("large_gradient", 3e-2)):
        x, y, z, b = cells[name]
        for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            for c in range(3):
                _both(g, "vel", (x + dx, y + dy, z + dz, b, c), F32(amp * rng.uniform(-1, 1)))
    return Entry("wale_branches", grids, params, 2, 0.0, cells)


OMEGA_FLOOR = 0.500001


def omega_clamp(tau: float) -> Entry:
    """tau 0.5 and 0.4999 with c_wale = nu_sgs_bg = 0: tau_turb = tau < 0.500001, so omega = 1 / 0.500001 (kernel :438, reference
    :300). The state is off equilibrium (cases.init_perturbed), so omega shows in every population's last bits: the census finds
    the output equal to a run at tau = 0.500001 and different from one at the next float above it."""
    grids, params = _perturbed_box(tau=tau, seed=19)
    params = dataclasses.replace(params, c_wale=0.0, nu_sgs_bg=0.0)
    return Entry(f"omega_clamp_tau{tau}", grids, params, 3, 0.0)


def _wall_tunnel(tau=0.5003, sponge_blend=True):
    return cases.tunnel_with_sphere((6, 4, 4), levels=1, wall_model=True, tau=tau, sponge_blend=sponge_blend)


def wall_distance_edges() -> Entry:
    """wall_dist 0, negative, NaN, 10 and the float just below 10 (kernel :152 `dist_wall > 0 && dist_wall < 10`, reference :205),
    each put next to an ordinary near-wall cell of the same block so that the block's flag (scan_flags, same test) is set."""
    grids, params = _wall_tunnel()
    g = grids[0]
    wd = g.wall_dist
    near = np.argwhere((wd > 0) & (wd < 10) & ~g.obstacle)
    blocks = np.unique(near[:, 3])
    values = {"zero": 0.0, "negative": -1.0, "nan": np.nan, "ten": 10.0, "below_ten": BELOW_10}
    assert len(blocks) >= len(values)
    cells = {}
    for (name, v), b in zip(values.items(), blocks):
        far = np.argwhere(~g.obstacle[..., b] & ~((wd[..., b] > 0) & (wd[..., b] < 10)))
        x, y, z = (int(c) for c in far[0])
        wd[x, y, z, b] = F32(v)
        cells[name] = (x, y, z, int(b))
    return Entry("wall_distance_edges", grids, params, 2, 0.05, cells)


def _near_wall_interior_cells(g, n):
    """n fluid cells with 0 < wall_dist < 10, no sponge, at 1..6 inside their block (put_pulled can write all their sources), in
    distinct blocks"""
    wd = g.wall_dist
    ok = (wd > 0) & (wd < 10) & ~g.obstacle & (g.sponge == 0)
    ok[[0, 7], :, :, :] = False
    ok[:, [0, 7], :, :] = False
    ok[:, :, [0, 7], :] = False
    out, used = [], set()
    for x, y, z, b in np.argwhere(ok):
        if b in used:
            continue
        out.append((int(x), int(y), int(z), int(b)))
        used.add(b)
        if len(out) == n:
            return out
    raise AssertionError("not enough near-wall interior cells")


def _moving_cell(level, cell, ux) -> None:
    """pulled set of rho = 1 exactly and u = (ux, 0, 0) exactly: the rest population 1 - ux and population 14 (c = (1, 0, 0)) ux"""
    v = np.zeros(27, np.float32)
    v[14] = F32(ux)
    v[REST] = F32(1.0) - F32(ux)
    assert F32(v[REST] + v[14]) == F32(1.0)
    put_pulled(level, cell, v)


UMAG_TAU = float(np.nextafter(F32(0.5), F32(1.0)))    # nu_visc = 2e-8: with wall_dist 0.1, tau_wall > tau_res just above 1e-6


def wall_umag_edges() -> Entry:
    """u_mag exactly 1e-6 and the float just above (kernel :154 `u_mag > 1e-6f`, reference :209), with tau = 0.5 + 1 ulp and wall_dist
    0.1, where tau_wall > tau_res for the cell just above. Its force cannot reach an output bit: at |u| = 1e-6 the force per unit
    density is below 3e-9 of the populations for any tau and any wall_dist < 10 (u_tau >= 1e-6 is needed against tau_res = nu u / d,
    and the force is (u_tau^2 - nu u / d) / d). So the census shows the threshold through the inputs read back from the output
    (u_mag = 1e-6 exactly, and one ulp more), and the GPU comparison pins the branch as far as any output can."""
    grids, params = _wall_tunnel(tau=UMAG_TAU)
    g = grids[0]
    at, above = _near_wall_interior_cells(g, 2)
    for c, ux in ((at, F32(1e-6)), (above, np.nextafter(F32(1e-6), F32(1.0)))):
        g.wall_dist[c] = F32(0.1)
        _moving_cell(g, c, ux)
    return Entry("wall_umag_edges", grids, params, 2, 0.05, {"at_1e-6": at, "above_1e-6": above})


def wall_y_plus(dist, u_mag, tau):
    """y_p of kernel wall_model_force_mag :155-158 (reference :210-215) in float32, operation by operation"""
    from oracle import oracle as _o
    import ctypes as C
    lib = _o.lib()
    lib.oracle_jl_powf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]

    def pw(x, y):
        xa, ya, out = np.array([x], np.float32), np.array([y], np.float32), np.zeros(1, np.float32)
        lib.oracle_jl_powf(xa.ctypes.data, ya.ctypes.data, out.ctypes.data, 1)
        return out[0]
    d, u = F32(dist), F32(u_mag)
    nu = (F32(tau) - F32(0.5)) / F32(3.0)
    u_tau = u * pw(nu / (d * u + F32(1e-10)), F32(1.0) / F32(7.0)) * pw(F32(2.0) * F32(8.3), -F32(1.0) / F32(7.0))
    u_tau = max(u_tau, F32(1e-6))
    return F32(u_tau * d / nu)


YP_LIMIT = F32(11.81)


def _yp_straddle(u_mag, tau):
    """adjacent float32 wall distances d_lo < d_hi with y_p(d_lo) <= 11.81 < y_p(d_hi) (bisection over the float bits)"""
    lo, hi = np.array([0.001], np.float32).view(np.uint32)[0], np.array([5.0], np.float32).view(np.uint32)[0]
    as_f = lambda i: np.array([i], np.uint32).view(np.float32)[0]
    assert wall_y_plus(as_f(lo), u_mag, tau) <= YP_LIMIT < wall_y_plus(as_f(hi), u_mag, tau)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if wall_y_plus(as_f(mid), u_mag, tau) <= YP_LIMIT:
            lo = mid
        else:
            hi = mid
    return float(as_f(lo)), float(as_f(hi))


def wall_y_plus_edges() -> Entry:
    """y_p on both sides of 11.81 (kernel :159, reference :216): two cells with u = (0.05, 0, 0) exactly and the two adjacent
    wall distances at which y_p crosses the limit. Above it the log law replaces u_tau, and at this u and distance that lowers
    tau_wall below tau_res: the cell above the limit gets no force, the one below does (census against a run without the wall
    model).
    `u_plus_law <= 0.1` (kernel :161) is not reached: once y_p > 11.81 the log law is at least log(11.81) / 0.41 + 5.2 = 11.2,
    so no entry chases it."""
    tau, u = 0.5003, 0.05
    grids, params = _wall_tunnel(tau=tau)
    g = grids[0]
    d_lo, d_hi = _yp_straddle(u, tau)
    below, above = _near_wall_interior_cells(g, 2)
    for c, d in ((below, d_lo), (above, d_hi)):
        g.wall_dist[c] = F32(d)
        _moving_cell(g, c, u)
    return Entry("wall_y_plus_edges", grids, params, 2, 0.05, {"y_p_below": below, "y_p_above": above},
                 note=f"{d_lo!r} {d_hi!r}")


def wall_model_tau_half() -> Entry:
    """tau 0.5: nu_visc = 0, so `nu_visc > 1e-10` (kernel :154, reference :209) is false for every near-wall cell: no wall force."""
    grids, params = _wall_tunnel(tau=0.5)
    return Entry("wall_model_tau_half", grids, params, 2, 0.05)


def sponge_edges(blend: bool) -> Entry:
    """sp = 0, the smallest subnormal and 1 (kernel :362-379, reference :181-199) with distribution blending on or off. sp = 1
    replaces rho by 1 and u by (u_inlet, 0, 0) exactly."""
    grids, params = cases.tunnel_with_sphere((6, 4, 4), levels=1, wall_model=False, sponge_blend=blend)
    g = grids[0]
    cells = {"zero": (2, 3, 4, 30), "tiny": (3, 3, 4, 30), "one": (4, 3, 4, 30), "one_b": (5, 5, 5, 31)}
    g.sponge[2, 3, 4, 30] = F32(0.0)
    g.sponge[3, 3, 4, 30] = F32(TINY_SUBNORMAL)
    g.sponge[4, 3, 4, 30] = F32(1.0)
    g.sponge[5, 5, 5, 31] = F32(1.0)
    assert not g.obstacle[2:6, 3:6, 4:6, 30:32].any()
    return Entry(f"sponge_edges_blend{int(blend)}", grids, params, 2, 0.05, cells)


Q_EDGE_HALVES = {
    "below_qmin": None, "at_or_above_qmin": None,          # filled in below: the halves on either side of 0.001
    "below_half": 0x37FF, "half": 0x3800, "above_half": 0x3801,
    "one": 0x3C00, "above_one": 0x3C01, "tiny_subnormal": 0x0001, "+inf": 0x7C00, "nan": 0x7E00,
}


def _qmin_neighbours():
    h = np.float16(0.001)
    lo = h if np.float32(h) <= F32(0.001) else np.nextafter(h, np.float16(0))
    hi = np.nextafter(lo, np.float16(1))
    return int(np.array(lo).view(np.uint16)), int(np.array(hi).view(np.uint16))


Q_EDGE_HALVES["below_qmin"], Q_EDGE_HALVES["at_or_above_qmin"] = _qmin_neighbours()


def bouzidi_edges(q_min: float) -> Entry:
    """The q-map encodings at the edges of `q > q_min && q <= 1` and `q < 0.5` (kernel k_bouzidi :910-921 / :936-956, reference
    bouzidi_kernel.jl:44-77), written on links of listed cells; q_min >= 0 takes the compact link list, q_min < 0 the full map.
    One more listed cell in a corner of the level has a q < 0.5 link whose cell one step behind lies off the level."""
    grids, params = cases.tunnel_with_sphere((6, 4, 4), levels=1, wall_model=False)
    params = dataclasses.replace(params, q_min_threshold=q_min)
    g = grids[0]
    qm = g.bouzidi_q_map.view(np.uint16)
    cx_, cy_, cz_, cb = (np.asarray(a, np.int64) - 1 for a in (g.bouzidi_cell_x, g.bouzidi_cell_y, g.bouzidi_cell_z, g.bouzidi_cell_block))
    fluid = np.flatnonzero(~g.obstacle[cx_, cy_, cz_, cb])
    cells = {}
    for i, (name, bits) in enumerate(Q_EDGE_HALVES.items()):
        c = fluid[7 * i]
        k = 1 + (i % 12)                                   # a link with c != 0
        qm[cx_[c], cy_[c], cz_[c], cb[c], k] = bits
        cells[name] = (int(cx_[c]), int(cy_[c]), int(cz_[c]), int(cb[c]), k)
    # an extra listed cell at the level's corner cell (0, 0, 0) of block (1, 1, 1), with q = 0.2 on link k = 26: the cell one step
    # behind, x + c_opp(k) = x - (1, 1, 1), lies off the level, so f_ff falls back to f_k (reference bouzidi_kernel.jl:48-66)
    b0 = int(g.block_pointer[0, 0, 0]) - 1
    k = 26
    qm[0, 0, 0, b0, k] = 0x3266                            # 0.2
    g.bouzidi_cell_x = np.append(g.bouzidi_cell_x, np.int8(1))
    g.bouzidi_cell_y = np.append(g.bouzidi_cell_y, np.int8(1))
    g.bouzidi_cell_z = np.append(g.bouzidi_cell_z, np.int8(1))
    g.bouzidi_cell_block = np.append(g.bouzidi_cell_block, np.int32(b0 + 1))
    g.n_boundary_cells += 1
    cells["behind_off_level"] = (0, 0, 0, b0, k)
    return Entry(f"bouzidi_edges_qmin{q_min}", grids, params, 2, 0.05, cells)


def interface_edges(kind: str, temporal: bool) -> Entry:
    """Coarse -> fine interface (kernel k_interface_links :859-867, reference physics_interpolation.jl:127-135): parent tau 0.5
    (tau_c <= 1e-6: scale 1), tau ratios below 0.01 and above 100 (the clamp), or NaN in the parent's state next to the child."""
    taus = {"parent_half": (0.5, 0.5003), "ratio_low": (0.6, 0.500001), "ratio_high": (0.5001, 0.6), "nan_parent": (0.5006, 0.5003)}
    tp, tc = taus[kind]
    grids, params = cases.tunnel_with_sphere((6, 4, 4), levels=2, wall_model=False, temporal=temporal, tau=tp)
    grids[1].tau = F32(tc)
    cells = {}
    if kind == "nan_parent":
        p, ch = grids[0], grids[1]
        # a parent cell just outside the refined blocks: its neighbours feed the child's interpolation stencils
        bx = int(ch.map_x.min() + 1) // 2 - 1           # parent block x of the first child column, 1-based -> one to the left
        by, bz = int(ch.map_y.min() + 1) // 2, int(ch.map_z.min() + 1) // 2
        pb = int(p.block_pointer[bx - 1, by - 1, bz - 1]) - 1
        assert pb >= 0
        c = (7, 3, 3, pb)
        assert not p.obstacle[c]
        _both(p, "f", c + (14,), np.nan)                 # population 14: c = (+1, 0, 0), pulled into the refined region's side
        cells["parent_cell"] = c
    return Entry(f"interface_{kind}_temporal{int(temporal)}", grids, params, 2, 0.05, cells)


def catalogue() -> List[Entry]:
    return [density_clamp(), subnormal_state(), *(nonfinite_population(kd) for kd in ("nan", "+inf", "-inf")),
            nonfinite_population("nan", k=REST), nan_velocity_only(), overflowed_rho(1.2), overflowed_rho(0.8), wale_branches(),
            omega_clamp(0.5), omega_clamp(0.4999), wall_distance_edges(), wall_umag_edges(), wall_y_plus_edges(), wall_model_tau_half(), sponge_edges(True),
            sponge_edges(False), bouzidi_edges(0.001), bouzidi_edges(-1.0), *(interface_edges(kd, t) for kd in
            ("parent_half", "ratio_low", "ratio_high", "nan_parent") for t in (True, False))]


def run_oracle(e: Entry) -> None:
    oracle.execute_timestep_batch(e.grids, 1, e.steps, F32(e.u), e.params)


def output_names(i: int, g, steps: int) -> List[str]:
    fn, vn = oracle.newest_buffers(i, steps)
    names = [fn, vn, "rho"]
    if g.n_boundary_cells > 0:
        names.append("f_post_collision")
    return names


# ---- divergence the kernel keeps ("Non-finite states") --------------------------------------------------------
def nonfinite_pull_cells(g, f_in: np.ndarray) -> np.ndarray:
    """bool [8,8,8,nb]: the cells of a periodic single level whose pulled set holds a +-Inf, or whose pulled density sum is not
    finite while every pulled value is. Where the reference multiplies such a value (or the Inf it leads to) by a lattice constant 0,
    the kernel drops the product: its outputs at these cells may differ from the reference's, which are NaN there."""
    nb = g.n_blocks
    nt = np.asarray(g.neighbor_table)
    total = np.zeros((8, 8, 8, nb), dtype=np.float64)
    has_inf = np.zeros((8, 8, 8, nb), dtype=bool)
    idx = np.indices((8, 8, 8)).reshape(3, -1).T
    for k in range(27):
        pulled = np.empty((8, 8, 8, nb), dtype=np.float32)
        for b in range(nb):
            for x, y, z in idx:
                sx, sy, sz = x - CX[k], y - CY[k], z - CZ[k]
                o = [(-1 if s < 0 else (1 if s > 7 else 0)) for s in (sx, sy, sz)]
                sb = b if o == [0, 0, 0] else nt[b, (o[0] + 1) + 3 * (o[1] + 1) + 9 * (o[2] + 1)] - 1
                pulled[x, y, z, b] = f_in[sx % 8, sy % 8, sz % 8, sb, k]
        has_inf |= np.isinf(pulled)
        total += pulled.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = has_inf | (~np.isfinite(total.astype(np.float32)) & ~np.isnan(total))
    return out
