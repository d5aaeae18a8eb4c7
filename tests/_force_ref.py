"""A plain numpy restatement of the surface-force path, written from the reference's Julia alone (test infrastructure).

Independent of open_ludwig_amd.forces / surface_stats / force_series and of the HIP kernels (none of them is imported): the search is
stated as a set (which cells are candidates, which one wins), not as the shell loop; the stress works on [n, 3] vectors with masked
assignment instead of a guarded division; the working float type is a parameter - float32, in the reference's written operand order,
defines the expected bits; float64 gives reference values. It never writes to its inputs.

What it restates (file:line of the reference):
  src/forces/surface.jl:32-89     compute_stress_from_cell: gauge pressure, tangential velocity, the two gates, the shear vector
  src/forces/surface.jl:95-124    get_cell_at_position: which global cell index is a readable cell
  src/forces/surface.jl:138-266   map_stresses_kernel!: base cell, expanding shells, strict `<`, the break after a shell > 1, the
                                  max(wall_dist, 0.5f0) clamp, zeros without a cell
  src/forces/surface.jl:282-366   integrate_forces_kernel!: the nine per-triangle contributions
  src/forces/surface.jl:467-571   integrate_surface_forces!: symmetry table, totals, F_ref / M_ref guards, coefficients
  src/forces/surface.jl:430       the coverage count: a Float32 pressure against the Float64 literal 1e-10

The inputs of the operation are Float32 arrays (triangle centres, normals, areas, the mesh offset, dx, tau, pressure_scale, rho,
vel): the float64 variant widens those values and rounds nothing afterwards. Literals keep their Float32 VALUES (0.5f0, 0.01f0,
1.0f-10, 3.0f0, Float32(1e10)): they belong to the operation's definition, not to its rounding.

The search, declaratively (equivalent to lines 191-240: shell 0 and 1 are always scanned, a later shell only while nothing was found;
inside a shell the scan order is dz, dy, dx and only a strictly smaller distance replaces the best):
  r1        = the smallest Chebyshev radius <= search_radius around the base cell floor(t / dx) + 1 holding a valid fluid cell
  candidates = the valid fluid cells within Chebyshev radius min(search_radius, max(1, r1))
  winner    = the candidate of the smallest squared distance; ties go to the smallest (shell radius, dz, dy, dx)
  no r1     -> no cell.

The nine sums are plain float64 sums of the per-triangle contributions: the reference adds with contended Float32 atomics in an
unspecified order, so no float32 order is "the" answer.

Tolerances (measured; see tests/test_force_reference_host.py and DESIGN.md section 5)
-----------------------------------------------------------------------------------
e_ref = |ref32 - ref64| / scale over every non-planted triangle of tests/_force_cases.py, with scale =
pressure_scale * max(|rho - 1| / 3, 2^-24) for p and rho * nu * |u| / wd * stress_scale for each shear component (|u|, not |u_t|: the
cancellation in u - (u.n) n is judged against what went in). MAX_E_REF is its maximum with under 10 % on top; the asserted bound for
anything against ref64 is MARGIN * MAX_E_REF.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

B = 8                                            # src/blocks.jl:14
F32 = np.float32
HALF, GATE_WD, GATE_U, THREE, ONE = F32(0.5), F32(0.01), F32(1.0e-10), F32(3.0), F32(1.0)
FAR = F32(1e10)                                  # Float32(1e10), line 182
COVERAGE_THRESHOLD = 1e-10                       # Float64, line 430

# ---- measured tolerances (CPU host run of tests/test_force_reference_host.py, printed by its census test) ----
# measured max e_ref over the table and the sphere: p 7.943e-08, tau 1.851e-07; recorded with < 10 % on top (elementwise IEEE
# operations only: no summation whose grouping could differ between CPUs)
MAX_E_REF = {"p": 8.6e-8, "tau": 2.0e-7}
# tests/_step_ref.py keeps 4 for 27-term sums in another association; the expressions here have at most three terms per sum and the
# code under test uses the SAME operand order as ref32, so its distance to ref64 is e_ref itself - 4 is kept as the one margin of
# this suite, not because this expression needs it
MARGIN = 4.0


def bound(kind: str) -> float:
    return MARGIN * MAX_E_REF[kind]


def _inputs(centers, offset, dx, ft):
    """t = Float32(c) + Float32(off) in the working type (lines 161-163) and dx"""
    c = np.asarray(centers, dtype=F32).astype(ft)
    off = np.asarray(offset, dtype=F32).astype(ft)
    return c + off[None, :], ft(F32(dx))


def _shell_offsets(radius: int):
    """every (ddx, dy, dz) of the cube of Chebyshev radius `radius`, its shell, and its rank in (shell, dz, dy, dx) order"""
    r = np.arange(-radius, radius + 1)
    dz, dy, ddx = np.meshgrid(r, r, r, indexing="ij")
    off = np.stack([ddx.ravel(), dy.ravel(), dz.ravel()], axis=1).astype(np.int64)
    shell = np.abs(off).max(axis=1)
    order = np.lexsort((off[:, 0], off[:, 1], off[:, 2], shell))           # last key is the primary one
    rank = np.empty(len(off), dtype=np.int64)
    rank[order] = np.arange(len(off))
    return off, shell, rank


def valid_fluid(g, obstacle, block_pointer):
    """get_cell_at_position (lines 95-124) and `!obstacle` (line 218) for global 1-based cells g [..., 3]:
    -> (valid bool [...], block 0-based [...], local 0-based [..., 3]); block and local are 0 where invalid"""
    bp = np.asarray(block_pointer)
    dims = np.array(bp.shape, dtype=np.int64)
    positive = (g >= 1).all(axis=-1)
    gb = np.where(positive[..., None], g - 1, 0)
    blk3 = gb // B
    inside = positive & (blk3 < dims).all(axis=-1)
    blk3 = np.where(inside[..., None], blk3, 0)
    b_idx = np.where(inside, bp[blk3[..., 0], blk3[..., 1], blk3[..., 2]], 0).astype(np.int64)
    present = b_idx > 0
    loc = np.where(present[..., None], gb % B, 0)
    b0 = np.where(present, b_idx - 1, 0)
    fluid = present & ~np.asarray(obstacle)[loc[..., 0], loc[..., 1], loc[..., 2], b0]
    return fluid, np.where(fluid, b0, 0), np.where(fluid[..., None], loc, 0)


def search(centers, offset, dx, obstacle, block_pointer, search_radius: int, ft=np.float64, chunk: int = 32):
    """lines 161-240 for all triangles: -> found bool [n], block [n], local [n, 3] (0-based; 0 where not found), wall_dist [n] in the
    working type (sqrt(d2) / dx of the winner, 0.5 where not found), base [n, 3] (1-based base cell)"""
    t, dxw = _inputs(centers, offset, dx, ft)
    n = t.shape[0]
    base = np.floor(t / dxw).astype(np.int64) + 1
    off, shell, rank = _shell_offsets(int(search_radius))
    found = np.zeros(n, dtype=bool)
    block = np.zeros(n, dtype=np.int64)
    local = np.zeros((n, 3), dtype=np.int64)
    wd = np.full(n, ft(HALF), dtype=ft)
    big = np.iinfo(np.int64).max
    for lo in range(0, n, chunk):
        sl = slice(lo, min(n, lo + chunk))
        g = base[sl, None, :] + off[None, :, :]                                    # [m, k, 3]
        ok, blk, loc = valid_fluid(g, obstacle, block_pointer)
        r1 = np.where(ok, shell[None, :], big).min(axis=1)                         # [m]
        has = r1 <= search_radius
        reach = np.minimum(search_radius, np.maximum(1, np.where(has, r1, 0)))
        cand = ok & (shell[None, :] <= reach[:, None]) & has[:, None]
        cc = (g.astype(ft) - ft(HALF)) * dxw                                       # lines 220-222
        e = t[sl, None, :] - cc
        d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]        # line 224, left to right
        d2 = np.where(cand & (d2 < ft(FAR)), d2, np.inf)                           # line 226 against the initial Float32(1e10)
        dmin = d2.min(axis=1)
        tie = np.isfinite(dmin)[:, None] & (d2 == dmin[:, None])
        win = np.where(tie, rank[None, :], big).argmin(axis=1)
        got = np.isfinite(dmin)
        rows = np.arange(win.size)
        found[sl] = got
        block[sl] = np.where(got, blk[rows, win], 0)
        local[sl] = np.where(got[:, None], loc[rows, win], 0)
        with np.errstate(invalid="ignore"):
            wd[sl] = np.where(got, np.sqrt(np.where(got, dmin, 0)).astype(ft) / dxw, ft(HALF))      # line 233
    return SimpleNamespace(found=found, block=block, local=local, wall_dist=wd, base=base)


def gather(cells, rho, vel, ft=np.float64):
    """best_rho [n], best_u [n, 3] of the winners (lines 183-186 where none: 1 and 0)"""
    n = cells.found.size
    r = np.ones(n, dtype=ft)
    u = np.zeros((n, 3), dtype=ft)
    j = np.flatnonzero(cells.found)
    x, y, z, b = cells.local[j, 0], cells.local[j, 1], cells.local[j, 2], cells.block[j]
    r[j] = np.asarray(rho)[x, y, z, b].astype(ft)
    u[j] = np.asarray(vel)[x, y, z, b, :].astype(ft)
    return r, u


def stress(rho, u, normals, wall_dist, found, tau, pressure_scale, ft=np.float64, stress_scale=None):
    """lines 243-258 and compute_stress_from_cell (32-89): -> (p, tau_vec [n, 3], gates) in the working type; gates records
    (shear gate open, clamp active) per triangle"""
    rho = np.asarray(rho).astype(ft)
    u = np.asarray(u).astype(ft)
    nrm = np.asarray(normals, dtype=F32).astype(ft)
    ps = ft(F32(pressure_scale))
    ss = ps if stress_scale is None else ft(F32(stress_scale))
    tau_m = ft(F32(tau))
    with np.errstate(all="ignore"):
        wd_raw = np.asarray(wall_dist).astype(ft)
        wd = np.where(wd_raw < ft(HALF), ft(HALF), wd_raw)                         # max(best_wall_dist, 0.5f0), line 250
        p = ((rho - ft(ONE)) / ft(THREE)) * ps                                     # lines 48-49
        u_dot_n = (u[:, 0] * nrm[:, 0] + u[:, 1] * nrm[:, 1]) + u[:, 2] * nrm[:, 2]           # line 58
        ut = u - u_dot_n[:, None] * nrm                                            # lines 59-61
        mag = np.sqrt((ut[:, 0] * ut[:, 0] + ut[:, 1] * ut[:, 1]) + ut[:, 2] * ut[:, 2])      # line 64
        nu = (tau_m - ft(HALF)) / ft(THREE)                                        # line 67
        gate = (mag > ft(GATE_U)) & (wd > ft(GATE_WD))                             # line 74
        shear = np.zeros_like(u)
        j = np.flatnonzero(gate)
        lat = rho[j] * nu * mag[j] / wd[j]                                         # line 77
        phys = lat * ss                                                            # line 80
        shear[j] = (ut[j] / mag[j][:, None]) * phys[:, None]                       # lines 83-85
    found = np.asarray(found, dtype=bool)
    p = np.where(found, p, ft(0.0)).astype(ft)
    shear = np.where(found[:, None], shear, ft(0.0)).astype(ft)
    gates = np.stack([gate & found, (wd_raw < ft(HALF)) & found], axis=1)
    return p, shear, gates


def scales(rho, u, wall_dist, tau, pressure_scale):
    """the e_ref scales of the module docstring, float64: (for p [n], for every shear component [n])"""
    rho = np.asarray(rho, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    ps = float(F32(pressure_scale))
    nu = (float(F32(tau)) - 0.5) / 3.0
    wd = np.maximum(np.asarray(wall_dist, dtype=np.float64), 0.5)
    with np.errstate(all="ignore"):
        return ps * np.maximum(np.abs(rho - 1.0) / 3.0, 2.0 ** -24), np.abs(rho) * nu * np.linalg.norm(u, axis=1) / wd * ps


def map_stresses(centers, normals, offset, dx, tau, pressure_scale, rho, vel, obstacle, block_pointer, search_radius=5, ft=np.float64):
    """map_stresses_kernel! whole: -> namespace(cells, rho, u, p, tau [n, 3], gates)"""
    cells = search(centers, offset, dx, obstacle, block_pointer, search_radius, ft)
    r, u = gather(cells, rho, vel, ft)
    p, shear, gates = stress(r, u, normals, cells.wall_dist, cells.found, tau, pressure_scale, ft)
    return SimpleNamespace(cells=cells, rho=r, u=u, p=p, tau=shear, gates=gates)


def coverage(p) -> int:
    """line 430: count(x -> abs(x) > 1e-10) - Julia promotes the Float32 pressure to Float64 for the comparison"""
    return int(np.count_nonzero(np.abs(np.asarray(p).astype(np.float64)) > COVERAGE_THRESHOLD))


def contributions(p, shear, centers, normals, areas, offset, moment_center, ft=np.float64):
    """integrate_forces_kernel! per triangle (lines 302-349): [n, 9] = dFp(3), dFv(3), dM(3) in the working type"""
    p = np.asarray(p).astype(ft)
    shear = np.asarray(shear).astype(ft)
    nrm = np.asarray(normals, dtype=F32).astype(ft)
    area = np.asarray(areas, dtype=F32).astype(ft)
    c, _ = _inputs(centers, offset, 1.0, ft)                                       # lines 314-316
    ref = np.asarray(moment_center, dtype=F32).astype(ft)
    with np.errstate(all="ignore"):
        d_fp = ((-p)[:, None] * nrm) * area[:, None]                               # lines 323-325: (-p * n) * A
        d_fv = shear * area[:, None]                                               # lines 329-331
        d_f = d_fp + d_fv                                                          # lines 334-336
        r = c - ref[None, :]                                                       # lines 342-344
        d_m = np.stack([r[:, 1] * d_f[:, 2] - r[:, 2] * d_f[:, 1],                 # lines 347-349
                        r[:, 2] * d_f[:, 0] - r[:, 0] * d_f[:, 2],
                        r[:, 0] * d_f[:, 1] - r[:, 1] * d_f[:, 0]], axis=1)
    return np.concatenate([d_fp, d_fv, d_m], axis=1).astype(ft)


def sums(contrib) -> np.ndarray:
    """the nine accumulators as plain float64 sums"""
    return np.asarray(contrib).astype(np.float64).sum(axis=0)


def finish(nine, symmetric: bool, rho_ref: float, u_ref: float, area_ref: float, chord_ref: float) -> dict:
    """lines 507-571, literally: Float64 throughout"""
    fx_p, fy_p, fz_p, fx_v, fy_v, fz_v, mx, my, mz = (float(v) for v in nine)
    if symmetric:                                                                  # lines 518-526
        fx_p *= 2.0; fz_p *= 2.0
        fx_v *= 2.0; fz_v *= 2.0
        my *= 2.0
        fy_p = 0.0; fy_v = 0.0
        mx = 0.0; mz = 0.0
    out = dict(Fx_pressure=fx_p, Fy_pressure=fy_p, Fz_pressure=fz_p, Fx_viscous=fx_v, Fy_viscous=fy_v, Fz_viscous=fz_v,
               Fx=fx_p + fx_v, Fy=fy_p + fy_v, Fz=fz_p + fz_v, Mx=mx, My=my, Mz=mz, Cd=0.0, Cl=0.0, Cs=0.0, Cmx=0.0, Cmy=0.0, Cmz=0.0)
    q_inf = 0.5 * rho_ref * u_ref ** 2                                             # line 548
    f_ref = q_inf * area_ref                                                       # line 551
    m_ref = f_ref * chord_ref                                                      # line 554
    if f_ref > 1e-10:                                                              # lines 556-565
        out["Cd"] = out["Fx"] / f_ref
        out["Cl"] = out["Fz"] / f_ref
        out["Cs"] = out["Fy"] / f_ref
    if m_ref > 1e-10:                                                              # lines 567-571
        out["Cmx"] = out["Mx"] / m_ref
        out["Cmy"] = out["My"] / m_ref
        out["Cmz"] = out["Mz"] / m_ref
    return out
