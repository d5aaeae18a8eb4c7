"""Host restatement of the wall diagnostics (kernels.hpp wall_model_state, k_wall_census, k_wall_surface) in numpy float32, operation
by operation. Pow comes from the oracle's oracle_jl_powf and log from oracle_jl_math(2, ...) cast to float32 - the route
tests/_edge_states.wall_y_plus takes - so the product package needs no host pow / log of its own.

Inputs are a level's fields in the reference layout, as ludwig_level_download returns them: rho [8,8,8,nb], vel [8,8,8,nb,3] (the
buffer the last sub-step wrote), obstacle [8,8,8,nb] bool, wall_dist [8,8,8,nb].
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from open_ludwig_amd import wall_diagnostics as wd
from open_ludwig_amd.surface_stats import scales
from oracle import oracle

F32 = np.float32
KAPPA = F32(0.41)


def _pow(x, y):
    lib = oracle.lib()
    x = np.ascontiguousarray(x, dtype=F32)
    y = np.ascontiguousarray(np.broadcast_to(F32(y), x.shape), dtype=F32)
    out = np.zeros(x.shape, dtype=F32)
    lib.oracle_jl_powf.restype = None
    lib.oracle_jl_powf(C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data), C.c_void_p(out.ctypes.data), C.c_int64(x.size))
    return out


def _log(x):
    lib = oracle.lib()
    xd = np.ascontiguousarray(x, dtype=F32).astype(np.float64)
    out = np.zeros(xd.shape, dtype=np.float64)
    lib.oracle_jl_math.restype = None
    lib.oracle_jl_math(C.c_int(2), C.c_void_p(xd.ctypes.data), C.c_void_p(out.ctypes.data), C.c_int64(xd.size))
    with np.errstate(over="ignore", invalid="ignore"):
        return out.astype(F32)


def _jl_max(a, b):
    """Julia's max: NaN propagates"""
    b = np.broadcast_to(F32(b), a.shape)
    return np.where(a != a, a, np.where(a > b, a, b)).astype(F32)


def wall_state(dist_wall, tau, rho, u_mag, obstacle=None):
    """(u_tau, y_plus, code) of 1-D arrays of cells; code as wall_diagnostics.CODE_* with CODE_FORCED or-ed in"""
    d, rho, u = (np.ascontiguousarray(a, dtype=F32).reshape(-1) for a in (dist_wall, rho, u_mag))
    n = d.size
    u_tau_out, y_plus, code = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, np.int64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        near = (d > F32(0.0)) & (d < F32(10.0))
        if obstacle is not None:
            near &= ~np.asarray(obstacle, dtype=bool).reshape(-1)
        code[near] = wd.CODE_SKIPPED
        nu = (F32(tau) - F32(0.5)) / F32(3.0)
        run = np.flatnonzero(near & (u > F32(1.0e-6)) & bool(nu > F32(1.0e-10)))
        if run.size == 0:
            return u_tau_out, y_plus, code
        d, rho, u = d[run], rho[run], u[run]
        u_tau = u * _pow(nu / (d * u + F32(1.0e-10)), F32(1.0) / F32(7.0)) * _pow(np.full(1, F32(2.0) * F32(8.3), F32), -F32(1.0) / F32(7.0))[0]
        u_tau = _jl_max(u_tau, 1.0e-6)
        y_p = u_tau * d / nu
        c = np.full(run.size, wd.CODE_POWER, np.int64)
        u_plus_law = (F32(1.0) / KAPPA) * _log(y_p) + F32(5.2)
        take = (y_p > F32(11.81)) & (u_plus_law > F32(0.1))
        law = _jl_max(u_tau * ((u / u_tau) / u_plus_law), 1.0e-6)
        u_tau = np.where(take, law, u_tau).astype(F32)
        c[take] = wd.CODE_LOG
        tau_wall = rho * u_tau * u_tau
        tau_res = rho * nu * (u / d)
        c[tau_wall > tau_res] |= wd.CODE_FORCED
        u_tau_out[run], y_plus[run], code[run] = u_tau, u_tau * d / nu, c
    return u_tau_out, y_plus, code


def _cells(a, nb, k=None):
    """[8,8,8,nb(,K)] -> [nb * 512(, K)] in (block, cell) order"""
    a = np.asarray(a)
    if k is None:
        return a.reshape(512, nb, order="F").T.reshape(-1)
    return a.reshape(512, nb, k, order="F").transpose(1, 0, 2).reshape(-1, k)


def _u_mag(u):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]).astype(F32)


def level_state(rho, vel, obstacle, wall_dist, tau, n_owned=None):
    """per cell of blocks [0, n_owned) in (block, cell) order: (u_tau, y_plus, code, rho)"""
    nb = int(rho.shape[3])
    n = (nb if n_owned is None else int(n_owned)) * 512
    r = _cells(np.asarray(rho, F32), nb)[:n]
    u = _cells(np.asarray(vel, F32), nb, 3)[:n]
    return wall_state(_cells(np.asarray(wall_dist, F32), nb)[:n], tau, r, _u_mag(u), _cells(obstacle, nb)[:n]) + (r,)


def census(rho, vel, obstacle, wall_dist, tau, n_owned=None) -> wd.Census:
    """the record ludwig_level_wall_census gives for these fields"""
    u_tau, y_plus, code, r = level_state(rho, vel, obstacle, wall_dist, tau, n_owned)
    base = code & 3
    ran = base >= wd.CODE_POWER
    with np.errstate(over="ignore", invalid="ignore"):
        finite = np.isfinite(y_plus) & np.isfinite((r * u_tau * u_tau).astype(F32))
    ev = ran & finite
    rec = wd.Census(near_cells=int((code > 0).sum()), evaluated=int(ev.sum()), log_law=int((ev & (base == wd.CODE_LOG)).sum()),
                    forced=int((ev & ((code & wd.CODE_FORCED) != 0)).sum()), non_finite=int((ran & ~finite).sum()))
    if rec.evaluated:
        bits = y_plus[ev].view(np.uint32)
        rec.min_bits, rec.max_bits = int(bits.min()), int(bits.max())
        rec.hist = np.bincount(wd.bin_of(y_plus[ev]), minlength=wd.N_BINS).astype(np.uint64)
    return rec


def surface_values(plan, rho, vel, obstacle, wall_dist, tau, params) -> np.ndarray:
    """[7, n_tri] float32: what ludwig_wall_surface_compute gives for the triangles of a surface_stats.SurfacePlan"""
    n = plan.n
    out = np.zeros((len(wd.ROWS), n), dtype=F32)
    ps, ss = scales(params)
    r = np.ones(n, dtype=F32)
    j = np.flatnonzero(plan.found)
    b, c = plan.blocks[j].astype(np.int64), plan.cells[j].astype(np.int64)
    x, y, z = c % 8, (c // 8) % 8, c // 64
    r[j] = rho[x, y, z, b]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        out[0] = ((r - F32(1.0)) / F32(3.0)) * ps
        if j.size:
            u = np.stack([vel[x, y, z, b, k] for k in range(3)], axis=1).astype(F32)
            u_tau, y_plus, code = wall_state(wall_dist[x, y, z, b], tau, r[j], _u_mag(u), obstacle[x, y, z, b])
            nrm = plan.normals[j].astype(F32)
            udn = u[:, 0] * nrm[:, 0] + u[:, 1] * nrm[:, 1] + u[:, 2] * nrm[:, 2]
            ut = [u[:, k] - udn * nrm[:, k] for k in range(3)]
            umag = np.sqrt(ut[0] * ut[0] + ut[1] * ut[1] + ut[2] * ut[2]).astype(F32)
            on = (umag > F32(1.0e-10)) & ((code & 3) >= wd.CODE_POWER)
            tmag = (r[j] * u_tau * u_tau) * ss
            for k in range(3):
                out[1 + k, j] = np.where(on, (ut[k] / umag) * tmag, F32(0.0))
            out[4, j], out[5, j], out[6, j] = u_tau, y_plus, code.astype(F32)
    return out
