"""Surface statistics: time-averaged wall pressure and shear per triangle (no reference counterpart: the reference writes the
instantaneous surface only).

Semantics ("Surface statistics"):
  * Triangle i reads its nearest fluid cell c(i) on the finest level (forces.nearest_fluid_cells, search radius 5): found once, on
    the host, from the geometry only.
  * A sample evaluates p, tau_x, tau_y, tau_z with the Float32 expressions of forces.stress_from_cells (those of k_map_stresses) on
    rho, u of the level's NEWEST state after the coarse step (statistics.t_sub_after: vel_temp if that sub-step is even, vel if odd),
    and |tau| = sqrt((tau_x tau_x + tau_y tau_y) + tau_z tau_z) in Float32, the order of save_surface_vtk's ShearMagnitude_Pa. A
    triangle with no fluid cell contributes zeros.
  * Seven Float64 sums per triangle, [7][n_tri] in COMPONENTS order; each a plain sequential `+=` of double(v) in sample order, the
    squares double(v) * double(v) (exact for a float32 v). HostSurfaceStats restates the device kernel k_accumulate_surface_stats
    bit for bit.
  * Sampled coarse steps: start_step + k interval.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from . import forces as forces_mod
from ._lib import Handle
from .blocks import BLOCK_SIZE
from .statistics import is_sample_step

F32 = np.float32
COMPONENTS = ("p", "pp", "tau_x", "tau_y", "tau_z", "tau_mag", "tau_mag2")
FORCES_MEAN_CSV_HEADER = "Step,Samples,FirstStep,LastStep,Fx_N,Fy_N,Fz_N,Mx_Nm,My_Nm,Mz_Nm,Cd,Cl,Cs,Cmy"


@dataclass
class SurfacePlan:
    """per triangle: the nearest fluid cell of the level (reference block index, -1 = none found; cell x + 8 y + 64 z), its wall
    distance in lattice units and the triangle's normal"""
    found: np.ndarray           # bool [n]
    blocks: np.ndarray          # int32 [n]
    cells: np.ndarray           # int32 [n]
    wall_dist: np.ndarray       # float32 [n]
    normals: np.ndarray         # float32 [n, 3]

    @property
    def n(self) -> int:
        return int(self.found.size)

    def subset(self, idx) -> "SurfacePlan":
        idx = np.asarray(idx, dtype=np.int64)
        return SurfacePlan(self.found[idx], self.blocks[idx], self.cells[idx], self.wall_dist[idx], self.normals[idx])


def plan_surface(mesh, level_host, params, search_radius: int = 5) -> SurfacePlan:
    """the triangle -> cell map of map_stresses_kernel! on host level `level_host` (a BlockLevel)"""
    nc = forces_mod.nearest_fluid_cells(mesh, level_host.obstacle, level_host.block_pointer, level_host.dx, params, search_radius)
    return plan_from_cells(nc, mesh)


def plan_from_cells(nc, mesh) -> SurfacePlan:
    """the plan of a forces.NearestCells"""
    blocks = np.where(nc.found, nc.block, -1).astype(np.int32)
    cells = np.where(nc.found, nc.lx + BLOCK_SIZE * nc.ly + BLOCK_SIZE * BLOCK_SIZE * nc.lz, 0).astype(np.int32)
    return SurfacePlan(nc.found.copy(), blocks, cells, nc.wall_dist.astype(np.float32),
                       np.ascontiguousarray(mesh.normals, dtype=np.float32))


def scales(params) -> Tuple[np.float32, np.float32]:
    """(pressure_scale, stress_scale) of forces.stress_from_cells"""
    s = F32(params.rho_physical * params.velocity_scale * params.velocity_scale)
    return s, s


# ---- the numpy restatement of k_accumulate_surface_stats ----
def sample_values(plan: SurfacePlan, rho: np.ndarray, vel: np.ndarray, tau, params):
    """(p, tau_x, tau_y, tau_z, |tau|) Float32 per triangle from one level's fields in the reference layout (rho [8,8,8,nb], vel
    [8,8,8,nb,3])"""
    B = BLOCK_SIZE
    n = plan.n
    best_rho = np.ones(n, dtype=F32)
    best_u = np.zeros((n, 3), dtype=F32)
    j = np.flatnonzero(plan.found)
    b, c = plan.blocks[j].astype(np.int64), plan.cells[j].astype(np.int64)
    x, y, z = c % B, (c // B) % B, c // (B * B)
    best_rho[j] = rho[x, y, z, b]
    for k in range(3):
        best_u[j, k] = vel[x, y, z, b, k]
    p, tx, ty, tz = forces_mod.stress_from_cells(best_rho, best_u, plan.wall_dist, plan.found, plan.normals, tau, params)
    mag = np.sqrt((tx * tx + ty * ty) + tz * tz).astype(F32)
    return p, tx, ty, tz, mag


def add_sample(sums: np.ndarray, values) -> None:
    """sums [7, n] Float64 += one sample's (p, tau_x, tau_y, tau_z, |tau|)"""
    p, tx, ty, tz, mag = (np.asarray(v, dtype=F32).astype(np.float64) for v in values)
    sums[0] += p
    sums[1] += p * p
    sums[2] += tx
    sums[3] += ty
    sums[4] += tz
    sums[5] += mag
    sums[6] += mag * mag


class HostSurfaceStats:
    """the sums on the host, from downloaded fields: the checker of the device set and the fallback of a stepper without one"""

    def __init__(self, plan: SurfacePlan, tau, params, start_step: int = 1, interval: int = 1):
        if int(interval) < 1:
            raise ValueError(f"surface statistics: interval {interval} < 1")
        self.plan, self.tau, self.params = plan, F32(tau), params
        self.start_step, self.interval = int(start_step), int(interval)
        self.sums = np.zeros((len(COMPONENTS), plan.n), dtype=np.float64)
        self.n = 0

    def reset(self) -> None:
        self.sums[...] = 0.0
        self.n = 0

    def accumulate(self, rho: np.ndarray, vel: np.ndarray) -> None:
        add_sample(self.sums, sample_values(self.plan, rho, vel, self.tau, self.params))
        self.n += 1

    def download(self) -> Tuple[np.ndarray, int]:
        return self.sums.copy(), self.n


# ---- the device set (ludwig_surface_stats_*) ----
class DeviceSurfaceStats(Handle):
    """a surface set on device level `device_level` (level index `level_index` of the batch's level array); plan.blocks are that
    level's own (reference-order) block indices"""
    _destroy, _closed = "ludwig_surface_stats_destroy", "surface statistics set closed"

    def __init__(self, plan: SurfacePlan, device_level, level_index: int, tau, params, start_step: int = 1, interval: int = 1):
        from . import _lib
        if int(interval) < 1:
            raise ValueError(f"surface statistics: interval {interval} < 1")
        self._lib = _lib.load()
        self.n_tri, self.level_index = plan.n, int(level_index)
        self.start_step, self.interval = int(start_step), int(interval)      # the coarse steps a batch samples
        ps, ss = scales(params)
        sp = _lib.SurfaceParams(0.0, float(F32(tau)), 0.0, 0.0, 0.0, float(ps), float(ss), 0)
        bl = np.ascontiguousarray(plan.blocks, dtype=np.int32)
        ce = np.ascontiguousarray(plan.cells, dtype=np.int32)
        wd = np.ascontiguousarray(plan.wall_dist, dtype=np.float32)
        nr = np.ascontiguousarray(plan.normals, dtype=np.float32)
        h = C.c_void_p()
        _lib.check(self._lib.ludwig_surface_stats_create(device_level.handle, plan.n, bl.ctypes.data, ce.ctypes.data, wd.ctypes.data,
                                                         nr.ctypes.data, C.byref(sp), C.byref(h)))
        self._h = h

    def is_sample_step(self, t: int) -> bool:
        return is_sample_step(t, self.start_step, self.interval)

    def reset(self) -> None:
        from . import _lib
        _lib.check(self._lib.ludwig_surface_stats_reset(self.handle))

    def accumulate(self, t_sub: int) -> None:
        from . import _lib
        _lib.check(self._lib.ludwig_surface_stats_accumulate(self.handle, int(t_sub)))

    def download(self) -> Tuple[np.ndarray, int]:
        """(sums [7, n_tri] Float64, samples)"""
        from . import _lib
        out = np.zeros((len(COMPONENTS), self.n_tri), dtype=np.float64)
        n = C.c_int64(0)
        _lib.check(self._lib.ludwig_surface_stats_download(self.handle, out.ctypes.data if out.size else None, out.nbytes, C.byref(n)))
        return out, int(n.value)


# ---- results ----
def finalize(sums: np.ndarray, n: int, params) -> Dict[str, np.ndarray]:
    """sums [7, n_tri] over n samples -> Float64 [n_tri] (mean_tau [n_tri, 3]): mean_p, p_rms = sqrt(max(<p^2> - <p>^2, 0)),
    mean_tau, mean_tau_mag, tau_mag_rms, Cp_mean, Cp_rms, Cf_mean = mean|tau| / q_inf with q_inf = rho U^2 / 2 (forces.finish_forces).
    n = 0 gives NaN everywhere."""
    s = np.asarray(sums, dtype=np.float64)
    q_inf = 0.5 * params.rho_physical * params.u_physical ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        nn = np.float64(n) if n > 0 else np.float64(np.nan)
        mean = s / nn
        p_rms = np.sqrt(np.maximum(mean[1] - mean[0] * mean[0], 0.0))
        m_rms = np.sqrt(np.maximum(mean[6] - mean[5] * mean[5], 0.0))
        if n <= 0:
            p_rms = np.full_like(p_rms, np.nan)
            m_rms = np.full_like(m_rms, np.nan)
        return {"mean_p": mean[0], "p_rms": p_rms, "mean_tau": np.stack([mean[2], mean[3], mean[4]], axis=1),
                "mean_tau_mag": mean[5], "tau_mag_rms": m_rms, "Cp_mean": mean[0] / q_inf, "Cp_rms": p_rms / q_inf,
                "Cf_mean": mean[5] / q_inf}


def mean_forces(mesh, fin: Dict[str, np.ndarray], params, symmetric: bool = False):
    """forces.ForceResult of the mean surface loads: integrate_forces_kernel!'s sums on the Float32-cast means, then finish_forces"""
    p = fin["mean_p"].astype(F32)
    tx, ty, tz = (fin["mean_tau"][:, k].astype(F32) for k in range(3))
    return forces_mod.integrate_surface_forces(mesh, p, tx, ty, tz, params, symmetric)


def save_surface_mean_vtk(filename: str, mesh, fin: Dict[str, np.ndarray], found: np.ndarray, window: Tuple[int, int, int]) -> str:
    """surface_mean_%06d.vtu: the triangle mesh of surface_%06d.vtu with Float32 cell arrays of the finalised statistics, and the
    averaging window (samples, first step, last step) as Int64 FieldData"""
    from .output import VTK_TRIANGLE, write_vtu
    n = mesh.triangles.shape[0]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    pts = np.asarray(mesh.triangles, dtype=np.float64).reshape(n * 3, 3)
    cd = [("Pressure_Pa_mean", f(fin["mean_p"])), ("Pressure_Pa_rms", f(fin["p_rms"])),
          ("ShearX_Pa_mean", f(fin["mean_tau"][:, 0])), ("ShearY_Pa_mean", f(fin["mean_tau"][:, 1])),
          ("ShearZ_Pa_mean", f(fin["mean_tau"][:, 2])), ("ShearMagnitude_Pa_mean", f(fin["mean_tau_mag"])),
          ("ShearMagnitude_Pa_rms", f(fin["tau_mag_rms"])), ("Cp_mean", f(fin["Cp_mean"])), ("Cp_rms", f(fin["Cp_rms"])),
          ("Cf_mean", f(fin["Cf_mean"])), ("Normal", f(mesh.normals)), ("Area_m2", f(mesh.areas)),
          ("MappingQuality", np.asarray(found, dtype=bool).astype(np.float32))]
    fd = [(name, np.array([v], dtype=np.int64)) for name, v in zip(("StatisticsSamples", "StatisticsFirstStep", "StatisticsLastStep"), window)]
    return write_vtu(filename, pts, np.arange(3 * n, dtype=np.int64), np.arange(1, n + 1, dtype=np.int64) * 3,
                     np.full(n, VTK_TRIANGLE, dtype=np.uint8), cd, compress=False, field_data=fd)


def forces_mean_csv_row(step: int, window: Tuple[int, int, int], fr) -> str:
    """Step,Samples,FirstStep,LastStep, then the forces, moments and coefficients to 10 significant digits (a float32 value
    reads back exactly)"""
    return ("%d,%d,%d,%d" + ",%.9e" * 10) % (
        step, window[0], window[1], window[2], fr.Fx, fr.Fy, fr.Fz, fr.Mx, fr.My, fr.Mz, fr.Cd, fr.Cl, fr.Cs, fr.Cmy)


def window_of(n: int, start_step: int, interval: int) -> Tuple[int, int, int]:
    """(samples, first sampled step, last sampled step) of n samples from start_step on"""
    return (int(n), int(start_step), int(start_step + (n - 1) * interval)) if n > 0 else (0, 0, 0)
