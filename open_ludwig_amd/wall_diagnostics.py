"""Wall diagnostics: the y+, friction velocity and modelled wall shear the wall model works with (no reference counterpart: the
reference reads y_plus_target and never computes a y+).

Semantics ("Wall diagnostics"):
  * The wall-model state of a cell - u_tau, y+ = u_tau wall_dist / nu with the FINAL u_tau, and a branch code - is evaluated on the
    device only (kernels.hpp wall_model_state, the float32 restatement of the step's wall_model_force_mag); this package holds no host
    restatement of its pow / log. Code: 0 not near the wall or an obstacle cell, 1 near the wall with the model skipped, 2 power law kept,
    3 log law applied; FORCED (4) is or-ed in where the step applies a force.
  * The census of a level (ludwig_level_wall_census) is all integers: counts, the float32 bits of the least and greatest y+, and a
    histogram with eight bins per octave whose bin is a shift of those bits (bin_of). Records of ranks add up exactly (merge).
  * Percentiles and the band share come from the histogram: percentile(hist, q) is the LOWER EDGE of the bin that holds the q-quantile,
    and a bin counts as inside a band [lo, hi) when its lower edge does.
  * The surface set (ludwig_wall_surface_*) gives per triangle of the finest level p, the modelled shear vector, u_tau, y+ and the code,
    from the state at a batch's end.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import forces as forces_mod
from ._lib import Handle
from .surface_stats import SurfacePlan, scales

F32 = np.float32
N_BINS = 194
E8_FIRST, E8_END = 936, 1128            # bits >> 20 of 2^-10 and of 2^14
ROWS = ("p", "tau_x", "tau_y", "tau_z", "u_tau", "y_plus", "code")
CODE_FAR, CODE_SKIPPED, CODE_POWER, CODE_LOG, CODE_FORCED = 0, 1, 2, 3, 4
NO_MIN, NO_MAX = 0xFFFFFFFF, 0

WALL_MODEL_CSV_HEADER = "Step,Level,NearCells,Evaluated,LogLaw,Forced,NonFinite,YPlusMin,YPlusP05,YPlusMedian,YPlusP95,YPlusMax,ShareInBand"
WALL_FORCES_CSV_HEADER = "Step,AreaMeanYPlus,MappedTriangles,Fx_N,Fy_N,Fz_N,Mx_Nm,My_Nm,Mz_Nm,Cd,Cl,Cs,Cmy"


# ---- the histogram's bit rule ----
def bin_of(y_plus) -> np.ndarray:
    """the bin of positive finite float32 values (+0 included): with e8 = bits >> 20, bin 0 if e8 < 936 (below 2^-10),
    1 + (e8 - 936) for 936 <= e8 < 1128, 193 from 2^14 on; int64, the shape of the input"""
    e8 = (np.asarray(y_plus, dtype=F32).view(np.uint32) >> np.uint32(20)).astype(np.int64)
    return np.where(e8 < E8_FIRST, 0, np.where(e8 >= E8_END, N_BINS - 1, 1 + (e8 - E8_FIRST)))


def bin_edges() -> np.ndarray:
    """float32 [194]: the lower edge of every bin - 0 for bin 0, the float with bits (935 + j) << 20 for bin j in 1..193"""
    bits = (np.arange(N_BINS, dtype=np.uint32) + np.uint32(E8_FIRST - 1)) << np.uint32(20)
    bits[0] = 0
    return bits.view(F32)


def percentile(hist, q: float) -> float:
    """the lower edge of the bin that holds the q-quantile (0 <= q <= 1) of a histogram: the first bin at which the running count
    reaches max(ceil(q n), 1); NaN for an empty histogram"""
    h = np.asarray(hist, dtype=np.int64)
    n = int(h.sum())
    if n == 0:
        return float("nan")
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"percentile: q = {q} not in [0, 1]")
    k = max(int(np.ceil(q * n)), 1)
    return float(bin_edges()[int(np.searchsorted(np.cumsum(h), k))])


def share_in_band(hist, band: Tuple[float, float]) -> float:
    """the share of a histogram's count in the bins whose lower edge lies in [lo, hi); NaN for an empty histogram"""
    h = np.asarray(hist, dtype=np.int64)
    n = int(h.sum())
    if n == 0:
        return float("nan")
    e = bin_edges().astype(np.float64)
    return float(h[(e >= float(band[0])) & (e < float(band[1]))].sum()) / n


# ---- the census record ----
@dataclass
class Census:
    near_cells: int = 0
    evaluated: int = 0
    log_law: int = 0
    forced: int = 0
    non_finite: int = 0
    min_bits: int = NO_MIN
    max_bits: int = NO_MAX
    hist: np.ndarray = field(default_factory=lambda: np.zeros(N_BINS, dtype=np.uint64))

    def __eq__(self, other) -> bool:
        return isinstance(other, Census) and all(getattr(self, n) == getattr(other, n) for n in _COUNTS + ("min_bits", "max_bits")) \
            and np.array_equal(self.hist, other.hist)

    @property
    def y_plus_min(self) -> float:
        return float(np.array(self.min_bits, np.uint32).view(F32)) if self.evaluated else float("nan")

    @property
    def y_plus_max(self) -> float:
        return float(np.array(self.max_bits, np.uint32).view(F32)) if self.evaluated else float("nan")


_COUNTS = ("near_cells", "evaluated", "log_law", "forced", "non_finite")


def merge(records: Sequence[Optional[Census]]) -> Census:
    """the record of a level from the records of its ranks (None: a rank that holds nothing of it): integers add, min / max of the bits"""
    out = Census()
    for rec in records:
        if rec is None:
            continue
        for name in _COUNTS:
            setattr(out, name, getattr(out, name) + getattr(rec, name))
        out.min_bits, out.max_bits = min(out.min_bits, rec.min_bits), max(out.max_bits, rec.max_bits)
        out.hist = out.hist + np.asarray(rec.hist, dtype=np.uint64)
    return out


def census(device_level, t_sub: int) -> Census:
    """ludwig_level_wall_census of a blocks.DeviceLevel: its owned blocks, the newest state after sub-step t_sub"""
    from . import _lib
    rec = _lib.WallCensus()
    _lib.check(_lib.load().ludwig_level_wall_census(device_level.handle, int(t_sub), C.byref(rec)))
    return Census(*(int(getattr(rec, n)) for n in _COUNTS), int(rec.min_bits), int(rec.max_bits), np.array(rec.hist[:], dtype=np.uint64))


def check_band(band) -> Tuple[float, float]:
    """advanced.wall_diagnostics.band: two numbers with 0 < lo < hi"""
    try:
        lo, hi = (float(v) for v in band)
    except (TypeError, ValueError):
        raise ValueError(f"advanced.wall_diagnostics.band must be two numbers [lo, hi], got {band!r}")
    if not (0.0 < lo < hi):
        raise ValueError(f"advanced.wall_diagnostics.band must satisfy 0 < lo < hi, got {band!r}")
    return lo, hi


def _num(x) -> str:
    from .output import _shortest
    return "nan" if x != x else _shortest(x)


def wall_model_csv_header(y_plus_target, band) -> str:
    """the comment line that echoes the case's y_plus_target and the band, then the column names"""
    return f"# y_plus_target = {_num(np.float64(y_plus_target))}, band = [{_num(np.float64(band[0]))}, {_num(np.float64(band[1]))})\n" + WALL_MODEL_CSV_HEADER


def wall_model_csv_row(step: int, level: int, rec: Census, band) -> str:
    """one wall_model.csv row: the counts, min / max y+ as shortest round-trip float32 decimals, the percentiles as bin edges"""
    cols = [str(int(step)), str(int(level))] + [str(getattr(rec, n)) for n in _COUNTS]
    cols += [_num(F32(v)) for v in (rec.y_plus_min, percentile(rec.hist, 0.05), percentile(rec.hist, 0.5), percentile(rec.hist, 0.95),
                                    rec.y_plus_max)]
    cols.append(_num(np.float64(share_in_band(rec.hist, band))))
    return ",".join(cols)


# ---- the device surface set (ludwig_wall_surface_*) ----
class DeviceWallSurface(Handle):
    """a wall-surface set on device level `device_level`; plan.blocks are that level's own (reference-order) block indices. The plan's
    own wall_dist is not used: the model reads the level's wall_dist array at the cell."""
    _destroy, _closed = "ludwig_wall_surface_destroy", "wall surface set closed"

    def __init__(self, plan: SurfacePlan, device_level, params):
        from . import _lib
        self._lib = _lib.load()
        self.n_tri = plan.n
        ps, ss = scales(params)
        sp = _lib.SurfaceParams(0.0, 0.0, 0.0, 0.0, 0.0, float(ps), float(ss), 0)
        bl = np.ascontiguousarray(plan.blocks, dtype=np.int32)
        ce = np.ascontiguousarray(plan.cells, dtype=np.int32)
        nr = np.ascontiguousarray(plan.normals, dtype=np.float32)
        h = C.c_void_p()
        _lib.check(self._lib.ludwig_wall_surface_create(device_level.handle, plan.n, bl.ctypes.data, ce.ctypes.data, nr.ctypes.data,
                                                        C.byref(sp), C.byref(h)))
        self._h = h

    def compute(self, t_sub: int) -> None:
        from . import _lib
        _lib.check(self._lib.ludwig_wall_surface_compute(self.handle, int(t_sub)))

    def download(self) -> np.ndarray:
        """values [7, n_tri] float32 in ROWS order"""
        from . import _lib
        out = np.zeros((len(ROWS), self.n_tri), dtype=np.float32)
        _lib.check(self._lib.ludwig_wall_surface_download(self.handle, out.ctypes.data if out.size else None, out.nbytes))
        return out


# ---- results ----
def finalize(values: np.ndarray, params) -> Dict[str, np.ndarray]:
    """values [7, n_tri] -> the float32 arrays of the surface file: YPlus, FrictionVelocity_m_s = u_tau velocity_scale,
    WallShearModel{X,Y,Z}_Pa, WallShearModelMagnitude_Pa = sqrt((x x + y y) + z z), Cf_model = |tau_w| / q_inf, WallModelBranch"""
    v = np.asarray(values, dtype=F32)
    tx, ty, tz = v[1], v[2], v[3]
    with np.errstate(over="ignore", invalid="ignore"):
        mag = np.sqrt((tx * tx + ty * ty) + tz * tz).astype(F32)
        q_inf = F32(0.5 * params.rho_physical * params.u_physical ** 2)
        return {"YPlus": v[5].copy(), "FrictionVelocity_m_s": (v[4] * F32(params.velocity_scale)).astype(F32),
                "WallShearModelX_Pa": tx.copy(), "WallShearModelY_Pa": ty.copy(), "WallShearModelZ_Pa": tz.copy(),
                "WallShearModelMagnitude_Pa": mag, "Cf_model": (mag / q_inf).astype(F32), "WallModelBranch": v[6].copy()}


def model_forces(mesh, values: np.ndarray, params, symmetric: bool = False):
    """forces.ForceResult of the pressure plus the MODELLED wall shear: integrate_forces_kernel!'s sums on p and tau_model"""
    v = np.asarray(values, dtype=F32)
    return forces_mod.integrate_surface_forces(mesh, v[0], v[1], v[2], v[3], params, symmetric)


def area_mean_y_plus(mesh, values: np.ndarray) -> Tuple[float, int]:
    """(Float64 area-weighted mean of y+ over the triangles with code >= 2, summed sequentially in triangle order; their number);
    NaN without such a triangle"""
    v = np.asarray(values, dtype=F32)
    area = np.asarray(mesh.areas, dtype=np.float64)
    num = den = 0.0
    n = 0
    for i in np.flatnonzero((v[6].astype(np.int64) & 3) >= CODE_POWER):
        num += area[i] * float(v[5, i])
        den += area[i]
        n += 1
    return (num / den if den > 0.0 else float("nan")), n


def wall_forces_csv_row(step: int, mesh, values: np.ndarray, fr) -> str:
    """Step, AreaMeanYPlus, MappedTriangles, then the forces, moments and coefficients to 10 significant digits"""
    mean, n = area_mean_y_plus(mesh, values)
    return ("%d,%s,%d" + ",%.9e" * 10) % (step, _num(np.float64(mean)), n, fr.Fx, fr.Fy, fr.Fz, fr.Mx, fr.My, fr.Mz, fr.Cd, fr.Cl, fr.Cs, fr.Cmy)
