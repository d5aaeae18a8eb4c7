"""Force series: the integrated surface loads at every sampled coarse step, reduced on the device (no reference counterpart: the
reference integrates at diagnostics steps only).

Semantics ("Force series"):
  * The set lives on the finest level and is built from a surface_stats.SurfacePlan (the triangle -> cell map), the triangles' Float32
    areas and their Float32 moment arms (forces.moment_arms: (float32(c) + float32(off)) - float32(mc)).
  * A sample evaluates p, tau per triangle with the Float32 expressions of forces.stress_from_cells (those of k_map_stresses) on rho,
    u of the level's NEWEST state after the coarse step (statistics.t_sub_after: vel_temp if that sub-step is even, vel if odd) - not
    forces.csv's always-`vel` buffer; on a nested case the finest level ends on an odd sub-step and the two coincide - and from them
    the nine Float32 contributions of forces.force_series_contributions, in the operand order of forces.partial_force_sums.
  * The contributions are widened to Float64 and added in one fixed balanced tree over the triangles in the caller's order
    (forces.tree_sum_f64, the monitor's tree); the coverage count, |p| widened to Float64 > 1e-10
    (forces.coverage_count), is an integer sum. One record = 9 Float64 + 1 Int64:
    forces.record_of(force_series_contributions(...)) restates the device kernels bit for bit.
  * Sampled coarse steps: start_step + k interval. Records wait in a device ring of `capacity` until they are downloaded.
  * Symmetry doubling and the coefficients stay on the host: forces.finish_forces on the Float64 sums.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np

from . import forces as forces_mod
from ._lib import Handle
from .output import FORCE_CSV_HEADER, force_csv_row
from .probes import samples_in                 # noqa: F401  (one rule for every ring's samples of a batch)
from .statistics import is_sample_step         # noqa: F401  (one rule for every observer's sampled steps)
from .surface_stats import SurfacePlan, scales

F32 = np.float32


class DeviceForceSeries(Handle):
    """a force-series set on device level `device_level` (level index `level_index` of the batch's level array); plan.blocks are that
    level's own (reference-order) block indices; area [n] and arm [3, n] Float32 in the plan's triangle order"""
    _destroy, _closed = "ludwig_force_series_destroy", "force series closed"

    def __init__(self, plan: SurfacePlan, area, arm, device_level, level_index: int, tau, params, start_step: int = 1, interval: int = 1,
                 capacity: int = 64):
        from . import _lib
        if int(interval) < 1:
            raise ValueError(f"force series: interval {interval} < 1")
        if int(capacity) < 1:
            raise ValueError(f"force series: capacity {capacity} < 1")
        self._lib = _lib.load()
        self.n_tri, self.level_index, self.capacity = plan.n, int(level_index), int(capacity)
        self.start_step, self.interval = int(start_step), int(interval)      # the coarse steps a batch samples
        ps, ss = scales(params)
        sp = _lib.SurfaceParams(0.0, float(F32(tau)), 0.0, 0.0, 0.0, float(ps), float(ss), 0)
        bl = np.ascontiguousarray(plan.blocks, dtype=np.int32)
        ce = np.ascontiguousarray(plan.cells, dtype=np.int32)
        wd = np.ascontiguousarray(plan.wall_dist, dtype=np.float32)
        nr = np.ascontiguousarray(plan.normals, dtype=np.float32)
        ar = np.ascontiguousarray(area, dtype=np.float32)
        am = np.ascontiguousarray(arm, dtype=np.float32)
        if ar.shape != (plan.n,) or am.shape != (3, plan.n):
            raise ValueError(f"force series: area {ar.shape} / arm {am.shape} for {plan.n} triangles")
        h = C.c_void_p()
        _lib.check(self._lib.ludwig_force_series_create(device_level.handle, plan.n, bl.ctypes.data, ce.ctypes.data, wd.ctypes.data,
                                                        nr.ctypes.data, ar.ctypes.data, am.ctypes.data, C.byref(sp), self.capacity,
                                                        C.byref(h)))
        self._h = h

    def is_sample_step(self, t: int) -> bool:
        return is_sample_step(t, self.start_step, self.interval)

    def sample(self, t_sub: int, t_coarse: int) -> None:
        from . import _lib
        _lib.check(self._lib.ludwig_force_series_sample(self.handle, int(t_sub), int(t_coarse)))

    def download(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(coarse steps [n] int64, sums [n, 9] Float64, covered [n] int64) taken since the last download; empties the ring"""
        from . import _lib
        sums = np.empty((self.capacity, 9), dtype=np.float64)
        cov = np.empty(self.capacity, dtype=np.int64)
        steps = np.empty(self.capacity, dtype=np.int64)
        n = C.c_int32(0)
        _lib.check(self._lib.ludwig_force_series_download(self.handle, sums.ctypes.data, cov.ctypes.data, steps.ctypes.data, self.capacity,
                                                          C.byref(n)))
        return steps[: n.value].copy(), sums[: n.value].copy(), cov[: n.value].copy()


def from_mesh(mesh, plan: SurfacePlan, device_level, level_index: int, tau, params, start_step: int = 1, interval: int = 1,
              capacity: int = 64, select=None) -> DeviceForceSeries:
    """the set of `mesh` over `plan` (of all its triangles, or of the triangles `select` in that order: one rank's share)"""
    area = mesh.areas.astype(np.float32)
    if select is not None:
        area = area[select]
    return DeviceForceSeries(plan, area, forces_mod.moment_arms(mesh, params, select), device_level, level_index, tau, params, start_step,
                             interval, capacity)


def host_record(mesh, plan: SurfacePlan, rho: np.ndarray, vel: np.ndarray, tau, params, select=None) -> Tuple[np.ndarray, int]:
    """(sums [9] Float64, covered) of one record from a level's fields in the reference layout: the restatement of a device sample"""
    from .surface_stats import sample_values
    p, tx, ty, tz, _ = sample_values(plan, rho, vel, tau, params)
    contrib, covered = forces_mod.force_series_contributions(mesh, p, tx, ty, tz, params, select)
    return forces_mod.record_of(contrib), covered


class Series:
    """the host copy of a force series: appended after every drain into buffers that double when full, so a run's appends cost O(1)
    each; take_new() hands out what came since the last take_new() (what run_case writes after a batch), arrays() the whole history.
    Per record Float64 sums of shape sums_shape and Int64 counts of shape count_shape (the force series: 9 sums, one coverage count;
    flux_planes.Series: per plane)"""

    def __init__(self, sums_shape: Tuple[int, ...] = (9,), count_shape: Tuple[int, ...] = ()):
        self._n = 0
        self._taken = 0
        self._sums_shape, self._count_shape = tuple(sums_shape), tuple(count_shape)
        self._steps = np.empty(64, np.int64)
        self._sums = np.empty((64,) + self._sums_shape, np.float64)
        self._cov = np.empty((64,) + self._count_shape, np.int64)

    def append(self, steps: np.ndarray, sums: np.ndarray, covered: np.ndarray) -> None:
        k = len(steps)
        if k == 0:
            return
        if self._n + k > self._steps.size:
            size = max(2 * self._steps.size, self._n + k)
            self._steps, self._sums, self._cov = (np.concatenate([a, np.empty((size - a.shape[0],) + a.shape[1:], a.dtype)])
                                                  for a in (self._steps, self._sums, self._cov))
        sl = slice(self._n, self._n + k)
        self._steps[sl] = steps
        self._sums[sl] = np.asarray(sums, dtype=np.float64).reshape((-1,) + self._sums_shape)
        self._cov[sl] = np.asarray(covered).reshape((-1,) + self._count_shape)
        self._n += k

    def _range(self, lo: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        return self._steps[lo:self._n].copy(), self._sums[lo:self._n].copy(), self._cov[lo:self._n].copy()

    def arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(steps [n], sums [n, 9], covered [n]) of every record so far"""
        return self._range(0)

    def take_new(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """the records appended since the last take_new()"""
        lo, self._taken = self._taken, self._n
        return self._range(lo)


def segment_end(t: int, end: int, start_step: int, interval: int, free: int) -> int:
    """the last coarse step of t..end a batch may run to before a ring with `free` free records would overflow"""
    if samples_in(t, end, start_step, interval) <= free:
        return end
    first = start_step + max(0, -(-(t - start_step) // interval)) * interval
    return first + (free - 1) * interval


# ---- result file ----
def csv_header() -> str:
    """forces.csv's columns plus Coverage"""
    return FORCE_CSV_HEADER + ",Coverage"


def csv_row(step: int, time_phys: float, fr, u_curr) -> str:
    """forces.csv's row (output.force_csv_row: same columns, same printf formats) of a forces.ForceResult, plus its coverage count"""
    return force_csv_row(step, time_phys, fr, u_curr) + ",%d" % int(fr.coverage)


def mean_rms(values) -> Tuple[float, float]:
    """(mean, rms about the mean) of a sequence; (nan, nan) when it is empty"""
    v = np.asarray(list(values), dtype=np.float64)
    if v.size == 0:
        return float("nan"), float("nan")
    m = float(v.mean())
    return m, float(np.sqrt(np.mean((v - m) ** 2)))
