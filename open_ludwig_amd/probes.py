"""Probes: time series of rho and u at points (no reference counterpart: the reference writes no monitor points).

Semantics ("Probes"):
  * Points are given in the STL's own coordinates after stl_scale and map to the domain frame - the frame of the flow file's point
    coordinates - by + params.mesh_offset.
  * A probe is sampled on the FINEST level whose active blocks hold its base cell: per axis g = p_domain / dx - 0.5, base cell
    i0 = floor(g), weights w = g - i0, both in float64 on the host; the weights are then cast to float32. A point outside the domain,
    or whose base cell is an obstacle cell, is refused at set-up with a message that names the probe.
  * The stencil is the 8 cells i0 + {0,1}^3, corner c = dx + 2 dy + 4 dz. A corner that is no fluid cell of an active block OF THAT
    LEVEL is replaced by the base cell: one rule for the domain edge, the edge of a refinement level and the body surface (no parent
    interpolation).
  * Values: rho, ux, uy, uz in lattice units (the flow file's Density / Velocity), trilinear in float32 in one fixed order - x first,
    then y, then z, each lerp (1 - w) a + w b (`trilinear` below; on the device kernels.hpp probe_trilinear, gathered by stencil_sample for
    k_probe_sample, evaluates the same expressions with -ffp-contract=off, bit for bit) - from the level's NEWEST state after the coarse step (statistics.t_sub_after; vel_temp if that
    sub-step is even, vel if odd).
  * Sampled coarse steps: start_step + k interval.
Physical units: u_phys = u * (U_phys / u_lattice) = u * params.velocity_scale.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import Handle
from .blocks import BLOCK_SIZE
from .statistics import is_sample_step         # (one rule for every observer's sampled steps)

F32 = np.float32
QUANTITIES = ("rho", "ux", "uy", "uz")


@dataclass
class ProbePlan:
    names: List[str]
    points: np.ndarray          # [n, 3] float64, as given (STL frame)
    domain: np.ndarray          # [n, 3] float64, domain frame
    level: np.ndarray           # [n] int32, 0-based level index
    blocks: np.ndarray          # [n, 8] int32, reference block index (0-based) of every stencil corner
    cells: np.ndarray           # [n, 8] int32, x + 8 y + 64 z within that block
    weights: np.ndarray         # [n, 3] float32, along x, y, z
    replaced: np.ndarray        # [n, 8] bool, the corner was replaced by the base cell

    @property
    def n(self) -> int:
        return len(self.names)

    def subset(self, idx) -> "ProbePlan":
        idx = np.asarray(idx, dtype=np.int64)
        return ProbePlan([self.names[i] for i in idx], self.points[idx], self.domain[idx], self.level[idx], self.blocks[idx],
                         self.cells[idx], self.weights[idx], self.replaced[idx])


def default_names(n: int) -> List[str]:
    return [f"p{i}" for i in range(n)]


def plan_probes(points, grids: Sequence, offset=(0.0, 0.0, 0.0), names: Optional[Sequence[str]] = None) -> ProbePlan:
    """points [n, 3] (STL frame) + offset -> the plan over `grids` (host BlockLevels, level 1 first). ValueError names the probe."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    names = list(names) if names is not None else default_names(n)
    if len(names) != n:
        raise ValueError(f"probes: {len(names)} names for {n} points")
    dom = pts + np.asarray(offset, dtype=np.float64).reshape(1, 3)
    B = BLOCK_SIZE
    l1 = grids[0]
    extent = np.array([l1.grid_dim_x, l1.grid_dim_y, l1.grid_dim_z], dtype=np.float64) * B * float(l1.dx)
    level = np.zeros(n, np.int32)
    blocks = np.zeros((n, 8), np.int32)
    cells = np.zeros((n, 8), np.int32)
    weights = np.zeros((n, 3), np.float32)
    replaced = np.zeros((n, 8), bool)
    for p in range(n):
        q = dom[p]
        if not np.all(np.isfinite(q)) or np.any(q < 0.0) or np.any(q > extent):
            raise ValueError(f"probe {names[p]!r} at {pts[p].tolist()} (domain frame {q.tolist()}) lies outside the domain "
                             f"[0, {extent[0]}] x [0, {extent[1]}] x [0, {extent[2]}]")
        chosen = None
        for li in range(len(grids) - 1, -1, -1):
            g = grids[li]
            gg = q / float(g.dx) - 0.5
            i0 = np.floor(gg).astype(np.int64)
            if _cell(g, i0) is not None:
                chosen = (li, gg, i0)
                break
        if chosen is None:
            raise ValueError(f"probe {names[p]!r} at {pts[p].tolist()}: its base cell lies outside the domain (within half a cell of a face)")
        li, gg, i0 = chosen
        g = grids[li]
        bc = _cell(g, i0)
        if g.obstacle[bc[1], bc[2], bc[3], bc[0]]:
            raise ValueError(f"probe {names[p]!r} at {pts[p].tolist()}: its base cell on level {g.level_id} is an obstacle cell (inside the body)")
        level[p] = li
        weights[p] = (gg - i0).astype(np.float32)
        for c in range(8):
            d = np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.int64)
            cc = _cell(g, i0 + d)
            if cc is None or g.obstacle[cc[1], cc[2], cc[3], cc[0]]:
                cc = bc
                replaced[p, c] = c != 0
            blocks[p, c] = cc[0]
            cells[p, c] = cc[1] + B * cc[2] + B * B * cc[3]
    return ProbePlan(names, pts, dom, level, blocks, cells, weights, replaced)


def _cell(g, i) -> Optional[Tuple[int, int, int, int]]:
    """(reference block index, x, y, z) of global 0-based cell i on level g, None if no active block holds it"""
    B = BLOCK_SIZE
    dims = (g.grid_dim_x, g.grid_dim_y, g.grid_dim_z)
    if any(i[a] < 0 or i[a] >= dims[a] * B for a in range(3)):
        return None
    b = int(g.block_pointer[i[0] // B, i[1] // B, i[2] // B])
    if b <= 0:
        return None
    return b - 1, int(i[0] % B), int(i[1] % B), int(i[2] % B)


# ---- the numpy restatement of k_probe_sample ----
def trilinear(v: np.ndarray, w: np.ndarray) -> np.ndarray:
    """v [..., 8] float32 (corner c = dx + 2 dy + 4 dz), w [..., 3] float32 -> [...] float32: x first, then y, then z, each lerp
    evaluated as (1 - w) a + w b with every product and sum rounded to float32 on its own"""
    v = np.asarray(v, dtype=F32)
    w = np.asarray(w, dtype=F32)
    one = F32(1.0)

    def lerp(a, b, t):
        return (one - t) * a + t * b

    wx, wy, wz = w[..., 0:1], w[..., 1:2], w[..., 2:3]
    x = lerp(v[..., 0::2], v[..., 1::2], wx)              # (0,1) (2,3) (4,5) (6,7)
    y = lerp(x[..., 0::2], x[..., 1::2], wy)              # (00,10) (01,11)
    return lerp(y[..., 0:1], y[..., 1:2], wz)[..., 0]


def gather(plan: ProbePlan, idx: np.ndarray, rho: np.ndarray, vel: np.ndarray) -> np.ndarray:
    """the stencil values [len(idx), 4, 8] of probes idx from one level's fields in the reference layout (rho [8,8,8,nb], vel
    [8,8,8,nb,3])"""
    B = BLOCK_SIZE
    b, c = plan.blocks[idx].astype(np.int64), plan.cells[idx].astype(np.int64)
    x, y, z = c % B, (c // B) % B, c // (B * B)
    out = np.empty((len(idx), 4, 8), dtype=F32)
    out[:, 0] = rho[x, y, z, b]
    for k in range(3):
        out[:, 1 + k] = vel[x, y, z, b, k]
    return out


def sample_fields(plan: ProbePlan, fields: Callable[[int], Tuple[np.ndarray, np.ndarray]]) -> np.ndarray:
    """[n, 4] float32 (rho, ux, uy, uz) of every probe; fields(level index) -> (rho, vel buffer) of that level"""
    out = np.full((plan.n, 4), np.nan, dtype=F32)
    for li in np.unique(plan.level):
        idx = np.flatnonzero(plan.level == li)
        rho, vel = fields(int(li))
        out[idx] = trilinear(gather(plan, idx, rho, vel), plan.weights[idx][:, None, :])
    return out


# ---- the device probe set (ludwig_probes_*) ----
class DeviceProbes(Handle):
    """a probe set over device levels (DeviceLevel, or None for a level no probe of the plan is on); plan.blocks are the levels' own
    (reference-order) block indices"""
    _destroy, _closed = "ludwig_probes_destroy", "probe set closed"

    def __init__(self, plan: ProbePlan, levels: Sequence, capacity: int, start_step: int = 1, interval: int = 1):
        from . import _lib
        if int(interval) < 1:
            raise ValueError(f"probes: interval {interval} < 1")
        self._lib = _lib.load()
        self.n_probes, self.capacity = plan.n, int(capacity)
        self.start_step, self.interval = int(start_step), int(interval)      # the coarse steps a batch samples
        self.levels_with_probes = sorted({int(l) for l in plan.level})
        self.n_levels = len(levels)
        arr = (C.c_void_p * len(levels))(*[(lv.handle if lv is not None else None) for lv in levels])
        li = np.ascontiguousarray(plan.level, dtype=np.int32)
        bl = np.ascontiguousarray(plan.blocks, dtype=np.int32)
        ce = np.ascontiguousarray(plan.cells, dtype=np.int32)
        w = np.ascontiguousarray(plan.weights, dtype=np.float32)
        h = C.c_void_p()
        _lib.check(self._lib.ludwig_probes_create(arr, len(levels), plan.n, li.ctypes.data, bl.ctypes.data, ce.ctypes.data, w.ctypes.data,
                                                  self.capacity, C.byref(h)))
        self._h = h

    def is_sample_step(self, t: int) -> bool:
        return is_sample_step(t, self.start_step, self.interval)

    def sample(self, level_index: int, t_sub: int) -> None:
        from . import _lib
        _lib.check(self._lib.ludwig_probes_sample(self.handle, int(level_index), int(t_sub)))

    def download(self) -> Tuple[np.ndarray, np.ndarray]:
        """(coarse steps [n] int64, values [n, n_probes, 4] float32) taken since the last download; empties the ring"""
        from . import _lib
        vals = np.empty((self.capacity, self.n_probes, 4), dtype=np.float32)
        steps = np.empty(self.capacity, dtype=np.int64)
        n = C.c_int32(0)
        _lib.check(self._lib.ludwig_probes_download(self.handle, vals.ctypes.data, steps.ctypes.data, self.capacity, C.byref(n)))
        return steps[: n.value].copy(), vals[: n.value].copy()


def samples_in(first: int, last: int, start_step: int, interval: int) -> int:
    lo = max(first, start_step)
    if last < lo:
        return 0
    s0 = start_step + (-(-(lo - start_step) // interval)) * interval
    return 0 if s0 > last else (last - s0) // interval + 1


class Series:
    """the host copy of a probe series: appended after every drain"""

    def __init__(self, n_probes: int):
        self.n_probes = n_probes
        self._steps: List[np.ndarray] = []
        self._vals: List[np.ndarray] = []

    def append(self, steps: np.ndarray, values: np.ndarray) -> None:
        if len(steps):
            self._steps.append(np.asarray(steps, dtype=np.int64))
            self._vals.append(np.asarray(values, dtype=np.float32))

    def arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        if not self._steps:
            return np.zeros(0, np.int64), np.zeros((0, self.n_probes, 4), np.float32)
        return np.concatenate(self._steps), np.concatenate(self._vals)


# ---- result files ----
def f32_text(x) -> str:
    """the shortest decimal that reads back to the same float32"""
    return str(F32(x))                                     # numpy prints the shortest unique digits of the float32


def write_points_csv(path: str, plan: ProbePlan, grids: Sequence) -> None:
    with open(path, "w") as io:
        io.write("name,x,y,z,x_domain,y_domain,z_domain,level\n")
        for p in range(plan.n):
            io.write(",".join([plan.names[p], *(repr(float(v)) for v in plan.points[p]), *(repr(float(v)) for v in plan.domain[p]),
                               str(int(grids[int(plan.level[p])].level_id))]) + "\n")


def series_csv_header(names: Sequence[str]) -> str:
    return ",".join(["step", "time"] + [f"{nm}_{q}" for nm in names for q in QUANTITIES])


def series_csv_rows(steps: np.ndarray, values: np.ndarray, time_scale: float) -> List[str]:
    """step,time,<name>_rho,<name>_ux,<name>_uy,<name>_uz,... - time = step * time_scale as forces.csv prints it"""
    return [",".join([str(int(s)), "%.6e" % (float(s) * time_scale)] + [f32_text(v) for v in values[i].reshape(-1)])
            for i, s in enumerate(steps)]


def read_series_csv(path: str) -> Tuple[List[str], np.ndarray, np.ndarray]:
    """(header fields, steps [n], values [n, n_probes, 4] float32) of a probes.csv"""
    with open(path) as io:
        head = io.readline().strip().split(",")
        rows = [l.strip().split(",") for l in io if l.strip()]
    n_p = (len(head) - 2) // 4
    steps = np.array([int(r[0]) for r in rows], dtype=np.int64)
    vals = np.array([[np.float32(v) for v in r[2:]] for r in rows], dtype=np.float32).reshape(len(rows), n_p, 4)
    return head, steps, vals
