"""Flow monitor: one health record per level - compute_flow_stats of the reference (src/diagnostics.jl:56-94) for every level, plus
the non-finite count and WHERE each extreme sits, and the warnings of its check_stability (src/diagnostics.jl:99-125, never called
there).

The record ("Flow monitor"), from a level's newest state - rho, the velocity buffer its last sub-step wrote, and
obstacle - over the owned blocks:
  * per non-obstacle ("fluid") cell v2 = (ux ux + uy uy) + uz uz in float32, in this order; the cell is COUNTED iff rho, ux, uy, uz
    and v2 are all finite, else BAD;
  * n_fluid, n_bad;
  * rho_min, rho_max, v2_max over the counted cells (IEEE < and >), each with its cell; among equal values the cell lowest in
    (bx, by, bz, k, j, i) order wins, whatever order the blocks are listed in; first_bad is the lowest bad cell. Without a counted
    cell: +inf, -inf, -inf and no cells;
  * sum_rho and sum_rho_v2 = sum of double(rho) double(v2) in Float64 over the counted cells (every other cell adds +0.0), in one fixed
    balanced tree: x = x[0::2] + x[1::2] nine times over a block's 512 cells in cell order, then the same halving over the per-block
    results in the level's block order, +0.0 appended wherever a length is odd (`tree_sum`).
A cell is (bx, by, bz, cell) with the level's 1-based block coordinates and cell = i + 8 j + 64 k, so records of ranks merge.

The device computes the record in ludwig_level_monitor (k_monitor_blocks, k_monitor_combine); host_monitor below restates it bit for
bit and serves a stepper without the device call.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import List, Optional, Sequence, Tuple

import numpy as np

F32, F64 = np.float32, np.float64
B = 8                       # cells per block edge
CELLS = B * B * B
Cell = Tuple[int, int, int, int]      # (bx, by, bz, i + 8 j + 64 k)

# check_stability's thresholds (src/diagnostics.jl:104-114)
SPEED_WARN, RHO_LOW_WARN, RHO_HIGH_WARN = 0.3, 0.5, 1.5


@dataclass
class Record:
    n_fluid: int = 0
    n_bad: int = 0
    rho_min: np.float32 = F32(np.inf)
    rho_max: np.float32 = F32(-np.inf)
    v2_max: np.float32 = F32(-np.inf)
    cell_rho_min: Optional[Cell] = None
    cell_rho_max: Optional[Cell] = None
    cell_v2_max: Optional[Cell] = None
    first_bad: Optional[Cell] = None
    sum_rho: np.float64 = F64(0.0)
    sum_rho_v2: np.float64 = F64(0.0)

    # -- derived on the host in Float64 --
    @property
    def n_counted(self) -> int:
        return self.n_fluid - self.n_bad

    @property
    def rho_mean(self) -> float:
        return float(self.sum_rho) / self.n_counted if self.n_counted > 0 else float("nan")

    @property
    def speed_max(self) -> float:
        """sqrt of the float32 v2_max: sqrt is monotone and correctly rounded, so this is the maximum of the per-cell speeds"""
        return math.sqrt(float(self.v2_max)) if self.cell_v2_max is not None else float("nan")

    @property
    def mach(self) -> float:
        return self.speed_max * math.sqrt(3.0)

    @property
    def kinetic_energy(self) -> float:
        return 0.5 * float(self.sum_rho_v2)

    def same_but_sums(self, other: "Record") -> bool:
        """every field but the two Float64 sums (which depend on how the blocks are spread over ranks)"""
        return all(getattr(self, f.name) == getattr(other, f.name) for f in fields(self) if f.name not in ("sum_rho", "sum_rho_v2"))


def from_arrays(counts, cells, extremes, sums) -> Record:
    """ludwig_level_monitor's output arrays -> Record"""
    cells = np.asarray(cells, dtype=np.int64).reshape(4, 4)
    c = [None if row[0] < 0 else tuple(int(v) for v in row) for row in cells]
    return Record(int(counts[0]), int(counts[1]), F32(extremes[0]), F32(extremes[1]), F32(extremes[2]), c[0], c[1], c[2], c[3],
                  F64(sums[0]), F64(sums[1]))


def tree_sum(x: np.ndarray) -> np.float64:
    """the fixed balanced tree over a 1-D Float64 array: adjacent pairs halved until one value is left, +0.0 appended wherever the
    length is odd; the empty array gives +0.0"""
    x = np.asarray(x, dtype=F64).reshape(-1)
    if x.size == 0:
        return F64(0.0)
    while x.size > 1:
        if x.size % 2:
            x = np.concatenate([x, np.zeros(1, F64)])
        x = x[0::2] + x[1::2]
    return F64(x[0])


def _block_sums(x: np.ndarray) -> np.ndarray:
    """[n_blocks, 512] Float64 -> [n_blocks]: nine halvings over the cells of each block"""
    for _ in range(9):
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def host_monitor(rho: np.ndarray, vel: np.ndarray, obstacle: np.ndarray, block_coords, n_owned: Optional[int] = None) -> Record:
    """the record of one level from its fields in the reference layout: rho [8,8,8,nb] float32, vel [8,8,8,nb,3] (the buffer the last
    sub-step wrote), obstacle [8,8,8,nb] bool, block_coords [nb] of (bx, by, bz); only blocks [0, n_owned) are read (default: all)"""
    nb = int(rho.shape[3])
    n = nb if n_owned is None else int(n_owned)
    if n <= 0:
        return Record()
    coords = np.asarray(block_coords, dtype=np.int64).reshape(nb, 3)[:n]
    r = np.asarray(rho, dtype=F32).reshape(CELLS, nb, order="F")[:, :n].T                   # [block, cell]
    u = np.asarray(vel, dtype=F32).reshape(CELLS, nb, 3, order="F")[:, :n].transpose(1, 0, 2)
    fluid = ~np.asarray(obstacle).astype(bool).reshape(CELLS, nb, order="F")[:, :n].T
    ux, uy, uz = u[..., 0], u[..., 1], u[..., 2]
    with np.errstate(over="ignore", invalid="ignore"):
        v2 = (ux * ux + uy * uy) + uz * uz
    counted = fluid & np.isfinite(r) & np.isfinite(ux) & np.isfinite(uy) & np.isfinite(uz) & np.isfinite(v2)
    bad = fluid & ~counted
    rec = Record(n_fluid=int(fluid.sum()), n_bad=int(bad.sum()))
    order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0]))                          # blocks by (bx, by, bz)

    def cell_at(flat: int) -> Cell:
        b = order[flat // CELLS]
        return (int(coords[b, 0]), int(coords[b, 1]), int(coords[b, 2]), int(flat % CELLS))

    if counted.any():
        cs = counted[order].reshape(-1)
        for name, a, fill, pick in (("rho_min", r, np.inf, np.argmin), ("rho_max", r, -np.inf, np.argmax), ("v2_max", v2, -np.inf, np.argmax)):
            vals = a[order].reshape(-1)
            at = int(pick(np.where(cs, vals, F32(fill))))           # the first of equal values: the lowest cell in (bx, by, bz, cell)
            setattr(rec, name, F32(vals[at]))
            setattr(rec, "cell_" + name, cell_at(at))
    if rec.n_bad:
        rec.first_bad = cell_at(int(np.argmax(bad[order].reshape(-1))))
    with np.errstate(over="ignore", invalid="ignore"):
        rd = np.where(counted, r.astype(F64), 0.0)
        rec.sum_rho = tree_sum(_block_sums(rd))
        rec.sum_rho_v2 = tree_sum(_block_sums(np.where(counted, r.astype(F64) * v2.astype(F64), 0.0)))
    return rec


def merge(records: Sequence[Optional[Record]]) -> Record:
    """the record of a level from the records of its ranks (None: a rank that holds nothing of it): integers add, the extremes and
    their cells follow the tie rule, the sums add in rank order"""
    out = Record()
    first = True
    for rec in records:
        if rec is None:
            continue
        out.n_fluid += rec.n_fluid
        out.n_bad += rec.n_bad
        for name, better in (("rho_min", lambda a, b: a < b), ("rho_max", lambda a, b: a > b), ("v2_max", lambda a, b: a > b)):
            c, v = getattr(rec, "cell_" + name), getattr(rec, name)
            c0, v0 = getattr(out, "cell_" + name), getattr(out, name)
            if c is not None and (c0 is None or better(v, v0) or (v == v0 and c < c0)):
                setattr(out, name, v)
                setattr(out, "cell_" + name, c)
        if rec.first_bad is not None and (out.first_bad is None or rec.first_bad < out.first_bad):
            out.first_bad = rec.first_bad
        out.sum_rho = rec.sum_rho if first else F64(out.sum_rho + rec.sum_rho)
        out.sum_rho_v2 = rec.sum_rho_v2 if first else F64(out.sum_rho_v2 + rec.sum_rho_v2)
        first = False
    return out


def cell_coordinates(cell: Cell, dx: float, mesh_offset=(0.0, 0.0, 0.0)) -> Tuple[float, float, float]:
    """the cell's centre in the STL's frame (the probes' convention): the centre in the flow file's domain frame,
    ((b - 1) 8 + local + 0.5) dx, minus mesh_offset; Float64"""
    bx, by, bz, c = cell
    local = (c % B, (c // B) % B, c // (B * B))
    return tuple((float((b - 1) * B + l) + 0.5) * float(dx) - float(o) for b, l, o in zip((bx, by, bz), local, mesh_offset))


class FlowDiverged(RuntimeError):
    """a level holds non-finite fluid cells (advanced.flow_monitor.stop_on_divergence)"""

    def __init__(self, step: int, level: int, cell: Cell, coordinates: Tuple[float, float, float], n_bad: int = 0):
        self.step, self.level, self.cell, self.coordinates, self.n_bad = int(step), int(level), cell, coordinates, int(n_bad)
        super().__init__(f"flow diverged at step {step}: level {level} holds {n_bad} non-finite fluid cells, the first in block "
                         f"{tuple(cell[:3])} cell {_local(cell)} at ({coordinates[0]:.6g}, {coordinates[1]:.6g}, {coordinates[2]:.6g})")


def _local(cell: Cell) -> Tuple[int, int, int]:
    c = cell[3]
    return (c % B, (c // B) % B, c // (B * B))


def warnings_of(rec: Record, step: int, level: int, dx: float = 1.0, mesh_offset=(0.0, 0.0, 0.0)) -> List[str]:
    """check_stability's lines (src/diagnostics.jl:99-125) for one level, plus the non-finite count; [] when the level is healthy"""
    out = []
    if rec.cell_v2_max is not None and rec.speed_max > SPEED_WARN:
        out.append("High velocity: %.4f (Ma > 0.5)" % rec.speed_max)
    if rec.cell_rho_min is not None and float(rec.rho_min) < RHO_LOW_WARN:
        out.append("Low density: %.4f" % float(rec.rho_min))
    if rec.cell_rho_max is not None and float(rec.rho_max) > RHO_HIGH_WARN:
        out.append("High density: %.4f" % float(rec.rho_max))
    if rec.n_bad > 0:
        x, y, z = cell_coordinates(rec.first_bad, dx, mesh_offset)
        out.append(f"Non-finite cells: {rec.n_bad}, the first in block {tuple(rec.first_bad[:3])} cell {_local(rec.first_bad)} "
                   f"at ({x:.6g}, {y:.6g}, {z:.6g})")
    if not out:
        return []
    return [f"[WARNING] Step {step} level {level} stability issues:"] + ["  - " + w for w in out]


CSV_HEADER = ",".join(["Step", "StateStep", "Level", "FluidCells", "NonFiniteCells", "RhoMin", "RhoMax", "RhoMean", "SpeedMax", "Mach",
                       "KineticEnergy"] + [f"{name}{axis}" for name in ("RhoMin", "RhoMax", "SpeedMax", "FirstNonFinite") for axis in "XYZ"])


def _num(x) -> str:
    from .output import _shortest
    return _shortest(x)


def csv_row(step: int, state_step: int, level: int, rec: Record, dx: float, mesh_offset=(0.0, 0.0, 0.0)) -> str:
    """one flow_monitor.csv row: float32 extremes and Float64 derived values as their shortest round-trip decimals, the X, Y, Z of a
    cell in the STL's frame, empty where the cell is absent"""
    out = [str(int(step)), str(int(state_step)), str(int(level)), str(rec.n_fluid), str(rec.n_bad), _num(F32(rec.rho_min)),
           _num(F32(rec.rho_max)), _num(F64(rec.rho_mean)), _num(F64(rec.speed_max)), _num(F64(rec.mach)), _num(F64(rec.kinetic_energy))]
    for cell in (rec.cell_rho_min, rec.cell_rho_max, rec.cell_v2_max, rec.first_bad):
        out += ["", "", ""] if cell is None else [_num(F64(v)) for v in cell_coordinates(cell, dx, mesh_offset)]
    return ",".join(out)
