"""Streamlines traced on the device (no reference counterpart: the reference writes whole flow files only).

advanced.streamlines in a case YAML lists seed groups {name, points | line}; run_case traces every line every `interval` coarse steps from
`start_step` through the newest state of ALL levels and writes stream_<name>_%06d.vtp (VTK XML PolyData, `Lines` cells, the flow file's
frame) and stream_<name>.pvd. The device side is ludwig_streamlines_* (k_streamlines): the one observer that locates a moving point on
the level hierarchy itself, through every level's dense block_pointer, instead of reading a stencil the host planned. This module holds
the definition as a numpy restatement (sample_host, trace_host: the checker), the seed expansion and the files.

Definition. Everything is float32, every product and sum rounded on its own.
  * A position P is three float32 in cell units of level index 0, domain frame: P = (p_stl + mesh_offset) / dx_1, formed in float64 and
    cast once (seed_positions). On level index li the cell coordinate is g = P 2^li - 0.5f: the scaling is exact, the subtraction the one
    rounding. This is NOT the probes' float64 g, so a vertex and a probe at the same place need not agree bit for bit; and float32
    positions resolve 6e-5 coarse cells at coordinate 1 000.
  * sample(P): for li from the finest level down, the level holds P iff every g_a is finite, 0 <= g_a and floor(g_a) <= 8 grid_dim_a - 1
    (tested in float before any conversion), and block_pointer[floor(g) // 8] > 0. The finest such level is chosen; none: code 1
    (END_OUTSIDE; a periodic neighbour is not followed, a line ends at the grid's extent). Base cell i0 = floor(g); an obstacle cell of
    that level: code 2 (END_OBSTACLE). Weights w = g - floor(g) (exact). Corners i0 + {0,1}^3, c = dx + 2 dy + 4 dz, each through
    block_pointer; a corner outside the grid, in an absent block or in an obstacle cell is replaced by the base cell (the probes'
    rule). rho, ux, uy, uz = probes.trilinear of the corner values.
  * A line (seed P, sign s = +-1; step in cells of the level a step starts on, min_speed, max_steps):
        k = 0
        loop: (rho, u, li) = sample(P)            on failure the line ends with that code; P is no vertex
              vertex k = (P, rho, u, li)
              k == max_steps: end, code 0 (END_STEPS)
              m = sqrt((ux ux + uy uy) + uz uz);  not (m >= min_speed): end, code 3 (END_SLOW; NaN ends here)
              h = step 2^-li
              Pm = P + (0.5f h) ((u / m) s)       per component
              um = sample(Pm) (its code ends the line), mm likewise; not (mm >= min_speed): end, code 3
              P = P + h ((um / mm) s); k += 1
    The midpoint rule with a unit direction: the step length follows the level at the start of the step, the midpoint is located anew
    and may sit on another level. A line has 0 .. max_steps + 1 vertices and one end code.
  * State: every level's newest state after coarse step t_coarse (statistics.t_sub_after: vel_temp after an even sub-step, vel after an
    odd one; rho as a download returns it).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import statistics as stats_mod
from ._lib import Handle
from .blocks import BLOCK_SIZE
from .probes import trilinear

F32 = np.float32
END_STEPS, END_OUTSIDE, END_OBSTACLE, END_SLOW = 0, 1, 2, 3
REC = 8                                           # floats per vertex record: x, y, z, rho, ux, uy, uz, level index
DIRECTIONS = ("forward", "backward", "both")


# ---- the numpy restatement of k_streamlines ----
def host_levels(grids: Sequence, fields: Callable[[int], Tuple[np.ndarray, np.ndarray]]) -> List[tuple]:
    """what sample_host reads of every level, level index 0 first: (block_pointer [gx, gy, gz] 1-based, obstacle [8,8,8,nb] bool,
    rho [8,8,8,nb], vel [8,8,8,nb,3]); fields(level index) -> (rho, the velocity buffer to read)"""
    out = []
    for li, g in enumerate(grids):
        rho, vel = fields(li)
        out.append((np.asarray(g.block_pointer), np.asarray(g.obstacle).astype(bool), np.asarray(rho, dtype=F32), np.asarray(vel, dtype=F32)))
    return out


def stepper_levels(stepper, grids, t_coarse: int) -> List[tuple]:
    """host_levels of a stepper's newest state after coarse step t_coarse, from downloaded fields (stepper.field(level, name))"""
    from .statistics import t_sub_after

    def fields(li):
        vel_name = "vel_temp" if t_sub_after(li, t_coarse) % 2 == 0 else "vel"
        return stepper.field(li, "rho"), stepper.field(li, vel_name)
    return host_levels(grids, fields)


def sample_host(P: np.ndarray, levels: Sequence[tuple]):
    """sample(P) of the definition for P [n, 3] float32 -> (code [n] int32: 0 found, 1 outside, 2 obstacle; values [n, 4] float32 rho,
    ux, uy, uz (NaN where code != 0); level index [n] int32 (-1: none); replaced [n, 8] bool: the corner took the base cell's values)"""
    B = BLOCK_SIZE
    P = np.asarray(P, dtype=F32).reshape(-1, 3)
    n = P.shape[0]
    code = np.full(n, END_OUTSIDE, np.int32)
    vals = np.full((n, 4), np.nan, F32)
    level = np.full(n, -1, np.int32)
    replaced = np.zeros((n, 8), bool)
    todo = np.ones(n, bool)
    for li in range(len(levels) - 1, -1, -1):
        idx = np.flatnonzero(todo)
        if idx.size == 0:
            break
        bp, obstacle, rho, vel = levels[li]
        dims = np.array(bp.shape, dtype=np.int64).reshape(3) if bp.size else np.zeros(3, np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            g = P[idx] * F32(2.0 ** li) - F32(0.5)
            f = np.floor(g)
            ok = (g >= F32(0.0)).all(axis=1) & (f <= (B * dims - 1).astype(F32)).all(axis=1)
        i0 = np.zeros((idx.size, 3), np.int64)
        i0[ok] = f[ok].astype(np.int64)
        b0 = np.zeros(idx.size, np.int64)
        if bp.size:
            b0[ok] = bp[i0[ok, 0] // B, i0[ok, 1] // B, i0[ok, 2] // B]
        hit = ok & (b0 > 0)
        if not hit.any():
            continue
        todo[idx[hit]] = False
        idx, g, f, i0, b0 = idx[hit], g[hit], f[hit], i0[hit], b0[hit] - 1
        level[idx] = li
        solid = obstacle[i0[:, 0] % B, i0[:, 1] % B, i0[:, 2] % B, b0]
        code[idx] = np.where(solid, END_OBSTACLE, 0)
        idx, g, f, i0, b0 = idx[~solid], g[~solid], f[~solid], i0[~solid], b0[~solid]
        if idx.size == 0:
            continue
        w = (g - f).astype(F32)
        v = np.empty((idx.size, 4, 8), F32)
        for c in range(8):
            i = i0 + np.array([c & 1, (c >> 1) & 1, c >> 2], dtype=np.int64)
            inside = (i < B * dims).all(axis=1)
            b = np.zeros(idx.size, np.int64)
            b[inside] = bp[i[inside, 0] // B, i[inside, 1] // B, i[inside, 2] // B]
            valid = inside & (b > 0)
            valid[valid] = ~obstacle[i[valid, 0] % B, i[valid, 1] % B, i[valid, 2] % B, b[valid] - 1]
            ii = np.where(valid[:, None], i, i0)
            bb = np.where(valid, b - 1, b0)
            x, y, z = ii[:, 0] % B, ii[:, 1] % B, ii[:, 2] % B
            v[:, 0, c] = rho[x, y, z, bb]
            for k in range(3):
                v[:, 1 + k, c] = vel[x, y, z, bb, k]
            replaced[idx, c] = ~valid
        with np.errstate(invalid="ignore", over="ignore"):
            vals[idx] = trilinear(v, w[:, None, :])
    return code, vals, level, replaced


def _speed(q: np.ndarray) -> np.ndarray:
    return np.sqrt((q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]).astype(F32)


def trace_host(levels: Sequence[tuple], seeds, sign, step, min_speed, max_steps: int, info: Optional[dict] = None):
    """every line of the definition, vectorised over the lines, one step at a time -> (counts [n] int32, codes [n] int32, records
    [n, max_steps + 1, 8] float32, zero beyond a line's count). info, if a dict, receives what the tests ask of their inputs: 'replaced'
    (stencils with a replaced corner) and 'midpoint_other_level' (steps whose midpoint lay on another level than their start)."""
    P = np.array(seeds, dtype=F32).reshape(-1, 3)
    s = np.asarray(sign, dtype=F32).reshape(-1)
    n, max_steps = P.shape[0], int(max_steps)
    step, min_speed = F32(step), F32(min_speed)
    rec = np.zeros((n, max_steps + 1, REC), F32)
    counts = np.zeros(n, np.int32)
    codes = np.full(n, -1, np.int32)
    alive = np.ones(n, bool)
    n_replaced = n_other = 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(max_steps + 1):
            idx = np.flatnonzero(alive)
            if idx.size == 0:
                break
            code, q, li, rep = sample_host(P[idx], levels)
            n_replaced += int(rep.any(axis=1).sum())
            bad = code != 0
            codes[idx[bad]] = code[bad]
            alive[idx[bad]] = False
            idx, q, li = idx[~bad], q[~bad], li[~bad]
            rec[idx, k, 0:3] = P[idx]
            rec[idx, k, 3:7] = q
            rec[idx, k, 7] = li
            counts[idx] = k + 1
            if k == max_steps:
                codes[idx] = END_STEPS
                break
            m = _speed(q)
            slow = ~(m >= min_speed)
            codes[idx[slow]] = END_SLOW
            alive[idx[slow]] = False
            idx, q, li, m = idx[~slow], q[~slow], li[~slow], m[~slow]
            h = np.ldexp(np.full(idx.size, step, F32), -li.astype(np.int32)).astype(F32)
            hh = F32(0.5) * h
            Pm = P[idx] + hh[:, None] * ((q[:, 1:4] / m[:, None]) * s[idx, None])
            code, qm, lm, rep = sample_host(Pm, levels)
            n_replaced += int(rep.any(axis=1).sum())
            n_other += int(((code == 0) & (lm != li)).sum())
            bad = code != 0
            codes[idx[bad]] = code[bad]
            alive[idx[bad]] = False
            idx, qm, h = idx[~bad], qm[~bad], h[~bad]
            mm = _speed(qm)
            slow = ~(mm >= min_speed)
            codes[idx[slow]] = END_SLOW
            alive[idx[slow]] = False
            idx, qm, h, mm = idx[~slow], qm[~slow], h[~slow], mm[~slow]
            P[idx] = P[idx] + h[:, None] * ((qm[:, 1:4] / mm[:, None]) * s[idx, None])
    if info is not None:
        info["replaced"] = n_replaced
        info["midpoint_other_level"] = n_other
    return counts, codes, rec


def used(counts: np.ndarray, records: np.ndarray) -> np.ndarray:
    """the used records [sum(counts), 8] of every line, line after line"""
    return np.concatenate([records[i, : int(c)] for i, c in enumerate(counts)] + [np.zeros((0, REC), F32)])


def level_changes(counts: np.ndarray, records: np.ndarray) -> np.ndarray:
    """per line, how often consecutive vertices lie on different levels"""
    return np.array([int((np.diff(records[i, : int(c), 7]) != 0).sum()) for i, c in enumerate(counts)], dtype=np.int64)


# ---- the device set (ludwig_streamlines_*) ----
class DeviceStreamlines(Handle):
    """a streamline set over ALL device levels of a hierarchy (DeviceLevel, level index 0 first); seeds [n, 3] float32 positions in
    cell units of level index 0 (seed_positions), sign [n] +-1"""
    _destroy, _closed = "ludwig_streamlines_destroy", "streamline set closed"

    def __init__(self, levels: Sequence, seeds, sign, step, min_speed, max_steps: int):
        from . import _lib
        self._lib = _lib.load()
        sd = np.ascontiguousarray(seeds, dtype=np.float32).reshape(-1, 3)
        sg = np.ascontiguousarray(sign, dtype=np.float32).reshape(-1)
        if sg.size != sd.shape[0]:
            raise ValueError(f"streamlines: {sg.size} signs for {sd.shape[0]} seeds")
        self.n_lines, self.max_steps = int(sd.shape[0]), int(max_steps)
        arr = (C.c_void_p * len(levels))(*[lv.handle for lv in levels])
        h = C.c_void_p()
        _lib.check(self._lib.ludwig_streamlines_create(arr, len(levels), self.n_lines, sd.ctypes.data if self.n_lines else None,
                                                       sg.ctypes.data if self.n_lines else None, float(F32(step)), float(F32(min_speed)),
                                                       self.max_steps, C.byref(h)))
        self._h = h

    def trace(self, t_coarse: int) -> None:
        """queue a trace of every line through the newest state after coarse step t_coarse"""
        from . import _lib
        _lib.check(self._lib.ludwig_streamlines_trace(self.handle, int(t_coarse)))

    def download(self):
        """the last trace: (counts [n] int32, codes [n] int32, records [n, max_steps + 1, 8] float32, zero beyond a line's count)"""
        from . import _lib
        counts, codes = np.zeros(self.n_lines, np.int32), np.zeros(self.n_lines, np.int32)
        rec = np.zeros((self.n_lines, self.max_steps + 1, REC), np.float32)
        none = self.n_lines == 0
        _lib.check(self._lib.ludwig_streamlines_download(self.handle, None if none else counts.ctypes.data, None if none else codes.ctypes.data,
                                                         None if none else rec.ctypes.data, rec.nbytes))
        if not none:                                       # the head of every row came down whole: clear what lies beyond each count
            head = rec[:, : int(counts.max())]
            head[np.arange(head.shape[1])[None, :] >= counts[:, None]] = 0
        return counts, codes, rec


# ---- seeds ----
def expand_group(group: dict, where: str = "seeds") -> np.ndarray:
    """the points [n, 3] float64 (STL frame) of one seed group: {points: [[x, y, z], ...]} or {line: {from, to, count}} - count points
    from + (to - from) i / (count - 1), the one point `from` for count 1. ValueError names `where`."""
    has_p, has_l = group.get("points") is not None, group.get("line") is not None
    if has_p == has_l:
        raise ValueError(f"{where} needs exactly one of points and line")
    if has_p:
        try:
            pts = np.asarray(group["points"], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{where}.points must be a list of [x, y, z]") from None
        if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
            raise ValueError(f"{where}.points must be a non-empty list of [x, y, z]")
    else:
        ln = group["line"]
        if not isinstance(ln, dict) or any(k not in ln for k in ("from", "to", "count")):
            raise ValueError(f"{where}.line must be {{from: [x, y, z], to: [x, y, z], count: n}}")
        try:
            a, b = np.asarray(ln["from"], dtype=np.float64).reshape(3), np.asarray(ln["to"], dtype=np.float64).reshape(3)
        except (TypeError, ValueError):
            raise ValueError(f"{where}.line.from and .to must be [x, y, z]") from None
        count = int(ln["count"])
        if count < 1:
            raise ValueError(f"{where}.line.count must be >= 1, got {count}")
        t = np.arange(count, dtype=np.float64) / max(count - 1, 1)
        pts = a[None, :] + (b - a)[None, :] * t[:, None]
    if not np.isfinite(pts).all():
        raise ValueError(f"{where}: every seed coordinate must be finite")
    return pts


def seed_positions(points, offset, dx1: float) -> np.ndarray:
    """points [n, 3] (STL frame) -> positions [n, 3] float32 in cell units of level index 0: (p + mesh_offset) / dx_1 in float64, cast
    once"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3) + np.asarray(offset, dtype=np.float64).reshape(1, 3)
    return (p / float(dx1)).astype(F32)


def to_domain(P: np.ndarray, dx1: float) -> np.ndarray:
    """positions in cell units of level index 0 -> the frame of the flow file's points: P dx_1 in float64, cast to float32"""
    return (np.asarray(P, dtype=np.float64) * float(dx1)).astype(F32)


def line_signs(direction: str) -> Tuple[float, ...]:
    if direction not in DIRECTIONS:
        raise ValueError(f"streamlines: unknown direction {direction!r} (one of {', '.join(DIRECTIONS)})")
    return {"forward": (1.0,), "backward": (-1.0,), "both": (1.0, -1.0)}[direction]


class SeedPlan:
    """every line of a run: the groups' seeds in order, each seed's lines together (forward before backward)"""

    def __init__(self, groups: Sequence, direction: str, offset, dx1: float):
        """groups: (name, points [n, 3] in the STL frame) pairs"""
        signs = line_signs(direction)
        self.names = [str(nm) for nm, _ in groups]
        self.dx1 = float(dx1)
        seeds, sign, seed_index, group = [], [], [], []
        for gi, (_, pts) in enumerate(groups):
            P = seed_positions(pts, offset, dx1)
            for k in range(P.shape[0]):
                for sg in signs:
                    seeds.append(P[k]); sign.append(sg); seed_index.append(k); group.append(gi)
        self.seeds = np.array(seeds, dtype=F32).reshape(-1, 3)
        self.sign = np.array(sign, dtype=F32)
        self.seed_index = np.array(seed_index, dtype=np.int32)
        self.group = np.array(group, dtype=np.int32)

    @property
    def n_lines(self) -> int:
        return int(self.sign.size)


def check_schedule(start_step: int, interval: int) -> Tuple[int, int]:
    return stats_mod.check_schedule("streamlines", start_step, interval)


# ---- files ----
def stream_file_name(name: str, step: int) -> str:
    return "stream_%s_%06d.vtp" % (name, step)


class Lines:
    """one group's sample as the file holds it: the lines of at least two vertices"""

    def __init__(self, points, offsets, rho, vel, level, seed, direction, end_code, n_short):
        self.points, self.offsets, self.rho, self.vel, self.level = points, offsets, rho, vel, level
        self.seed, self.direction, self.end_code, self.n_short = seed, direction, end_code, n_short


def group_lines(plan: SeedPlan, gi: int, counts, codes, records) -> Lines:
    """the lines of group gi with at least 2 vertices: points in the domain frame, offsets (the end of every line in the point list),
    point arrays rho, vel, level id (level index + 1), cell arrays seed index, direction (+-1), end code; n_short = the lines left out"""
    sel = np.flatnonzero(plan.group == gi)
    keep = sel[counts[sel] >= 2]
    r = np.concatenate([records[i, : int(counts[i])] for i in keep] + [np.zeros((0, REC), F32)])
    return Lines(to_domain(r[:, 0:3], plan.dx1), np.cumsum(counts[keep], dtype=np.int64), r[:, 3].astype(F32), r[:, 4:7].astype(F32),
                 r[:, 7].astype(np.int32) + 1, plan.seed_index[keep].astype(np.int32), plan.sign[keep].astype(np.int32),
                 np.asarray(codes)[keep].astype(np.int32), int(sel.size - keep.size))


class StreamlineWriter:
    """stream_<name>_%06d.vtp per sample and stream_<name>.pvd (time = step * time_scale), rewritten after every file"""

    def __init__(self, out_dir: str, plan: SeedPlan, time_scale: float):
        self.out_dir, self.plan, self.time_scale = out_dir, plan, float(time_scale)
        self.entries: Dict[str, List[Tuple[float, str]]] = {n: [] for n in plan.names}

    def write(self, step: int, counts, codes, records) -> List[Lines]:
        from .output import write_vtp_lines
        from .slices import write_pvd
        out = []
        for gi, name in enumerate(self.plan.names):
            ln = group_lines(self.plan, gi, counts, codes, records)
            f = stream_file_name(name, step)
            write_vtp_lines(os.path.join(self.out_dir, f), ln.points, ln.offsets, ln.rho, ln.vel, ln.level, ln.seed, ln.direction, ln.end_code)
            self.entries[name].append((float(step) * self.time_scale, f))
            write_pvd(os.path.join(self.out_dir, "stream_%s.pvd" % name), self.entries[name])
            out.append(ln)
        return out


def summary(plan: SeedPlan, gi: int, counts, codes) -> str:
    """one log line of a group's sample: lines, vertices, lines left out, lines per end code"""
    sel = plan.group == gi
    c, e = np.asarray(counts)[sel], np.asarray(codes)[sel]
    ends = ", ".join(f"{nm} {int((e == k).sum())}" for k, nm in enumerate(("max_steps", "outside", "obstacle", "slow")))
    return f"{int(sel.sum())} lines, {int(c.sum())} vertices, {int((c < 2).sum())} with fewer than 2 vertices left out; ended by: {ends}"


from .isosurface import read_vtp                   # noqa: E402,F401  (the reader of both kinds of PolyData file)
