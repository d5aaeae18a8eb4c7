"""Slices: planar grids of points sampled on the device and written as VTK images (no reference counterpart).

Semantics ("Slices"):
  * Points. A plane (preprocess.SlicePlane) has a normal axis n (x, y or z) and two in-plane axes a < b. Point (i, j) lies at
    a0 + i h, b0 + j h, computed in float64 in the STL frame after stl_scale (the frame of advanced.probes.points), with
    floor((a1 - a0) / h) + 1 points per axis; the normal coordinate is `position`. Default bounds: the whole domain; default h: dx
    of the finest level. The point then moves to the domain frame by + params.mesh_offset, exactly as probes.plan_probes does.
    Point index p = i + n_a j, which is VTK's point order of an image with one layer along the normal.
  * Sampling rule: the probes' rule unchanged (probes.py). The level is the finest one whose active blocks hold the base cell
    floor(p / dx - 0.5); weights in float64, then cast to float32; a corner that is no fluid cell of an active block of that level
    is replaced by the base cell; trilinear in float32, x, then y, then z, every lerp (1 - w) a + w b, no contraction. A point at the
    same float64 coordinates gets the same level, corners, weights and values as a probe.
  * Invalid points: a point a probe would refuse (outside the domain, base cell held by no level, base cell an obstacle) gets
    Valid = 0 and 0 in every field. It is not refused.
  * State read: the newest state after the coarse step, as probes and statistics read it (statistics.t_sub_after): vel_temp after
    an even sub-step, vel after an odd one - on levels 2 and finer always `vel`. NOT the flow file's buffer (vel_temp after every
    even coarse step on every level).
  * Fields: Density and Velocity are interpolated; VelocityMagnitude = sqrt((ux^2 + uy^2) + uz^2) of the interpolated components in
    float32; Vorticity and QCriterion are the trilinear interpolation, with the same stencil and weights, of the cell values
    ludwig_level_gradient_fields_compute gives for the same velocity buffer with scale 1/dx of the level: per unit length of the
    file's coordinates, as in the flow file.
  * Sampled coarse steps: start_step + k interval. Files: slice_<name>_%06d.vti (VTK XML ImageData: Origin and Spacing in the domain
    frame, float32 point arrays named as in the flow file plus a UInt8 Valid array) and slice_<name>.pvd (time = step * time_scale),
    rewritten after every file.
The device kernel is k_slice_sample (ludwig_slices_*; vorticity and Q by kernels.hpp vorticity_q, the interpolation by probe_trilinear);
sample_slice below restates it bit for bit.
"""
from __future__ import annotations

import base64
import ctypes as C
import math
import os
import xml.etree.ElementTree as ET
import zlib
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import Handle
from .blocks import BLOCK_SIZE
from .preprocess import SLICE_MAX_POINTS, SlicePlane, slice_axis_points
from . import statistics as stats_mod
from .probes import gather, trilinear

F32 = np.float32
# rows of a sample, in the order the device writes them
ROWS = ("rho", "ux", "uy", "uz", "umag", "wx", "wy", "wz", "q")
ROWS_BASIC, ROWS_GRAD = 5, 9
# config key -> (file array name, rows)
FIELD_ROWS = {"density": ("Density", (0,)), "velocity": ("Velocity", (1, 2, 3)), "velocity_magnitude": ("VelocityMagnitude", (4,)),
              "vorticity": ("Vorticity", (5, 6, 7)), "q_criterion": ("QCriterion", (8,))}
GRAD_FIELDS = ("vorticity", "q_criterion")


@dataclass
class SlicePlan:
    spec: SlicePlane
    axes: Tuple[int, int]           # in-plane axes a < b
    origin: np.ndarray              # [3] float64, point (0, 0) in the domain frame
    spacing: float                  # h
    dims: Tuple[int, int]           # points along a, b
    points: np.ndarray              # [n, 3] float64, STL frame
    domain: np.ndarray              # [n, 3] float64, domain frame
    valid: np.ndarray               # [n] bool
    level: np.ndarray               # [n] int32 (0 where invalid)
    blocks: np.ndarray              # [n, 8] int32, reference block index of every corner (0 where invalid)
    cells: np.ndarray               # [n, 8] int32, x + 8 y + 64 z
    weights: np.ndarray             # [n, 3] float32
    replaced: np.ndarray            # [n, 8] bool

    @property
    def n(self) -> int:
        return self.points.shape[0]

    @property
    def gradient(self) -> bool:
        return any(f in GRAD_FIELDS for f in self.spec.fields)


def _extent(grids) -> np.ndarray:
    l1 = grids[0]
    return np.array([l1.grid_dim_x, l1.grid_dim_y, l1.grid_dim_z], dtype=np.float64) * BLOCK_SIZE * float(l1.dx)


def plane_grid(spec: SlicePlane, grids: Sequence, offset=(0.0, 0.0, 0.0)):
    """(in-plane axes, spacing, dims, points [n, 3] float64 in the STL frame) of a plane; ValueError for a plane wholly outside the
    domain or with more than SLICE_MAX_POINTS points"""
    off = np.asarray(offset, dtype=np.float64).reshape(3)
    lo, hi = -off, _extent(grids) - off                      # the domain in the STL frame
    nrm = int(spec.normal)
    axes = tuple(a for a in range(3) if a != nrm)
    h = float(spec.spacing) if spec.spacing is not None else float(grids[-1].dx)
    bounds = spec.bounds if spec.bounds is not None else tuple((float(lo[a]), float(hi[a])) for a in axes)
    where = f"slice {spec.name!r}"
    if not lo[nrm] <= spec.position <= hi[nrm]:
        raise ValueError(f"{where}: position {spec.position} lies outside the domain [{lo[nrm]}, {hi[nrm]}] along {'xyz'[nrm]}")
    for (b0, b1), a in zip(bounds, axes):
        if b1 < lo[a] or b0 > hi[a]:
            raise ValueError(f"{where}: bounds [{b0}, {b1}] along {'xyz'[a]} miss the domain [{lo[a]}, {hi[a]}]")
    dims = tuple(slice_axis_points(b0, b1, h) for b0, b1 in bounds)
    if dims[0] * dims[1] > SLICE_MAX_POINTS:
        raise ValueError(f"{where}: {dims[0]} x {dims[1]} points, more than {SLICE_MAX_POINTS} per plane")
    ca = bounds[0][0] + np.arange(dims[0], dtype=np.float64) * h
    cb = bounds[1][0] + np.arange(dims[1], dtype=np.float64) * h
    pts = np.empty((dims[0] * dims[1], 3), dtype=np.float64)
    pts[:, axes[0]] = np.tile(ca, dims[1])                   # i fastest
    pts[:, axes[1]] = np.repeat(cb, dims[0])
    pts[:, nrm] = float(spec.position)
    return axes, h, dims, pts


def _lookup(g, i: np.ndarray) -> np.ndarray:
    """[m] reference block index (0-based) of global cells i [m, 3] on level g, -1 where no active block holds it"""
    B = BLOCK_SIZE
    dims = np.array([g.grid_dim_x, g.grid_dim_y, g.grid_dim_z], dtype=np.int64)
    inside = np.all((i >= 0) & (i < dims * B), axis=1)
    out = np.full(i.shape[0], -1, dtype=np.int64)
    j = i[inside] // B
    out[inside] = np.asarray(g.block_pointer)[j[:, 0], j[:, 1], j[:, 2]].astype(np.int64) - 1
    return out


def _fluid(g, blk: np.ndarray, i: np.ndarray) -> np.ndarray:
    """blk >= 0 and the cell is no obstacle"""
    B = BLOCK_SIZE
    ok = blk >= 0
    r = i % B
    out = np.zeros(blk.shape[0], dtype=bool)
    out[ok] = ~np.asarray(g.obstacle)[r[ok, 0], r[ok, 1], r[ok, 2], blk[ok]].astype(bool)
    return out


def plan_points(pts: np.ndarray, grids: Sequence, offset=(0.0, 0.0, 0.0)):
    """probes.plan_probes over numpy arrays, one level at a time: (domain [n, 3], valid, level, blocks, cells, weights, replaced);
    where valid, every array equals plan_probes' at the same coordinates, bit for bit"""
    B = BLOCK_SIZE
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    dom = pts + np.asarray(offset, dtype=np.float64).reshape(1, 3)
    extent = _extent(grids)
    undecided = np.all(np.isfinite(dom), axis=1) & np.all(dom >= 0.0, axis=1) & np.all(dom <= extent, axis=1)
    level = np.zeros(n, np.int32)
    blocks = np.zeros((n, 8), np.int32)
    cells = np.zeros((n, 8), np.int32)
    weights = np.zeros((n, 3), np.float32)
    replaced = np.zeros((n, 8), bool)
    valid = np.zeros(n, bool)
    for li in range(len(grids) - 1, -1, -1):
        idx = np.flatnonzero(undecided)
        if idx.size == 0:
            break
        g = grids[li]
        gg = dom[idx] / float(g.dx) - 0.5
        i0 = np.floor(gg).astype(np.int64)
        b0 = _lookup(g, i0)
        held = b0 >= 0
        idx, gg, i0, b0 = idx[held], gg[held], i0[held], b0[held]
        undecided[idx] = False                                # the finest level holding the base cell, fluid or not
        fluid = _fluid(g, b0, i0)
        idx, gg, i0, b0 = idx[fluid], gg[fluid], i0[fluid], b0[fluid]
        valid[idx] = True
        level[idx] = li
        weights[idx] = (gg - i0).astype(np.float32)
        base_cell = (i0[:, 0] % B) + B * (i0[:, 1] % B) + B * B * (i0[:, 2] % B)
        for c in range(8):
            ic = i0 + np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.int64)
            bc = _lookup(g, ic)
            keep = _fluid(g, bc, ic)
            cc = (ic[:, 0] % B) + B * (ic[:, 1] % B) + B * B * (ic[:, 2] % B)
            blocks[idx, c] = np.where(keep, bc, b0)
            cells[idx, c] = np.where(keep, cc, base_cell)
            replaced[idx, c] = ~keep & (c != 0)
    return dom, valid, level, blocks, cells, weights, replaced


def plan_slice(spec: SlicePlane, grids: Sequence, offset=(0.0, 0.0, 0.0)) -> SlicePlan:
    """the plan of one plane over `grids` (host BlockLevels, level 1 first); offset = params.mesh_offset"""
    axes, h, dims, pts = plane_grid(spec, grids, offset)
    dom, valid, level, blocks, cells, weights, replaced = plan_points(pts, grids, offset)
    origin = np.zeros(3, dtype=np.float64)
    origin[:] = dom[0] if len(dom) else 0.0
    return SlicePlan(spec, axes, origin, h, dims, pts, dom, valid, level, blocks, cells, weights, replaced)


# ---- the numpy restatement of k_slice_sample ----
def sample_slice(plan: SlicePlan, fields: Callable[[int], Tuple], gradient: Optional[bool] = None) -> np.ndarray:
    """[rows, n] float32 (ROWS; 9 rows with the gradient, else 5) of every point, 0 where invalid. fields(level index) ->
    (rho, vel, vorticity, q) of that level in the reference layout - rho [8,8,8,nb], vel and vorticity [8,8,8,nb,3], q [8,8,8,nb] -
    where vorticity and q are the level's gradient fields of the same vel with scale 1/dx (None without the gradient)"""
    grad = plan.gradient if gradient is None else bool(gradient)
    out = np.zeros((ROWS_GRAD if grad else ROWS_BASIC, plan.n), dtype=F32)
    for li in np.unique(plan.level[plan.valid]):
        idx = np.flatnonzero(plan.valid & (plan.level == li))
        rho, vel, vort, q = fields(int(li))
        w = plan.weights[idx][:, None, :]
        u = trilinear(gather(plan, idx, rho, vel), w)                       # [m, 4]: rho, ux, uy, uz
        out[0:4, idx] = u.T
        out[4, idx] = np.sqrt((u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]) + u[:, 3] * u[:, 3])
        if grad:
            g = trilinear(gather(plan, idx, q, vort), w)                    # [m, 4]: q, wx, wy, wz
            out[5:8, idx] = g[:, 1:4].T
            out[8, idx] = g[:, 0]
    return out


def host_sample(stepper, plans: Sequence[SlicePlan], grids: Sequence, t_coarse: int) -> List[np.ndarray]:
    """the samples of `plans` after coarse step t_coarse from a stepper's downloaded fields (a stepper without slices_setup, e.g. the
    CPU oracle): field(level, name), and gradient_fields(level, vel name, scale) when a plane asks for vorticity or Q"""
    from .statistics import t_sub_after
    cache: Dict[int, Tuple] = {}
    grad = any(p.gradient for p in plans)

    def fields(li):
        if li not in cache:
            vel_name = "vel_temp" if t_sub_after(li, t_coarse) % 2 == 0 else "vel"
            rho, vel = stepper.field(li, "rho"), stepper.field(li, vel_name)
            vort = q = None
            if grad:
                vort, q = stepper.gradient_fields(li, vel_name, F32(1.0 / grids[li].dx))
            cache[li] = (rho, vel, vort, q)
        return cache[li]
    return [sample_slice(p, fields) for p in plans]


def check_schedule(start_step: int, interval: int) -> Tuple[int, int]:
    """(start_step, interval) of a stepper's slice set; ValueError below 1"""
    return stats_mod.check_schedule("slices", start_step, interval)


def check_sample_step(t_coarse: int, start_step: int, interval: int) -> None:
    if not stats_mod.is_sample_step(int(t_coarse), start_step, interval):
        raise ValueError(f"slices: coarse step {t_coarse} is no sampled step (start_step {start_step}, interval {interval})")


def stencil_cells(plan: SlicePlan, idx: np.ndarray, grid) -> np.ndarray:
    """global cells (block * 512 + cell) points idx of one level read: their 8 corners and, with the gradient, the 6 face neighbours
    of every corner (a face neighbour across a face where no block lies is the corner itself, the gradient's own-value rule)"""
    B = BLOCK_SIZE
    b = plan.blocks[idx].astype(np.int64).reshape(-1)
    c = plan.cells[idx].astype(np.int64).reshape(-1)
    out = [b * 512 + c]
    if plan.gradient:
        nt = np.asarray(grid.neighbor_table).reshape(grid.n_blocks, 27).astype(np.int64)
        x = np.stack([c % B, (c // B) % B, c // (B * B)], axis=1)
        for a in range(3):
            for s in (-1, 1):
                y = x.copy()
                y[:, a] += s
                o = np.zeros_like(y)
                o[:, a] = np.where(y[:, a] < 0, -1, np.where(y[:, a] >= B, 1, 0))
                nb = np.where(o[:, a] == 0, b + 1, nt[b, (o[:, 0] + 1) + 3 * (o[:, 1] + 1) + 9 * (o[:, 2] + 1)])
                y %= B
                cell = np.where(nb > 0, (nb - 1) * 512 + y[:, 0] + B * y[:, 1] + B * B * y[:, 2], b * 512 + c)
                out.append(cell)
    return np.unique(np.concatenate(out))


def local_plan(plan: SlicePlan, mine: np.ndarray, global_to_local: Sequence[Optional[np.ndarray]]) -> SlicePlan:
    """the plan a rank samples: only the valid points `mine` (bool [n]) stay valid, their blocks in the rank's local ids
    (global_to_local[level][global block] = local block, -1: no copy here)"""
    valid = plan.valid & mine
    blocks = np.zeros_like(plan.blocks)
    for li in np.unique(plan.level[valid]):
        sel = valid & (plan.level == li)
        loc = global_to_local[int(li)][plan.blocks[sel]]
        assert (loc >= 0).all(), "a slice corner in a block this rank holds no copy of"
        blocks[sel] = loc
    return SlicePlan(**{**plan.__dict__, "valid": valid, "blocks": blocks})


# ---- the device slice set (ludwig_slices_*) ----
class DeviceSlices(Handle):
    """one device set over every plane of `plans` on device levels (DeviceLevel, or None for a level no point is on); the plans'
    blocks are the levels' own (reference-order) block indices"""
    _destroy, _closed = "ludwig_slices_destroy", "slice set closed"

    def __init__(self, plans: Sequence[SlicePlan], levels: Sequence, grids: Sequence):
        from . import _lib
        self._lib = _lib.load()
        self.sizes = [p.n for p in plans]
        self.gradient = any(p.gradient for p in plans)
        self.rows = ROWS_GRAD if self.gradient else ROWS_BASIC
        self.n = int(sum(self.sizes))
        arr = (C.c_void_p * len(levels))(*[(lv.handle if lv is not None else None) for lv in levels])
        cat = lambda name, dt: np.ascontiguousarray(np.concatenate([getattr(p, name) for p in plans]), dtype=dt)
        li, bl, ce, w = cat("level", np.int32), cat("blocks", np.int32), cat("cells", np.int32), cat("weights", np.float32)
        va = cat("valid", np.uint8)
        scales = np.ascontiguousarray([F32(1.0 / g.dx) for g in grids], dtype=np.float32)
        h = C.c_void_p()
        _lib.check(self._lib.ludwig_slices_create(arr, len(levels), self.n, li.ctypes.data, bl.ctypes.data, ce.ctypes.data,
                                                  w.ctypes.data, va.ctypes.data, scales.ctypes.data,
                                                  _lib.SLICE_GRADIENT if self.gradient else 0, C.byref(h)))
        self._h = h

    def sample(self, t_coarse: int) -> None:
        """queue a sample of every point after coarse step t_coarse"""
        from . import _lib
        _lib.check(self._lib.ludwig_slices_sample(self.handle, int(t_coarse)))

    def download(self) -> List[np.ndarray]:
        """the last sample, one [rows, n] float32 array per plane"""
        from . import _lib
        out = np.empty((self.rows, self.n), dtype=np.float32)
        _lib.check(self._lib.ludwig_slices_download(self.handle, out.ctypes.data, out.nbytes))
        cuts = np.cumsum([0] + self.sizes)
        return [np.ascontiguousarray(out[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


# ---- files ----
def point_arrays(plan: SlicePlan, values: np.ndarray) -> List[Tuple[str, np.ndarray]]:
    """(file name, [n] or [n, k] array) of the plane's fields, in preprocess.SLICE_FIELDS order, then Valid (UInt8)"""
    out = []
    for f in plan.spec.fields:
        name, rows = FIELD_ROWS[f]
        a = values[list(rows)].T if len(rows) > 1 else values[rows[0]]
        out.append((name, np.ascontiguousarray(a, dtype=F32)))
    out.append(("Valid", plan.valid.astype(np.uint8)))
    return out


def write_vti(path: str, plan: SlicePlan, values: np.ndarray, compress: bool = True) -> str:
    """VTK XML ImageData of one sample: one layer along the normal, Origin / Spacing in the domain frame"""
    from .output import _data_array
    ext = [0, 0, 0, 0, 0, 0]
    for a, d in zip(plan.axes, plan.dims):
        ext[2 * a + 1] = d - 1
    extent = " ".join(str(e) for e in ext)
    origin = " ".join(repr(float(v)) for v in plan.origin)
    h = repr(float(plan.spacing))
    comp_attr = ' compressor="vtkZLibDataCompressor"' if compress else ""
    tmp = path + ".part"
    with open(tmp, "w") as io:
        io.write('<?xml version="1.0" encoding="utf-8"?>\n')
        io.write(f'<VTKFile type="ImageData" version="1.0" byte_order="LittleEndian" header_type="UInt64"{comp_attr}>\n')
        io.write(f'<ImageData WholeExtent="{extent}" Origin="{origin}" Spacing="{h} {h} {h}">\n')
        io.write(f'<Piece Extent="{extent}">\n<PointData>\n')
        for name, a in point_arrays(plan, values):
            io.write(_data_array(name, a, compress, 1 if a.ndim == 1 else a.shape[1]))
        io.write("</PointData>\n<CellData>\n</CellData>\n</Piece>\n</ImageData>\n</VTKFile>\n")
    os.replace(tmp, path)
    return path


def write_pvd(path: str, entries: Sequence[Tuple[float, str]]) -> str:
    """a ParaView collection of (time, file name relative to the .pvd); replaced whole, so a killed run leaves a valid file"""
    tmp = path + ".part"
    with open(tmp, "w") as io:
        io.write('<?xml version="1.0" encoding="utf-8"?>\n<VTKFile type="Collection" version="0.1" byte_order="LittleEndian">\n<Collection>\n')
        for t, f in entries:
            io.write(f'<DataSet timestep="{t!r}" group="" part="0" file="{f}"/>\n')
        io.write("</Collection>\n</VTKFile>\n")
    os.replace(tmp, path)
    return path


def slice_file_name(name: str, step: int) -> str:
    return "slice_%s_%06d.vti" % (name, step)


class SliceWriter:
    """slice_<name>_%06d.vti per sample and slice_<name>.pvd (time = step * time_scale), rewritten after every file"""

    def __init__(self, out_dir: str, plans: Sequence[SlicePlan], time_scale: float):
        self.out_dir, self.plans, self.time_scale = out_dir, list(plans), float(time_scale)
        self.entries: List[List[Tuple[float, str]]] = [[] for _ in self.plans]

    def write(self, step: int, values: Sequence[np.ndarray]) -> None:
        for k, (plan, v) in enumerate(zip(self.plans, values)):
            f = slice_file_name(plan.spec.name, step)
            write_vti(os.path.join(self.out_dir, f), plan, v)
            self.entries[k].append((float(step) * self.time_scale, f))
            write_pvd(os.path.join(self.out_dir, "slice_%s.pvd" % plan.spec.name), self.entries[k])


def _decode(text: str, dtype, compressed: bool) -> np.ndarray:
    text = text.strip()
    if not compressed:
        n = int(np.frombuffer(base64.b64decode(text[:12]), dtype=np.uint64)[0])
        return np.frombuffer(base64.b64decode(text[12:])[:n], dtype=dtype)
    nb = int(np.frombuffer(base64.b64decode(text[:32]), dtype=np.uint64)[0])
    hl = 4 * math.ceil((3 + nb) * 8 / 3)
    head = np.frombuffer(base64.b64decode(text[:hl]), dtype=np.uint64)
    data = base64.b64decode(text[hl:])
    raw, pos = [], 0
    for s in head[3:3 + nb]:
        raw.append(zlib.decompress(data[pos:pos + int(s)]))
        pos += int(s)
    return np.frombuffer(b"".join(raw), dtype=dtype)


_NP_TYPE = {"Float32": np.float32, "Float64": np.float64, "Int32": np.int32, "Int64": np.int64, "UInt8": np.uint8}


def read_vti(path: str) -> Tuple[Dict[str, str], Dict[str, np.ndarray]]:
    """(ImageData attributes, point arrays [n] or [n, k]) of a file write_vti wrote"""
    root = ET.parse(path).getroot()
    compressed = root.get("compressor") is not None
    img = root.find("ImageData")
    arrays = {}
    for da in img.find("Piece").find("PointData").findall("DataArray"):
        a = _decode(da.text or "", _NP_TYPE[da.get("type")], compressed)
        k = int(da.get("NumberOfComponents", "1"))
        arrays[da.get("Name")] = a.reshape(-1, k) if k > 1 else a
    return dict(img.attrib), arrays


def read_pvd(path: str) -> List[Tuple[float, str]]:
    root = ET.parse(path).getroot()
    return [(float(d.get("timestep")), d.get("file")) for d in root.find("Collection").findall("DataSet")]
