"""User-facing outputs of a run (scope row N4): flow VTU, surface VTU, convergence.csv, forces.csv, surface-loads CSV.

Restates src/io_vtk.jl:13-129 (merged multi-level flow mesh), src/forces/io.jl:26-82 (surface VTU), :89-110 (forces.csv),
:166-190 (per-triangle loads CSV) and the convergence.csv lines of src/main.jl:81-82,207-209. What is kept exactly: which
blocks are exported (a block is dropped only when all 8 of its children exist on the next level, io_vtk.jl:27-46), the
order of blocks / points / cells, the voxel connectivity, the velocity buffer choice (`vel_temp` after an even step, `vel`
after an odd one, on EVERY level - io_vtk.jl:56), the NaN/Inf -> 0 scrub, array names and dtypes, and the CSV columns and
printf formats. What is not claimed: byte identity with WriteVTK's files (same VTK XML dialect - inline base64, zlib
blocks, UInt64 headers - but compressor output and attribute order are WriteVTK's own).
"""
from __future__ import annotations

import base64
import os
import zlib
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .blocks import BLOCK_SIZE

VTK_VOXEL, VTK_TRIANGLE = 11, 5
_ZBLOCK = 1 << 15
_PARALLEL_ABOVE = 64 << 20      # bytes of one array above which its zlib blocks are compressed on all cores


# ----------------------------------------------------------------------------------------------------------------
# VTK XML writer (UnstructuredGrid, inline binary, optional zlib)
# ----------------------------------------------------------------------------------------------------------------
_VTK_TYPE = {np.dtype(np.float32): "Float32", np.dtype(np.float64): "Float64", np.dtype(np.int32): "Int32",
             np.dtype(np.int64): "Int64", np.dtype(np.uint8): "UInt8"}


def _encode(a: np.ndarray, compress: bool) -> str:
    raw = np.ascontiguousarray(a).tobytes()
    if not compress:
        return (base64.b64encode(np.uint64(len(raw)).tobytes()) + base64.b64encode(raw)).decode()
    view = memoryview(raw)
    starts = range(0, len(raw), _ZBLOCK) if len(raw) else [0]
    n_blocks = len(starts)
    if len(raw) > _PARALLEL_ABOVE:   # a shipped-size flow mesh is 9 GB of arrays: zlib releases the GIL, the blocks are independent
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=_zlib_threads()) as pool:
            comp = list(pool.map(lambda i: zlib.compress(view[i:i + _ZBLOCK], 6), starts, chunksize=256))
    else:
        comp = [zlib.compress(view[i:i + _ZBLOCK], 6) for i in starts]
    tail = len(raw) - (n_blocks - 1) * _ZBLOCK
    last = tail if tail != _ZBLOCK else 0
    head = np.array([n_blocks, _ZBLOCK, last] + [len(c) for c in comp], dtype=np.uint64)
    return (base64.b64encode(head.tobytes()) + base64.b64encode(b"".join(comp))).decode()


def _zlib_threads() -> int:
    try:
        return max(1, min(32, len(os.sched_getaffinity(0))))
    except AttributeError:
        return max(1, min(32, os.cpu_count() or 1))


def _data_array(name: str, a: np.ndarray, compress: bool, ncomp: int = 1) -> str:
    nc = f' NumberOfComponents="{ncomp}"' if ncomp > 1 or name == "Points" else ""
    return f'<DataArray type="{_VTK_TYPE[a.dtype]}" Name="{name}"{nc} format="binary">{_encode(a, compress)}</DataArray>\n'


def write_vtu(filename: str, points: np.ndarray, connectivity: np.ndarray, offsets: np.ndarray, types: np.ndarray,
              cell_data: Sequence[Tuple[str, np.ndarray]], compress: bool = True,
              field_data: Optional[Sequence[Tuple[str, np.ndarray]]] = None) -> str:
    """points [n,3]; connectivity 0-based; cell_data: (name, [ncells] or [ncells, ncomp]). field_data: (name, 1-D array) of the
    whole dataset (VTK FieldData, e.g. an averaging window); None writes no FieldData element. Returns the path written."""
    path = filename if filename.endswith(".vtu") else filename + ".vtu"
    comp_attr = ' compressor="vtkZLibDataCompressor"' if compress else ""
    with open(path, "w") as io:
        io.write('<?xml version="1.0" encoding="utf-8"?>\n')
        io.write(f'<VTKFile type="UnstructuredGrid" version="1.0" byte_order="LittleEndian" header_type="UInt64"{comp_attr}>\n')
        io.write("<UnstructuredGrid>\n")
        if field_data is not None:
            io.write("<FieldData>\n")
            for name, v in field_data:
                v = np.atleast_1d(v)
                io.write(f'<DataArray type="{_VTK_TYPE[v.dtype]}" Name="{name}" NumberOfTuples="{v.size}" format="binary">{_encode(v, compress)}</DataArray>\n')
            io.write("</FieldData>\n")
        io.write(f'<Piece NumberOfPoints="{points.shape[0]}" NumberOfCells="{types.shape[0]}">\n')
        io.write("<Points>\n" + _data_array("Points", points, compress, 3) + "</Points>\n")
        io.write("<Cells>\n")
        io.write(_data_array("connectivity", np.asarray(connectivity, dtype=np.int64), compress))       # (no copy when already Int64)
        io.write(_data_array("offsets", np.asarray(offsets, dtype=np.int64), compress))
        io.write(_data_array("types", np.asarray(types, dtype=np.uint8), compress))
        io.write("</Cells>\n<CellData>\n")
        for name, a in cell_data:
            io.write(_data_array(name, a, compress, 1 if a.ndim == 1 else a.shape[1]))
        io.write("</CellData>\n</Piece>\n</UnstructuredGrid>\n</VTKFile>\n")
    return path


def write_vtp(filename: str, points: np.ndarray, triangles: np.ndarray, density: np.ndarray, velocity: np.ndarray, level: np.ndarray,
              compress: bool = True) -> str:
    """VTK XML PolyData of an iso-surface (no reference counterpart; isosurface.py): welded points [n, 3] Float32 in the flow file's
    frame, triangles [m, 3] of point indices, point arrays Density, Velocity, VelocityMagnitude = sqrt((ux^2 + uy^2) + uz^2) of the
    interpolated components, cell array Level (Int32). Written whole, then renamed. Returns the path."""
    path = filename if filename.endswith(".vtp") else filename + ".vtp"
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    rho = np.ascontiguousarray(density, dtype=np.float32).reshape(-1)
    vel = np.ascontiguousarray(velocity, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        mag = np.sqrt((vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1]) + vel[:, 2] * vel[:, 2]).astype(np.float32)
    comp_attr = ' compressor="vtkZLibDataCompressor"' if compress else ""
    tmp = path + ".part"
    with open(tmp, "w") as io:
        io.write('<?xml version="1.0" encoding="utf-8"?>\n')
        io.write(f'<VTKFile type="PolyData" version="1.0" byte_order="LittleEndian" header_type="UInt64"{comp_attr}>\n')
        io.write("<PolyData>\n")
        io.write(f'<Piece NumberOfPoints="{pts.shape[0]}" NumberOfVerts="0" NumberOfLines="0" NumberOfStrips="0" '
                 f'NumberOfPolys="{tri.shape[0]}">\n')
        io.write("<Points>\n" + _data_array("Points", pts, compress, 3) + "</Points>\n")
        io.write("<Polys>\n")
        io.write(_data_array("connectivity", tri.reshape(-1), compress))
        io.write(_data_array("offsets", np.arange(1, tri.shape[0] + 1, dtype=np.int64) * 3, compress))
        io.write("</Polys>\n<PointData>\n")
        io.write(_data_array("Density", rho, compress))
        io.write(_data_array("Velocity", vel, compress, 3))
        io.write(_data_array("VelocityMagnitude", mag, compress))
        io.write("</PointData>\n<CellData>\n")
        io.write(_data_array("Level", np.ascontiguousarray(level, dtype=np.int32).reshape(-1), compress))
        io.write("</CellData>\n</Piece>\n</PolyData>\n</VTKFile>\n")
    os.replace(tmp, path)
    return path


def write_vtp_lines(filename: str, points: np.ndarray, offsets: np.ndarray, density: np.ndarray, velocity: np.ndarray, level: np.ndarray,
                    seed: np.ndarray, direction: np.ndarray, end_code: np.ndarray, compress: bool = True) -> str:
    """VTK XML PolyData of streamlines (no reference counterpart; streamlines.py): points [n, 3] Float32 in the flow file's frame, line
    after line; offsets [m] = the end of every line in the point list (each line its points in order); point arrays Density, Velocity,
    Level (Int32); cell arrays Seed, Direction, EndCode (Int32). Written whole, then renamed. Returns the path."""
    path = filename if filename.endswith(".vtp") else filename + ".vtp"
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    comp_attr = ' compressor="vtkZLibDataCompressor"' if compress else ""
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    tmp = path + ".part"
    with open(tmp, "w") as io:
        io.write('<?xml version="1.0" encoding="utf-8"?>\n')
        io.write(f'<VTKFile type="PolyData" version="1.0" byte_order="LittleEndian" header_type="UInt64"{comp_attr}>\n')
        io.write("<PolyData>\n")
        io.write(f'<Piece NumberOfPoints="{pts.shape[0]}" NumberOfVerts="0" NumberOfLines="{off.shape[0]}" NumberOfStrips="0" '
                 'NumberOfPolys="0">\n')
        io.write("<Points>\n" + _data_array("Points", pts, compress, 3) + "</Points>\n")
        io.write("<Lines>\n")
        io.write(_data_array("connectivity", np.arange(pts.shape[0], dtype=np.int64), compress))
        io.write(_data_array("offsets", off, compress))
        io.write("</Lines>\n<PointData>\n")
        io.write(_data_array("Density", np.ascontiguousarray(density, dtype=np.float32).reshape(-1), compress))
        io.write(_data_array("Velocity", np.ascontiguousarray(velocity, dtype=np.float32).reshape(-1, 3), compress, 3))
        io.write(_data_array("Level", i32(level), compress))
        io.write("</PointData>\n<CellData>\n")
        io.write(_data_array("Seed", i32(seed), compress))
        io.write(_data_array("Direction", i32(direction), compress))
        io.write(_data_array("EndCode", i32(end_code), compress))
        io.write("</CellData>\n</Piece>\n</PolyData>\n</VTKFile>\n")
    os.replace(tmp, path)
    return path


def write_vtp_tracers(filename: str, points: np.ndarray, velocity: np.ndarray, level: np.ndarray, particle_id: np.ndarray, seed: np.ndarray,
                      age: np.ndarray, line_connectivity: np.ndarray, line_offsets: np.ndarray, compress: bool = True) -> str:
    """VTK XML PolyData of tracer particles (no reference counterpart; tracers.py): points [n, 3] Float32 in the flow file's frame, one
    `Verts` cell per point; `Lines` cells = streaklines (connectivity of point indices, offsets = the end of every line in it); point
    arrays Velocity, Level, ParticleId, Seed, Age (Int32). Cells carry no arrays. Written whole, then renamed. Returns the path."""
    path = filename if filename.endswith(".vtp") else filename + ".vtp"
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    conn = np.ascontiguousarray(line_connectivity, dtype=np.int64).reshape(-1)
    off = np.ascontiguousarray(line_offsets, dtype=np.int64).reshape(-1)
    comp_attr = ' compressor="vtkZLibDataCompressor"' if compress else ""
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    n = pts.shape[0]
    tmp = path + ".part"
    with open(tmp, "w") as io:
        io.write('<?xml version="1.0" encoding="utf-8"?>\n')
        io.write(f'<VTKFile type="PolyData" version="1.0" byte_order="LittleEndian" header_type="UInt64"{comp_attr}>\n')
        io.write("<PolyData>\n")
        io.write(f'<Piece NumberOfPoints="{n}" NumberOfVerts="{n}" NumberOfLines="{off.shape[0]}" NumberOfStrips="0" NumberOfPolys="0">\n')
        io.write("<Points>\n" + _data_array("Points", pts, compress, 3) + "</Points>\n")
        io.write("<Verts>\n")
        io.write(_data_array("connectivity", np.arange(n, dtype=np.int64), compress))
        io.write(_data_array("offsets", np.arange(1, n + 1, dtype=np.int64), compress))
        io.write("</Verts>\n<Lines>\n")
        io.write(_data_array("connectivity", conn, compress))
        io.write(_data_array("offsets", off, compress))
        io.write("</Lines>\n<PointData>\n")
        io.write(_data_array("Velocity", np.ascontiguousarray(velocity, dtype=np.float32).reshape(-1, 3), compress, 3))
        io.write(_data_array("Level", i32(level), compress))
        io.write(_data_array("ParticleId", i32(particle_id), compress))
        io.write(_data_array("Seed", i32(seed), compress))
        io.write(_data_array("Age", i32(age), compress))
        io.write("</PointData>\n</Piece>\n</PolyData>\n</VTKFile>\n")
    os.replace(tmp, path)
    return path


# ----------------------------------------------------------------------------------------------------------------
# flow export (src/io_vtk.jl)
# ----------------------------------------------------------------------------------------------------------------
def select_export_blocks(block_coords_per_level: Sequence[Sequence[Tuple[int, int, int]]]) -> List[Tuple[int, int]]:
    """(level index 0-based, block index 0-based) in the reference's order (src/io_vtk.jl:17-46): levels ascending, blocks
    in list order; a block is skipped only when all 8 children (2b-1+d) exist on the next level."""
    sets = [set(map(tuple, np.asarray(c, dtype=np.int64).reshape(-1, 3).tolist())) for c in block_coords_per_level]
    out: List[Tuple[int, int]] = []
    for lvl, coords in enumerate(block_coords_per_level):
        nxt = sets[lvl + 1] if lvl + 1 < len(sets) else None
        for b, (bx, by, bz) in enumerate(np.asarray(coords, dtype=np.int64).reshape(-1, 3).tolist()):
            if nxt is not None:
                kids = sum((2 * bx - 1 + dx, 2 * by - 1 + dy, 2 * bz - 1 + dz) in nxt for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
                if kids == 8:
                    continue
            out.append((lvl, b))
    return out


def _scrub(a: np.ndarray) -> np.ndarray:
    """replace!(…, NaN32 => 0, Inf32 => 0, -Inf32 => 0) (src/io_vtk.jl:110-111)"""
    a = a.copy()
    a[~np.isfinite(a)] = 0
    return a


def _cells_of(a: np.ndarray, blocks: np.ndarray) -> np.ndarray:
    """[8,8,8,nb(,K)] -> [len(blocks), 512(, K)] with the cell index x fastest; whole 512-cell chunks when the array is Fortran-ordered"""
    n_cells = BLOCK_SIZE ** 3
    if a.flags.f_contiguous:
        nb = a.shape[3]
        if a.ndim == 4:
            return np.take(a.T.reshape(nb, n_cells), blocks, axis=0)
        return np.take(a.T.reshape(a.shape[4], nb, n_cells), blocks, axis=1).transpose(1, 2, 0)
    sub = a[:, :, :, blocks]
    if a.ndim == 4:
        return sub.reshape(n_cells, len(blocks), order="F").T
    return sub.reshape(n_cells, len(blocks), a.shape[4], order="F").transpose(1, 0, 2)


def _flow_geometry(grids, valid: List[Tuple[int, int]]) -> Dict[str, np.ndarray]:
    """points, voxel connectivity, offsets, types and Level of the exported blocks `valid` (select_export_blocks), plus the
    per-block level / block index arrays (lv_of, blk_of) the cell arrays are gathered by"""
    B = BLOCK_SIZE
    n_total = len(valid)
    n_pts, n_cells = (B + 1) ** 3, B ** 3
    points = np.empty((n_total, n_pts, 3), dtype=np.float32)
    level = np.empty((n_total, n_cells), dtype=np.int32)
    pz, py, px = np.meshgrid(np.arange(B + 1), np.arange(B + 1), np.arange(B + 1), indexing="ij")      # px fastest
    pxyz = np.stack([px.reshape(-1), py.reshape(-1), pz.reshape(-1)], axis=1).astype(np.float32)
    lv_of = np.array([l for l, _ in valid], dtype=np.int64)
    blk_of = np.array([b for _, b in valid], dtype=np.int64)
    for lvl in sorted({l for l, _ in valid}):                        # a level at a time (the valid list is level-major, blocks ascending)
        rows = np.flatnonzero(lv_of == lvl)
        bc = np.asarray(grids[lvl].active_block_coords, dtype=np.int64)[blk_of[rows]]
        off = ((bc - 1) * B).astype(np.float32)
        points[rows] = (off[:, None, :] + pxyz[None, :, :]) * np.float32(grids[lvl].dx)      # (off + p) * dx in Float32, as the reference
        level[rows] = lvl + 1
    z, y, x = np.meshgrid(np.arange(B), np.arange(B), np.arange(B), indexing="ij")
    sy, sz = B + 1, (B + 1) ** 2
    base = (x + y * sy + z * sz).reshape(-1)
    corner = np.array([0, 1, sy, sy + 1, sz, sz + 1, sz + sy, sz + sy + 1])
    conn_block = base[:, None] + corner[None, :]                      # 0-based within the block's points
    conn = (conn_block[None, :, :] + (np.arange(n_total) * n_pts)[:, None, None]).reshape(-1)
    return {
        "points": points.reshape(-1, 3), "connectivity": np.asarray(conn, dtype=np.int64),
        "offsets": np.arange(8, 8 * (n_total * n_cells + 1), 8, dtype=np.int64),
        "types": np.full(n_total * n_cells, VTK_VOXEL, dtype=np.uint8),
        "Level": level.reshape(-1), "lv_of": lv_of, "blk_of": blk_of,
    }


def _gather_cells(geo: Dict[str, np.ndarray], arrays_of_level, dtypes: Sequence, ncomps: Sequence[int]) -> List[np.ndarray]:
    """cell arrays of the exported blocks: arrays_of_level(lvl) -> one [8,8,8,nb(,K)] array per output; [n_exported_cells(, K)] each"""
    n_total, n_cells = geo["lv_of"].size, BLOCK_SIZE ** 3
    outs = [np.empty((n_total, n_cells) + ((k,) if k > 1 else ()), dtype=dt) for dt, k in zip(dtypes, ncomps)]
    for lvl in sorted(set(geo["lv_of"].tolist())):
        rows = np.flatnonzero(geo["lv_of"] == lvl)
        blocks = geo["blk_of"][rows]
        for o, a in zip(outs, arrays_of_level(lvl)):
            o[rows] = _cells_of(a, blocks)                            # cell order x fastest
    return [o.reshape((n_total * n_cells,) + o.shape[2:]) for o in outs]


def build_flow_mesh(t_step: int, grids, fields, derived: Optional[Sequence[Tuple[str, Callable, int]]] = None) -> Dict[str, np.ndarray]:
    """The arrays of export_merged_mesh_sync before they hit the file. `grids`: host levels (active_block_coords, dx);
    `fields(level_index, name)` returns the named array of that level ('rho', 'vel', 'vel_temp', 'obstacle').
    derived: optional extra cell arrays (no reference counterpart), (name, array_of_level, components) with array_of_level(lvl) ->
    Float32 [8,8,8,nb(,K)]; gathered on the same blocks and cell order, NaN / Inf scrubbed, returned under `name`."""
    valid = select_export_blocks([g.active_block_coords for g in grids])
    vel_name = "vel_temp" if t_step % 2 == 0 else "vel"
    geo = _flow_geometry(grids, valid)
    rho, vel, obst = _gather_cells(geo, lambda lvl: (fields(lvl, "rho"), fields(lvl, vel_name), np.asarray(fields(lvl, "obstacle")).astype(bool)),
                                   (np.float32, np.float32, np.uint8), (1, 3, 1))
    vel = _scrub(vel)
    m = {
        "points": geo["points"], "connectivity": geo["connectivity"], "offsets": geo["offsets"], "types": geo["types"],
        "Density": _scrub(rho), "Velocity": vel,
        "VelocityMagnitude": np.sqrt(vel[:, 0] ** 2 + vel[:, 1] ** 2 + vel[:, 2] ** 2),
        "Obstacle": obst, "Level": geo["Level"],
    }
    for name, array_of_level, k in derived or ():
        m[name] = _scrub(_gather_cells(geo, lambda lvl: (array_of_level(lvl),), (np.float32,), (k,))[0])
    return m


DEFAULT_FLOW_FIELDS = ("Density", "Velocity", "VelocityMagnitude", "Obstacle", "Level")


def export_merged_mesh(t_step: int, grids, fields, out_dir: str, output_fields: Sequence[str] = DEFAULT_FLOW_FIELDS,
                       compress: bool = True, derived: Optional[Sequence[Tuple[str, Callable, int]]] = None) -> Optional[str]:
    """export_merged_mesh_sync (src/io_vtk.jl:13-129): writes <out_dir>/flow_%06d.vtu; None when nothing to export.
    derived (build_flow_mesh; e.g. Vorticity, QCriterion): written after the reference's arrays, in the order given. Without it the
    file is the reference's arrays alone."""
    m = build_flow_mesh(t_step, grids, fields, derived)
    if m["types"].size == 0:
        return None
    cd = [(n, m[n]) for n in DEFAULT_FLOW_FIELDS if n in output_fields] + [(n, m[n]) for n, _, _ in derived or ()]
    return write_vtu(os.path.join(out_dir, "flow_%06d" % t_step), m["points"], m["connectivity"], m["offsets"], m["types"], cd, compress)


def export_mean_mesh(t_step: int, grids, stats_of_level, window: Tuple[int, int, int], out_dir: str, compress: bool = True,
                     extra: Optional[Sequence[Tuple[str, Callable]]] = None) -> Optional[str]:
    """<out_dir>/flow_mean_%06d.vtu: the time-averaged flow (no reference counterpart) on the mesh of flow_%06d.vtu - same blocks
    (select_export_blocks), points and cell order. stats_of_level(lvl) -> the finalised statistics of that level
    (statistics.finalize: mean_rho, mean_u, reynolds_stress, tke; Float64 in the reference layout); window = (samples, first
    step, last step), written as Int64 FieldData. Cell arrays Float32 except Obstacle (UInt8) and Level (Int32).
    extra: optional scalar cell arrays, (name, array_of_level) with array_of_level(lvl) -> [8,8,8,nb] (the subgrid measures, subgrid.py),
    written as Float32 after the arrays above in the order given; without it the file is those arrays alone."""
    valid = select_export_blocks([g.active_block_coords for g in grids])
    if not valid:
        return None
    geo = _flow_geometry(grids, valid)

    def arrays(lvl):
        st = stats_of_level(lvl)
        return (st["mean_rho"].astype(np.float32), st["mean_u"].astype(np.float32), st["reynolds_stress"].astype(np.float32),
                st["tke"].astype(np.float32), np.asarray(grids[lvl].obstacle).astype(bool))
    rho, u, rs, k, obst = _gather_cells(geo, arrays, (np.float32,) * 4 + (np.uint8,), (1, 3, 6, 1, 1))
    cd = [("MeanDensity", rho), ("MeanVelocity", u), ("ReynoldsStress", rs), ("TurbulentKineticEnergy", k),
          ("Obstacle", obst), ("Level", geo["Level"])]
    for name, array_of_level in extra or ():
        cd.append((name, _gather_cells(geo, lambda lvl: (np.asarray(array_of_level(lvl)).astype(np.float32),), (np.float32,), (1,))[0]))
    fd = [(name, np.array([v], dtype=np.int64)) for name, v in zip(("StatisticsSamples", "StatisticsFirstStep", "StatisticsLastStep"), window)]
    return write_vtu(os.path.join(out_dir, "flow_mean_%06d" % t_step), geo["points"], geo["connectivity"], geo["offsets"], geo["types"],
                     cd, compress, field_data=fd)


def export_modes_mesh(t_step: int, grids, modes_of_level, window: Tuple[int, int, int, int], frequencies_hz: Sequence[float], out_dir: str,
                      compress: bool = True) -> Optional[str]:
    """<out_dir>/flow_modes_%06d.vtu: the Fourier modes of a finished window (no reference counterpart; modes.py) on the mesh of
    flow_%06d.vtu - same blocks (select_export_blocks), points and cell order. modes_of_level(lvl) -> modes.finalize of that level's
    sums: (mean [8,8,8,nb,4], amplitude [K,8,8,8,nb,4], phase [K,8,8,8,nb,4]) with the components rho, ux, uy, uz. Cell arrays, Float32:
    DensityMean, VelocityMean, then per mode k DensityAmp_<k>, VelocityAmp_<k>, DensityPhase_<k>, VelocityPhase_<k>; then Obstacle (UInt8)
    and Level (Int32). window = (first step, last step, samples, interval), written as Int64 FieldData beside ModesFrequencyHz (Float64)."""
    valid = select_export_blocks([g.active_block_coords for g in grids])
    if not valid:
        return None
    geo = _flow_geometry(grids, valid)
    K = len(frequencies_hz)
    f32 = lambda a: np.asarray(a).astype(np.float32)

    def arrays(lvl):
        mean, amp, phase = modes_of_level(lvl)
        out = [f32(mean[..., 0]), f32(mean[..., 1:4])]
        for k in range(K):
            out += [f32(amp[k][..., 0]), f32(amp[k][..., 1:4]), f32(phase[k][..., 0]), f32(phase[k][..., 1:4])]
        return out + [np.asarray(grids[lvl].obstacle).astype(bool)]
    names = ["DensityMean", "VelocityMean"]
    for k in range(K):
        names += [f"DensityAmp_{k}", f"VelocityAmp_{k}", f"DensityPhase_{k}", f"VelocityPhase_{k}"]
    got = _gather_cells(geo, arrays, (np.float32,) * (2 + 4 * K) + (np.uint8,), (1, 3) * (1 + 2 * K) + (1,))
    cd = list(zip(names, got[:-1])) + [("Obstacle", got[-1]), ("Level", geo["Level"])]
    fd = [(name, np.array([v], dtype=np.int64)) for name, v in zip(("ModesFirstStep", "ModesLastStep", "ModesSamples", "ModesInterval"), window)]
    fd.append(("ModesFrequencyHz", np.asarray(frequencies_hz, dtype=np.float64)))
    return write_vtu(os.path.join(out_dir, "flow_modes_%06d" % t_step), geo["points"], geo["connectivity"], geo["offsets"], geo["types"],
                     cd, compress, field_data=fd)


# ----------------------------------------------------------------------------------------------------------------
# surface export + CSV (src/forces/io.jl)
# ----------------------------------------------------------------------------------------------------------------
def save_surface_vtk(filename: str, mesh, p, sx, sy, sz, extra=None) -> str:
    """save_surface_vtk (src/forces/io.jl:26-82): 3 Float64 points per triangle, 8 cell arrays, uncompressed. extra: (name, float32
    [n_tri]) cell arrays written after those (the wall diagnostics); without them the file is the reference's."""
    n = mesh.triangles.shape[0]
    p, sx, sy, sz = (np.asarray(a, dtype=np.float32) for a in (p, sx, sy, sz))
    pts = np.asarray(mesh.triangles, dtype=np.float64).reshape(n * 3, 3)
    quality = ((np.abs(p) > 1e-10) | (np.abs(sx) > 1e-10)).astype(np.float32)
    cd = [("Pressure_Pa", p), ("ShearX_Pa", sx), ("ShearY_Pa", sy), ("ShearZ_Pa", sz),
          ("ShearMagnitude_Pa", np.sqrt(sx ** 2 + sy ** 2 + sz ** 2)),
          ("Normal", np.asarray(mesh.normals, dtype=np.float32)), ("Area_m2", np.asarray(mesh.areas, dtype=np.float32)),
          ("MappingQuality", quality)]
    cd += [(name, np.ascontiguousarray(a, dtype=np.float32)) for name, a in (extra or ())]
    return write_vtu(filename, pts, np.arange(3 * n, dtype=np.int64), np.arange(1, n + 1, dtype=np.int64) * 3,
                     np.full(n, VTK_TRIANGLE, dtype=np.uint8), cd, compress=False)


FORCE_CSV_HEADER = "Step,Time_s,U_inlet,Fx_N,Fy_N,Fz_N,Fx_p_N,Fx_v_N,Mx_Nm,My_Nm,Mz_Nm,Cd,Cl,Cs,Cmy"
CONVERGENCE_CSV_HEADER = "Step,Walltime,Time_phys_s,U_inlet_lat,Rho_min,MLUPS,Cd,Cl"


def write_force_csv_header(path: str) -> None:
    with open(path, "w") as io:
        io.write(FORCE_CSV_HEADER + "\n")


def force_csv_row(step: int, time_phys: float, fr, u_inlet) -> str:
    """append_force_csv's printf (src/forces/io.jl:99-110)"""
    return ("%d,%.6e,%.6f,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6f,%.6f,%.6f,%.6f" %
            (step, time_phys, float(u_inlet), fr.Fx, fr.Fy, fr.Fz, fr.Fx_pressure, fr.Fx_viscous, fr.Mx, fr.My, fr.Mz, fr.Cd, fr.Cl, fr.Cs, fr.Cmy))


def append_force_csv(path: str, step: int, time_phys: float, fr, u_inlet) -> None:
    with open(path, "a") as io:
        io.write(force_csv_row(step, time_phys, fr, u_inlet) + "\n")


def walltime_str(elapsed: float) -> str:
    """src/main.jl:37-40"""
    return "%02d:%02d:%05.2f" % (int(elapsed // 3600), int((elapsed % 3600) // 60), elapsed % 60)


def _shortest(x) -> str:
    """shortest round-trip decimal of a Float32/Float64 (what Julia's string interpolation prints, up to its choice of
    exponent notation for very small / large magnitudes)"""
    return np.format_float_positional(x, unique=True, trim="0") if 1e-5 <= abs(float(x)) < 1e6 or float(x) == 0.0 \
        else np.format_float_scientific(x, unique=True, trim="0", exp_digits=1).replace("e+", "e")


def convergence_csv_row(step: int, elapsed: float, time_phys: float, u_curr, rho_min, mlups: float, cd: Optional[float], cl: Optional[float]) -> str:
    """src/main.jl:207-209: "$diag_step,$(walltime_str()),$time_phys,$u_curr,$(stats.rho_min),$mlups,$cd_str,$cl_str" """
    cd_s = "N/A" if cd is None else "%.4f" % cd
    cl_s = "N/A" if cl is None else "%.4f" % cl
    return ",".join([str(step), walltime_str(elapsed), _shortest(np.float64(time_phys)), _shortest(np.float32(u_curr)),
                     _shortest(np.float32(rho_min)), _shortest(np.float64(mlups)), cd_s, cl_s])


def export_surface_loads_csv(filename: str, mesh, mesh_offset, p, sx, sy, sz) -> None:
    """export_surface_loads_csv (src/forces/io.jl:166-190)"""
    c = np.asarray(mesh.centers, dtype=np.float64) + np.asarray(mesh_offset, dtype=np.float64)[None, :]
    nrm, area = np.asarray(mesh.normals, dtype=np.float64), np.asarray(mesh.areas, dtype=np.float64)
    with open(filename, "w") as io:
        io.write("triangle_id,cx,cy,cz,nx,ny,nz,area_m2,pressure_Pa,shear_x_Pa,shear_y_Pa,shear_z_Pa\n")
        for i in range(c.shape[0]):
            io.write("%d,%.6e,%.6e,%.6e,%.6f,%.6f,%.6f,%.6e,%.6e,%.6e,%.6e,%.6e\n" %
                     (i + 1, c[i, 0], c[i, 1], c[i, 2], nrm[i, 0], nrm[i, 1], nrm[i, 2], area[i], p[i], sx[i], sy[i], sz[i]))


def force_summary(fr, rho_ref: float, u_ref: float, area_ref: float, chord_ref: float) -> str:
    """print_force_summary (src/forces/io.jl:117-160) as a string"""
    q = 0.5 * rho_ref * u_ref ** 2
    lines = ["", "=" * 60, "         AERODYNAMIC FORCES SUMMARY", "=" * 60, "", "Reference Values:",
             "  ρ_ref  = %.4f kg/m³" % rho_ref, "  U_ref  = %.4f m/s" % u_ref, "  A_ref  = %.4f m²" % area_ref,
             "  L_ref  = %.4f m" % chord_ref, "  q_∞    = %.4f Pa" % q, "", "Forces [N]:",
             "  Fx (drag)  = %+.4e  (pressure: %+.4e, viscous: %+.4e)" % (fr.Fx, fr.Fx_pressure, fr.Fx_viscous),
             "  Fy (side)  = %+.4e  (pressure: %+.4e, viscous: %+.4e)" % (fr.Fy, fr.Fy_pressure, fr.Fy_viscous),
             "  Fz (lift)  = %+.4e  (pressure: %+.4e, viscous: %+.4e)" % (fr.Fz, fr.Fz_pressure, fr.Fz_viscous),
             "", "Moments [N·m]:", "  Mx (roll)  = %+.4e" % fr.Mx, "  My (pitch) = %+.4e" % fr.My, "  Mz (yaw)   = %+.4e" % fr.Mz,
             "", "Coefficients:", "  Cd = %+.6f" % fr.Cd, "  Cl = %+.6f" % fr.Cl, "  Cs = %+.6f" % fr.Cs, "  Cmy = %+.6f" % fr.Cmy]
    if abs(fr.Fx) > 1e-10:
        lines += ["", "Drag breakdown: %.1f%% pressure, %.1f%% viscous" % (abs(fr.Fx_pressure) / abs(fr.Fx) * 100, abs(fr.Fx_viscous) / abs(fr.Fx) * 100)]
    lines += ["=" * 60, ""]
    return "\n".join(lines)
