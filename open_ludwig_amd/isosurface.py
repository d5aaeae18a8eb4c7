"""Iso-surfaces extracted on the device (no reference counterpart: the reference writes whole flow files only).

advanced.isosurfaces in a case YAML lists surfaces {name, field, value, bounds?}; run_case extracts them every `interval` coarse steps from
`start_step` on every level that exports blocks and writes iso_<name>_%06d.vtp (VTK XML PolyData in the flow file's frame) and
iso_<name>.pvd. The device side is ludwig_level_isosurface_extract / _download (k_iso_count, k_iso_emit); this module holds the
definition as a numpy restatement (extract_host, the checker), the welding of the triangle soup into an indexed mesh, and the files.

Definition (one level). Surfaces live on the dual grid: a cube is anchored at a cell (block b; x, y, z) and its corner c = dx + 2 dy + 4 dz
is the cell (x + dx, y + dy, z + dz), reached through the anchor block's neighbour row when it lies beyond the block (three faces, three
edges, one corner; a periodic entry continues the surface unwrapped). A cube is live iff its anchor block is owned and not skipped, its
anchor's global cell coordinates lie in [cell_lo, cell_hi), all eight corner blocks exist, no corner is an obstacle cell and all eight
scalars are finite. It is split into the six tetrahedra KUHN_TETS around the diagonal 0-7 (every cube face is cut along the same diagonal
from both sides: watertight without a 256-case table). A corner is inside iff s >= value; a tetrahedron with 1 or 3 inside corners gives
one triangle, with 2 a quad = two triangles, wound by the integer table CASE_TRIANGLES so that the normal points from the inside corners
to the outside ones. A vertex sits on a tetrahedron edge (a, b), a < b as corner numbers - one operand order for every cube sharing the
edge, so the same bits from each: t = clamp((value - s_a) / (s_b - s_a), 0, 1) (NaN -> 0), position g_a + t d in cell units of the level
(g_a the anchor-relative global cell coordinate of corner a, d = b - a in {0, 1}^3), attributes rho, ux, uy, uz = q_a + t (q_b - q_a), key
= (512 block + cell) of a and of b (reference block order). Float32 throughout. Triangles come by anchor block (reference order), anchor
cell x + 8 y + 64 z, tetrahedron, first / second triangle.
"""
from __future__ import annotations

import os
import xml.etree.ElementTree as ET
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import statistics as stats_mod
from .blocks import BLOCK_SIZE

F32 = np.float32
FIELDS = ("density", "velocity_magnitude", "q_criterion", "vorticity_magnitude")      # enum LudwigIsoScalar, in this order
GRADIENT_FIELDS = ("q_criterion", "vorticity_magnitude")
CELL_MAX = 2 ** 31 - 1

# the six tetrahedra of a cube, all around the diagonal from corner 0 to corner 7 (Kuhn's split), all of positive orientation
KUHN_TETS = np.array([(0, 1, 3, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 6, 4, 7), (0, 4, 5, 7), (0, 5, 1, 7)], dtype=np.int64)
# the six edges of a tetrahedron as pairs of its corners 0..3
TET_EDGES = np.array([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)], dtype=np.int64)
# case = sum of 2^k over the inside corners k of a positively oriented tetrahedron -> up to two triangles of three tetrahedron edges
# (-1: none), normal from the inside corners to the outside ones; case 15 - m is case m reversed
CASE_TRIANGLES = np.array([
    [[-1, -1, -1], [-1, -1, -1]], [[0, 1, 2], [-1, -1, -1]], [[0, 4, 3], [-1, -1, -1]], [[1, 2, 4], [1, 4, 3]],
    [[1, 3, 5], [-1, -1, -1]], [[0, 3, 5], [0, 5, 2]], [[0, 4, 5], [0, 5, 1]], [[2, 4, 5], [-1, -1, -1]],
    [[2, 5, 4], [-1, -1, -1]], [[0, 1, 5], [0, 5, 4]], [[0, 2, 5], [0, 5, 3]], [[1, 5, 3], [-1, -1, -1]],
    [[1, 3, 4], [1, 4, 2]], [[0, 3, 4], [-1, -1, -1]], [[0, 2, 1], [-1, -1, -1]], [[-1, -1, -1], [-1, -1, -1]]], dtype=np.int64)


def _cells(a: np.ndarray) -> np.ndarray:
    """[8,8,8,nb(,K)] -> [nb, 512(, K)], cell index x fastest"""
    a = np.asarray(a)
    nb = a.shape[3]
    if a.ndim == 4:
        return a.reshape(512, nb, order="F").T
    return a.reshape(512, nb, a.shape[4], order="F").transpose(1, 0, 2)


def extract_host(s, obstacle, neighbor_table, skip, cell_lo, cell_hi, value, rho, vel, block_coords, n_owned: Optional[int] = None):
    """the triangles of the surface s = value on one level: positions [n, 3, 3] (cell units of the level), attributes [n, 3, 4] (rho,
    ux, uy, uz), both Float32, and keys [n, 3, 2] Int32, in the device's order. s, rho [8,8,8,nb], vel [8,8,8,nb,3], obstacle
    [8,8,8,nb] bool; neighbor_table [nb, 27] 1-based, 0 = none; skip [nb] (non-zero: no cube anchored in the block) or None;
    block_coords [nb, 3] 1-based; n_owned: blocks [0, n_owned) anchor cubes (None: all)."""
    B = BLOCK_SIZE
    S, OB, RHO, VEL = _cells(np.asarray(s, dtype=F32)), _cells(np.asarray(obstacle)).astype(bool), _cells(np.asarray(rho, dtype=F32)), \
        _cells(np.asarray(vel, dtype=F32))
    nb = S.shape[0]
    nt = np.asarray(neighbor_table).reshape(nb, 27).astype(np.int64)
    bc = np.asarray(block_coords, dtype=np.int64).reshape(nb, 3)
    value = F32(value)
    lo, hi = np.asarray(cell_lo, dtype=np.int64), np.asarray(cell_hi, dtype=np.int64)
    empty = (np.zeros((0, 3, 3), F32), np.zeros((0, 3, 4), F32), np.zeros((0, 3, 2), np.int32))
    if nb == 0:
        return empty
    cell = np.arange(512, dtype=np.int64)
    xyz = np.stack([cell % B, (cell // B) % B, cell // (B * B)], axis=1)                    # [512, 3]
    blk = np.arange(nb, dtype=np.int64)
    live = np.ones((nb, 512), bool)
    live[(n_owned if n_owned is not None else nb):] = False
    if skip is not None:
        live[np.asarray(skip).reshape(nb) != 0] = False
    g0 = (bc[:, None, :] - 1) * B + xyz[None, :, :]                                         # [nb, 512, 3] anchor's global cell
    live &= ((g0 >= lo) & (g0 < hi)).all(axis=2)
    cblk = np.empty((nb, 512, 8), np.int64)
    ccell = np.empty((nb, 512, 8), np.int64)
    for c in range(8):
        p = xyz + np.array([c & 1, (c >> 1) & 1, c >> 2])
        o = p >> 3
        d = 13 + o[:, 0] + 3 * o[:, 1] + 9 * o[:, 2]
        cb = np.where(d[None, :] == 13, blk[:, None], nt[:, d] - 1)
        cblk[:, :, c] = cb
        ccell[:, :, c] = ((p[:, 0] & 7) + 8 * (p[:, 1] & 7) + 64 * (p[:, 2] & 7))[None, :]
    live &= (cblk >= 0).all(axis=2)
    idx_b, idx_c = np.nonzero(live)                                                         # block-major, cell ascending
    cb, cc = cblk[idx_b, idx_c], ccell[idx_b, idx_c]                                        # [m, 8]
    v = S[cb, cc]
    ok = np.isfinite(v).all(axis=1) & ~OB[cb, cc].any(axis=1)
    idx_b, idx_c, cb, cc, v = idx_b[ok], idx_c[ok], cb[ok], cc[ok], v[ok]
    inside = v >= value                                                                     # [m, 8]
    case = np.zeros((len(v), 6), np.int64)
    for k in range(4):
        case += inside[:, KUHN_TETS[:, k]].astype(np.int64) << k
    tris = CASE_TRIANGLES[case]                                                             # [m, 6, 2, 3] edge ids
    cube, tet, which = np.nonzero(tris[..., 0] >= 0)                                        # cube, tetrahedron, triangle: the order
    if cube.size == 0:
        return empty
    e = tris[cube, tet, which]                                                              # [n, 3]
    ca = KUHN_TETS[tet[:, None], TET_EDGES[e, 0]]                                           # [n, 3] cube corners
    cbn = KUHN_TETS[tet[:, None], TET_EDGES[e, 1]]
    a, b = np.minimum(ca, cbn), np.maximum(ca, cbn)
    cu = cube[:, None]
    sa, sb = v[cu, a], v[cu, b]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (value - sa) / (sb - sa)
    t = np.fmin(np.fmax(t, F32(0)), F32(1)).astype(F32)
    off = lambda c: np.stack([c & 1, (c >> 1) & 1, c >> 2], axis=-1)                         # [n, 3, 3]
    ga = (g0[idx_b, idx_c][cu] + off(a)).astype(F32)
    d = (off(b) - off(a)).astype(F32)
    pos = (ga + t[..., None] * d).astype(F32)
    ba, bb, xa, xb = cb[cu, a], cb[cu, b], cc[cu, a], cc[cu, b]
    qa = np.concatenate([RHO[ba, xa][..., None], VEL[ba, xa]], axis=-1)                      # [n, 3, 4]
    qb = np.concatenate([RHO[bb, xb][..., None], VEL[bb, xb]], axis=-1)
    with np.errstate(invalid="ignore", over="ignore"):
        att = (qa + t[..., None] * (qb - qa)).astype(F32)
    keys = np.stack([512 * ba + xa, 512 * bb + xb], axis=-1).astype(np.int32)
    return pos, att, keys


def weld(keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """keys [n, 3, 2] -> (first [n_points]: the index into the flattened [3 n] vertices of each unique vertex's first occurrence,
    triangles [n, 3]: indices into those unique vertices). Vertices are unique by their key pair, in ascending key order."""
    k = np.asarray(keys).reshape(-1, 2).astype(np.int64)
    if k.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros((0, 3), np.int64)
    packed = (k[:, 0] << 32) | k[:, 1]
    _, first, inv = np.unique(packed, return_index=True, return_inverse=True)
    return first.astype(np.int64), inv.reshape(-1, 3).astype(np.int64)


def to_domain(pos: np.ndarray, dx: float) -> np.ndarray:
    """cell units of a level -> the frame of the flow file's points: (pos + 0.5) dx in Float64, cast to Float32"""
    return ((np.asarray(pos, dtype=np.float64) + 0.5) * float(dx)).astype(F32)


def cell_box(bounds, dx: float, offset=(0.0, 0.0, 0.0)) -> Tuple[np.ndarray, np.ndarray]:
    """(cell_lo, cell_hi) Int32 [3] of one level for a surface's `bounds` ([[x0, x1], [y0, y1], [z0, z1]] in the STL frame, moved by
    + offset into the domain frame; None: everything): the anchors whose cell centre (i + 0.5) dx lies in [lower, upper)"""
    if bounds is None:
        return np.zeros(3, np.int32), np.full(3, CELL_MAX, np.int32)
    b = np.asarray(bounds, dtype=np.float64) + np.asarray(offset, dtype=np.float64)[:, None]
    edge = np.ceil(b / float(dx) - 0.5)
    edge = np.clip(edge, 0, CELL_MAX)
    return edge[:, 0].astype(np.int32), edge[:, 1].astype(np.int32)


def skip_flags(grids) -> List[np.ndarray]:
    """per level, UInt8 [n_blocks]: 1 for the blocks output.select_export_blocks drops (all 8 children exist on the next level)"""
    from .output import select_export_blocks
    out = [np.ones(g.n_blocks, np.uint8) for g in grids]
    for lvl, b in select_export_blocks([g.active_block_coords for g in grids]):
        out[lvl][b] = 0
    return out


def check_field(field: str) -> int:
    if field not in FIELDS:
        raise ValueError(f"isosurface: unknown field {field!r} (one of {', '.join(FIELDS)})")
    return FIELDS.index(field)


def scalar_host(field: str, rho, vel, vort, q) -> np.ndarray:
    """the scalar of `field` from downloaded arrays, with the device's expressions"""
    check_field(field)
    if field == "density":
        return np.asarray(rho, dtype=F32)
    if field == "q_criterion":
        return np.asarray(q, dtype=F32)
    w = np.asarray(vel if field == "velocity_magnitude" else vort, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]).astype(F32)


class Surface:
    """one merged sample of a surface: welded points in the domain frame, triangles, point attributes and the level of every triangle"""

    def __init__(self, points, triangles, rho, vel, level):
        self.points, self.triangles, self.rho, self.vel, self.level = points, triangles, rho, vel, level


def merge_levels(parts: Sequence[Tuple[int, float, np.ndarray, np.ndarray, np.ndarray]]) -> Surface:
    """parts: per level in ascending order (level index 0-based, dx, positions, attributes, keys) of one extraction -> the welded
    Surface; vertices are welded within a level only (a key names cells of its own level)"""
    pts, tri, rho, vel, lev, base = [], [], [], [], [], 0
    for li, dx, pos, att, keys in parts:
        first, t = weld(keys)
        p = to_domain(np.asarray(pos).reshape(-1, 3)[first], dx)
        a = np.asarray(att, dtype=F32).reshape(-1, 4)[first]
        pts.append(p); rho.append(a[:, 0]); vel.append(a[:, 1:4]); tri.append(t + base)
        lev.append(np.full(t.shape[0], li + 1, np.int32))
        base += p.shape[0]
    cat = lambda xs, shape, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt)
    return Surface(cat(pts, (0, 3), F32), cat(tri, (0, 3), np.int64), cat(rho, (0,), F32), cat(vel, (0, 3), F32), cat(lev, (0,), np.int32))


def host_extract_levels(stepper, grids, field: str, value, t_coarse: int, boxes, skips, n_owned=None):
    """the parts merge_levels takes, from a stepper's downloaded fields through extract_host (the checker; a stepper without
    `isosurface`, e.g. the CPU oracle): field(level, name), and gradient_fields(level, vel name, scale) for Q / vorticity"""
    from .statistics import t_sub_after
    parts = []
    for li, g in enumerate(grids):
        if skips[li].all():
            continue
        vel_name = "vel_temp" if t_sub_after(li, t_coarse) % 2 == 0 else "vel"
        rho, vel = stepper.field(li, "rho"), stepper.field(li, vel_name)
        vort = q = None
        if field in GRADIENT_FIELDS:
            vort, q = stepper.gradient_fields(li, vel_name, F32(1.0 / g.dx))
        s = scalar_host(field, rho, vel, vort, q)
        pos, att, keys = extract_host(s, g.obstacle, g.neighbor_table, skips[li], boxes[li][0], boxes[li][1], value, rho, vel,
                                      np.asarray(g.active_block_coords).reshape(-1, 3), n_owned)
        parts.append((li, g.dx, pos, att, keys))
    return parts


def check_schedule(start_step: int, interval: int) -> Tuple[int, int]:
    return stats_mod.check_schedule("isosurfaces", start_step, interval)


# ---- files ----
def iso_file_name(name: str, step: int) -> str:
    return "iso_%s_%06d.vtp" % (name, step)


class IsoWriter:
    """iso_<name>_%06d.vtp per sample and iso_<name>.pvd (time = step * time_scale), rewritten after every file"""

    def __init__(self, out_dir: str, names: Sequence[str], time_scale: float):
        self.out_dir, self.names, self.time_scale = out_dir, list(names), float(time_scale)
        self.entries: Dict[str, List[Tuple[float, str]]] = {n: [] for n in self.names}

    def write(self, step: int, name: str, surface: Surface) -> str:
        from .output import write_vtp
        from .slices import write_pvd
        f = iso_file_name(name, step)
        path = write_vtp(os.path.join(self.out_dir, f), surface.points, surface.triangles, surface.rho, surface.vel, surface.level)
        self.entries[name].append((float(step) * self.time_scale, f))
        write_pvd(os.path.join(self.out_dir, "iso_%s.pvd" % name), self.entries[name])
        return path


def read_vtp(path: str) -> Dict[str, np.ndarray]:
    """the arrays of a file output.write_vtp, write_vtp_lines or write_vtp_tracers wrote: Points [n, 3], connectivity, offsets (of the
    Polys or the Lines, whichever the file holds), the point arrays and the cell arrays by name; a file with a Verts section (the
    tracers') also gives verts_connectivity, verts_offsets and NumberOfVerts"""
    from .slices import _NP_TYPE, _decode
    root = ET.parse(path).getroot()
    compressed = root.get("compressor") is not None
    piece = root.find("PolyData").find("Piece")
    out: Dict[str, np.ndarray] = {}
    for tag in ("Points", "Polys", "Lines", "PointData", "CellData"):
        section = piece.find(tag)
        for da in (section.findall("DataArray") if section is not None else ()):
            a = _decode(da.text or "", _NP_TYPE[da.get("type")], compressed)
            k = int(da.get("NumberOfComponents", "1"))
            out[da.get("Name")] = a.reshape(-1, k) if k > 1 else a
    verts = piece.find("Verts")
    if verts is not None:
        for da in verts.findall("DataArray"):
            out["verts_" + da.get("Name")] = _decode(da.text or "", _NP_TYPE[da.get("type")], compressed)
        out["NumberOfVerts"] = np.int64(piece.get("NumberOfVerts"))
    out["NumberOfPoints"] = np.int64(piece.get("NumberOfPoints"))
    out["NumberOfPolys"] = np.int64(piece.get("NumberOfPolys"))
    out["NumberOfLines"] = np.int64(piece.get("NumberOfLines"))
    return out
