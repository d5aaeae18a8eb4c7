"""Small levels and meshes, made in code, for the set-up restatement (tests/_setup_ref.py); shared by the host and the device test.

Geometry is given in CELL UNITS of the level (cell n has its centre at n - 0.5, its faces at n - 1 and n) and turned into Float32
vertices (as an STL file holds them) and a Float64 mesh offset: vertex = Float32(position * dx - offset). Every level has at most 64
blocks, every mesh at most about 400 triangles. `planted` cases put geometry exactly on a threshold; their expectations under
`by_hand` are typed-in literals, never computed here. Direction index k: k = (cx + 1) + 3 (cy + 1) + 9 (cz + 1).
"""
import math
import struct
from types import SimpleNamespace

import numpy as np

F16 = np.float16
K = lambda cx, cy, cz: (cx + 1) + 3 * (cy + 1) + 9 * (cz + 1)


def full(nx, ny, nz, lo=(1, 1, 1)):
    return [(lo[0] + x, lo[1] + y, lo[2] + z) for z in range(nz) for y in range(ny) for x in range(nx)]


# ----------------------------------------------------------------------------------------------------------------
# meshes in cell units
# ----------------------------------------------------------------------------------------------------------------
def quad(a, b, c, d):
    """two triangles a b c, a c d sharing the diagonal a - c"""
    return [[a, b, c], [a, c, d]]


def box_mesh(lo, hi):
    """12 triangles, the z-low face first, then z-high, y-low, y-high, x-low, x-high; outward winding"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    t = []
    t += quad((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0))
    t += quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1))
    t += quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1))
    t += quad((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0))
    t += quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0))
    t += quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1))
    return np.asarray(t, dtype=np.float64)


def rotate_y(tris, angle, about):
    c, s = math.cos(angle), math.sin(angle)
    p = np.asarray(tris, dtype=np.float64) - np.asarray(about)
    out = np.stack([c * p[..., 0] + s * p[..., 2], p[..., 1], -s * p[..., 0] + c * p[..., 2]], axis=-1)
    return out + np.asarray(about)


def icosphere(centre, radius, subdivisions):
    """20 * 4^subdivisions triangles (80 for 1, 320 for 2), slightly turned so that no vertex sits on a lattice line"""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.asarray(p, dtype=np.float64) / math.sqrt(1 + g * g) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    tris = [[v[a], v[b], v[c]] for a, b, c in f]
    for _ in range(subdivisions):
        nxt = []
        for a, b, c in tris:
            ab, bc, ca = ((a + b) / 2, (b + c) / 2, (c + a) / 2)
            ab, bc, ca = (p / np.linalg.norm(p) for p in (ab, bc, ca))
            nxt += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        tris = nxt
    t = np.asarray(tris) * radius
    t = rotate_y(t, 0.37, (0, 0, 0))
    t = t[..., [1, 2, 0]]
    t = rotate_y(t, 0.21, (0, 0, 0))
    return t + np.asarray(centre, dtype=np.float64)


def to_mesh(cells_tris, dx, offset):
    """cell units -> the Float64 triangles an STL reader returns (Float32 values widened), to which `offset` is added"""
    world = np.asarray(cells_tris, dtype=np.float64) * dx - np.asarray(offset, dtype=np.float64)
    return world.astype(np.float32).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------
# STL files
# ----------------------------------------------------------------------------------------------------------------
def write_binary_stl(path, tri):
    t32 = np.asarray(tri, dtype=np.float32)
    with open(path, "wb") as fh:
        fh.write(b"made in code".ljust(80, b" "))
        fh.write(struct.pack("<I", t32.shape[0]))
        for t in t32:
            fh.write(struct.pack("<12fH", 0.0, 0.0, 0.0, *t.reshape(-1).tolist(), 0))


def write_ascii_stl(path, tri):
    t32 = np.asarray(tri, dtype=np.float32)
    with open(path, "w") as fh:
        fh.write("solid made_in_code\n")
        for t in t32:
            fh.write(" facet normal 0 0 0\n  outer loop\n")
            for p in t:
                fh.write("   vertex " + " ".join(repr(float(x)) for x in p) + "\n")     # repr of the widened Float32: parses back to it
            fh.write("  endloop\n endfacet\n")
        fh.write("endsolid made_in_code\n")


# ----------------------------------------------------------------------------------------------------------------
# mesh cases: voxelizer, fill, wall distance, q-map
# ----------------------------------------------------------------------------------------------------------------
DX_DYADIC = 2.0 ** -5
OFF_DYADIC = (0.25, 0.5, 0.125)


def _case(name, coords, cells_tris, dx, offset, planted=False, exact=True, by_hand=None):
    return SimpleNamespace(name=name, coords=coords, tri=to_mesh(cells_tris, dx, offset), dx=dx, offset=np.asarray(offset, dtype=np.float64),
                           planted=planted, exact=exact, by_hand=by_hand or {})


def _n(n):
    """global cell index n (1-based, per axis) on a level whose blocks start at 1 -> (x, y, z, block) 0-based of a full(3, 3, 3) level"""
    l = [(v - 1) % 8 for v in n]
    b = [(v - 1) // 8 for v in n]
    return (l[0], l[1], l[2], b[0] + 3 * b[1] + 9 * b[2])


def _height_case(name, dx, h):
    """a two-triangle sheet a planted height h below the centre of cell n = (6, 6, 6): Float32 vertices at z = 0, the height in the offset"""
    zc = (6 - 0.5) * dx
    off = (0.0, 0.0, zc - h)
    sheet = np.asarray(quad((1.3, 1.2, 0), (14.6, 1.2, 0), (14.6, 14.9, 0), (1.3, 14.9, 0)), dtype=np.float64)
    tri = sheet * dx
    tri[..., 2] = 0.0
    c = SimpleNamespace(name=name, coords=full(2, 2, 2), tri=tri.astype(np.float32).astype(np.float64), dx=dx,
                        offset=np.asarray(off), planted=True, exact=False, by_hand={})
    return c


SLIVER_D = 1.5e-6 / DX_DYADIC                      # 1.5e-6 m in cell units of the dyadic level
SLIVER_X, SLIVER_Y = 18.5 + 0.75 * 1.001, 5.5 + 0.75 * 1.001     # the x-high, y-high box edge of cell (19, 6, 6), in cell units
SLIVERS = (1, 2)                                   # their places in edge_triangles


def mesh_cases():
    out = {}
    # --- aligned box, faces on a cell face (9.0) and on cell centres (14.5), dyadic dx: every link evaluates exactly
    box = box_mesh((9.0, 9.0, 9.0), (14.5, 14.5, 14.5))
    c = _case("box_dyadic", full(3, 3, 3), box, DX_DYADIC, OFF_DYADIC, planted=True)
    c.by_hand = dict(
        n_obstacle_after_fill=343,                      # cells 9..15 per axis: shell where a coordinate is 9, 10 or 15, the rest filled
        fill=64,                                        # cells 11..14 per axis
        q={(_n((9, 11, 12)), K(1, 0, 0)): 0.5,          # centre 8.5, face 9.0
           (_n((16, 11, 12)), K(-1, 0, 0)): 1.0,        # centre 15.5, face 14.5: the inclusion boundary q <= 1
           (_n((15, 11, 12)), K(-1, 0, 0)): 0.0,        # centre ON the face x = 14.5 (t = 0); the face x = 9 is 5.5 cells away
           (_n((15, 11, 12)), K(1, 0, 0)): 0.0,         # t = 0 again: no link
           (_n((8, 11, 12)), K(1, 0, 0)): 0.0,          # 1.5 cells: out of range
           (_n((12, 16, 12)), K(0, -1, 0)): 1.0,
           (_n((12, 12, 9)), K(0, 0, 1)): 0.5,
           # the ray meets the diagonal of the face x = 9 (y = z): u + v = 1 on one triangle, v = 0 on the other, both inclusive
           (_n((9, 12, 12)), K(1, 0, 0)): 0.5,
           # diagonal links through the shared edge (y = z = 12 on x = 9, from centre (8.5, 11.5, 11.5) along (1, 1, 1) / sqrt(3)):
           # the hit is (9, 12, 12), on the diagonal; q = 0.5
           (_n((9, 12, 12)), K(1, 1, 1)): 0.5},
        # a centre ON the face x = 14.5: every ray either stays in the plane (|a| < EPSILON), leaves it at t = 0, or meets another face
        # more than a cell away - the cell is solid and not listed
        listed=[(_n((16, 11, 12)), True), (_n((15, 11, 12)), False), (_n((7, 11, 12)), False)],
        wall={_n((8, 12, 12)): 1, _n((8, 8, 8)): 3, _n((8, 8, 12)): 2, _n((7, 12, 12)): 0, _n((12, 12, 12)): 0})
    out[c.name] = c
    # --- the same kind of box at dx = 0.02 (not dyadic): x faces on the centre 10.5 and the cell face 23.0 (clear of the min-x blocks, whose fluid cells are seeds), as decimal metres
    dx = 0.02
    tri = np.asarray(box_mesh((-0.125, -0.13, -0.13), (0.125, 0.13, 0.13)), dtype=np.float32).astype(np.float64)
    out["box_002"] = SimpleNamespace(name="box_002", coords=full(3, 3, 3), tri=tri, dx=dx, offset=np.asarray([0.335, 0.25, 0.25]),
                                     planted=True, exact=False, by_hand={})
    # --- planted heights above a sheet (float literals: their side of EPSILON was confirmed in the written-order restatement)
    cell = (5, 5, 5, 0)
    down = [K(cx, cy, -1) for cx in (-1, 0, 1) for cy in (-1, 0, 1)]
    c = _height_case("height_below_epsilon", 0.02, 0.5e-9)
    c.by_hand = dict(q={(cell, k): 0.0 for k in down}, listed=[(cell, False)])
    out[c.name] = c
    c = _height_case("height_above_epsilon", 0.02, 2e-9)
    c.by_hand = dict(q={(cell, k): 1e-7 for k in down}, listed=[(cell, True)])              # Float16(1e-7) = 2 * 2^-24, positive
    out[c.name] = c
    c = _height_case("height_rounds_to_zero", 0.05, 1.2e-9)
    c.by_hand = dict(q={(cell, k): 0.0 for k in range(27)}, listed=[(cell, True)])          # q = 2.4e-8 < 2^-25: an all-zero listed row
    out[c.name] = c
    # --- thin closed slabs, a quarter cell thick; their edges keep clear of every link line (the distances of x0, x1, y0, y1 and the z faces
    # from the cell centres are pairwise different, so no diagonal link meets an edge); the z-low face comes first in the mesh, so "first hit" takes the farther face from above
    slabs = np.concatenate([box_mesh((3.28125, 2.8125, 10.625), (20.71875, 20.4375, 10.875)),
                            box_mesh((3.28125, 2.8125, 12.0625), (20.71875, 20.4375, 12.3125))])
    c = _case("slab_aligned", full(3, 3, 3), slabs, DX_DYADIC, OFF_DYADIC)
    c.by_hand = dict(fill=0,
                     q={(_n((12, 12, 12)), K(0, 0, -1)): 0.625,        # centre 11.5: top face 10.875 wins over the bottom face 10.625
                        (_n((12, 12, 12)), K(0, 0, 1)): 0.5625,        # and the link opposite is cut by the other slab
                        (_n((12, 12, 12)), K(1, 1, -1)): 0.625,
                        (_n((12, 12, 11)), K(0, 0, 1)): 0.125,         # centre 10.5, from below: bottom face 10.625
                        (_n((12, 12, 13)), K(0, 0, -1)): 0.1875})      # centre 12.5, above the upper slab's top face 12.3125
    out[c.name] = c
    tilted = rotate_y(box_mesh((3.28125, 2.8125, 10.625), (20.71875, 20.4375, 10.875)), 0.11, (12.0, 12.0, 10.75))
    c = _case("slab_tilted", full(3, 3, 3), tilted, DX_DYADIC, OFF_DYADIC)
    c.by_hand = dict(fill=0)
    out[c.name] = c
    # --- an open sheet: marked, never filled; hit from the front and from the back alike
    sheet = np.asarray(quad((3.28125, 2.8125, 10.25), (20.71875, 2.8125, 10.25), (20.71875, 20.4375, 10.25), (3.28125, 20.4375, 10.25)))
    c = _case("open_sheet", full(3, 3, 3), sheet, DX_DYADIC, OFF_DYADIC)
    c.by_hand = dict(fill=0, q={(_n((12, 13, 11)), K(0, 0, -1)): 0.25, (_n((12, 13, 10)), K(0, 0, 1)): 0.75, (_n((12, 13, 10)), K(-1, 1, 1)): 0.75})
    out[c.name] = c
    # --- a lone triangle whose corner v2 sits on a -z link: u = 1 and v = 0 exactly (dyadic, and a = e1 x e2 = 8 dx^2 is a power of two, so
    # f = 1 / a and u = f * a are exact); `u > 1.0` must let it through. v1 lies on a link line too (u = v = 0)
    lone = np.asarray([[(10.5, 10.5, 12.25), (12.5, 12.5, 12.25), (10.5, 14.5, 12.25)]])
    c = _case("vertex_hit", full(3, 3, 3), lone, DX_DYADIC, OFF_DYADIC, planted=True, exact=False)
    c.by_hand = dict(fill=0, q={(_n((13, 13, 13)), K(0, 0, -1)): 0.25, (_n((13, 13, 12)), K(0, 0, 1)): 0.75, (_n((11, 11, 13)), K(0, 0, -1)): 0.25,
                                (_n((14, 13, 13)), K(0, 0, -1)): 0.0, (_n((12, 13, 13)), K(0, 0, -1)): 0.25})
    out[c.name] = c
    # --- general position
    a, b, c, d = (10.31, 5.17, 6.23), (23.43, 7.41, 8.19), (15.77, 18.61, 7.03), (16.29, 9.83, 19.47)
    tetra = np.asarray([[a, b, c], [a, c, d], [a, d, b], [b, d, c]])
    out["tetrahedron"] = _case("tetrahedron", full(3, 3, 3), tetra, 0.013, (0.031, 0.017, 0.023))
    out["icosphere80"] = _case("icosphere80", full(3, 2, 2), icosphere((16.13, 7.81, 8.29), 5.07, 1), 0.013, (0.031, 0.017, 0.023))
    # the finest level of a 2-level nest: block indices that do not start at 1, a ragged block set (one corner block absent)
    nest = [b for b in full(3, 3, 3, lo=(3, 5, 3)) if b != (5, 7, 5)]
    shift = np.asarray((16.0, 32.0, 16.0))
    out["tetrahedron_nested"] = _case("tetrahedron_nested", nest, tetra + shift, 0.0065, (0.031, 0.017, 0.023))
    out["icosphere80_nested"] = _case("icosphere80_nested", nest, icosphere((28.13, 43.81, 28.29), 5.07, 1), 0.0065, (0.031, 0.017, 0.023))
    out["icosphere320_nested"] = _case("icosphere320_nested", nest, icosphere((28.13, 43.81, 28.29), 5.07, 2), 0.0065, (0.031, 0.017, 0.023))
    # --- triangles at the edges of the definition, all in one mesh
    c0 = np.asarray((12.5, 12.5, 12.5))
    edge = [
        [(5.25, 5.25, 5.25), (5.25, 5.25, 5.25), (7.75, 6.5, 5.25)],                       # two equal vertices
        # a sliver: edges of 5e-6 .. 7e-6 m, which survive Float32 at 0.6 m (ulp 6e-8 m): 0 < |a| < 1e-9 in every direction, and every cross
        # axis has 0 < dot(axis, axis) < 1e-10. It lies d = 1.5e-6 m OUTSIDE the x-high / y-high edge of the box of cell (19, 6, 6) (x + y >=
        # corner + d), its bounding box reaching d inside: the box axes do not separate it, its own cross axis (1, 1, 0) would, and is skipped
        [(SLIVER_X - SLIVER_D, SLIVER_Y + 2 * SLIVER_D, 5.5), (SLIVER_X + 2 * SLIVER_D, SLIVER_Y - SLIVER_D, 5.5),
         (SLIVER_X + 0.8 * SLIVER_D, SLIVER_Y + 0.5 * SLIVER_D, 5.5 + 3 * SLIVER_D)],
        # a second sliver straight below the centre of cell (6, 18, 18), 0.4 cells down, the link line through its inside: 0 < |a| < 1e-9 too
        [(5.5 - 2 * SLIVER_D, 17.5 - SLIVER_D, 17.1), (5.5 + 2 * SLIVER_D, 17.5 - SLIVER_D, 17.1 + 0.5 * SLIVER_D),
         (5.5 + 0.3 * SLIVER_D, 17.5 + 2 * SLIVER_D, 17.1 - 0.7 * SLIVER_D)],
        [(-40.0, -35.0, 20.3), (70.0, -30.0, 20.3), (10.0, 90.0, 20.3)],                   # larger than the level
        [(-3.0, 2.2, 3.3), (2.6, -4.0, 3.3), (2.2, 2.6, -3.0)],                            # reaches below block index 1
        list(map(tuple, c0 + np.asarray([(6.625, -2, -2), (-2, 6.625, -2), (-2, -2, 6.625)]))),   # only its normal separates it from cell 13
        [(15.3, 9.3, 9.3), (18.9, 9.3, 9.3), (15.3, 11.1, 10.7)],                          # an edge parallel to x: a cross axis is exactly 0
    ]
    c = _case("edge_triangles", full(3, 3, 3), np.asarray(edge, dtype=np.float64), DX_DYADIC, (0.0, 0.0, 0.0), planted=True, exact=False)
    c.by_hand = dict(
        solid=[(_n((13, 13, 13)), True),                   # x + y + z = 2.625 misses the box corner at 3 * 0.75075: an as-written quirk
               # the first sliver: the four cells whose boxes its bounding box touches, (19, 6, 6) among them although the sliver lies outside
               # its box - with every cross axis under 1e-10 only the box axes are left; and none of their neighbours
               (_n((19, 6, 6)), True), (_n((20, 6, 6)), True), (_n((19, 7, 6)), True), (_n((20, 7, 6)), True),
               (_n((18, 6, 6)), False), (_n((21, 7, 6)), False), (_n((19, 5, 6)), False), (_n((20, 8, 6)), False), (_n((19, 6, 5)), False),
               (_n((20, 7, 7)), False)],
        # no sliver cuts a link: |a| < EPSILON returns before any hit test, also for the ray that passes through the second one's inside
        q={(_n((6, 18, 18)), k): 0.0 for k in range(27)} | {(_n((20, 7, 6)), k): 0.0 for k in range(27)},
        listed=[(_n((6, 18, 18)), False), (_n((20, 7, 6)), False), (_n((19, 6, 6)), False)])
    out[c.name] = c
    return out


# ----------------------------------------------------------------------------------------------------------------
# shell cases: flood fill and wall distance on typed-in shells
# ----------------------------------------------------------------------------------------------------------------
def _shell(coords, solid_cells, fluid_cells=()):
    """bool [8,8,8,nb], F order, from global cell indices (1-based); blocks must start at (1, 1, 1) .. any set"""
    idx = {tuple(b): i for i, b in enumerate(coords)}
    a = np.zeros((8, 8, 8, len(coords)), dtype=bool, order="F")
    for cells, v in ((solid_cells, True), (fluid_cells, False)):
        for n in cells:
            b = tuple((c - 1) // 8 + 1 for c in n)
            a[(n[0] - 1) % 8, (n[1] - 1) % 8, (n[2] - 1) % 8, idx[b]] = v
    return a


def _hollow(lo, hi):
    r = lambda a: range(lo[a], hi[a] + 1)
    return [(x, y, z) for x in r(0) for y in r(1) for z in r(2)
            if x in (lo[0], hi[0]) or y in (lo[1], hi[1]) or z in (lo[2], hi[2])]


# the wall distances of the shell cases use a dx at which sqrt(Float32(d^2)) * Float32(dx) and Float32(sqrt(Float64(d^2)) * dx) differ for
# d^2 = 2 and 3 (at 0.02, 0.013, 0.0065, 0.05 and 2^-5 the two happen to round alike)
WALL_DX = 0.011


def shell_cases():
    """name -> namespace(coords, shell, fill by hand, fluid: cells that must stay fluid, filled: cells that must be filled)"""
    out = {}
    lvl = full(3, 2, 2)
    box = _hollow((10, 5, 5), (17, 12, 12))                         # walls one cell thick, interior 6^3
    out["hollow_sealed"] = SimpleNamespace(coords=lvl, shell=_shell(lvl, box), fill=216, fluid=[(9, 8, 8)], filled=[(11, 6, 6), (16, 11, 11)])
    out["hollow_one_cell_hole"] = SimpleNamespace(coords=lvl, shell=_shell(lvl, box, [(10, 8, 8)]), fill=0, fluid=[(11, 6, 6), (10, 8, 8)], filled=[])
    # the edge cell (10, 5, 8) touches the interior cell (11, 6, 8) only across an edge: the fill is 6-connected
    out["hollow_diagonal_gap"] = SimpleNamespace(coords=lvl, shell=_shell(lvl, box, [(10, 5, 8)]), fill=216, fluid=[(10, 5, 8)], filled=[(11, 6, 8)])
    # the body reaches into the min-x blocks: its interior cells there are seeds, and the whole interior hangs together
    low = _hollow((5, 5, 5), (12, 12, 12))
    out["hollow_in_min_x_block"] = SimpleNamespace(coords=lvl, shell=_shell(lvl, low), fill=0, fluid=[(6, 6, 6), (11, 11, 11)], filled=[])
    # an absent block is a wall: block (3, 1, 1) is cut off from the seeds by the missing (2, 1, 1); the y-row above it connects nothing
    ragged = [(1, 1, 1), (3, 1, 1), (1, 2, 1), (2, 2, 1)]
    plate = [(x, 9, z) for x in range(9, 17) for z in range(1, 9)]  # the floor of block (2, 2, 1), next to the absent block
    out["absent_block"] = SimpleNamespace(coords=ragged, shell=_shell(ragged, plate), fill=512, fluid=[(1, 1, 1), (9, 10, 1)], filled=[(17, 1, 1)])
    return out


# ----------------------------------------------------------------------------------------------------------------
# sponge cases: dyadic domains with cell centres exactly on outlet_start, inlet_thickness and the y and z starts
# ----------------------------------------------------------------------------------------------------------------
def sponge_cases():
    """name -> namespace(coords, dx_coarse, lvl_scale, domain_size, thickness (a Float32 value), symmetric)"""
    out = {}
    f32 = lambda x: float(np.float32(x))
    for lvl in (1, 2, 3):
        s = 2 ** (lvl - 1)
        coords = full(4 if lvl == 1 else 2, 2, 2) + ([(4 * s, 2 * s, 2 * s)] if lvl > 1 else [])
        for sym in (False, True):
            for st in (0.125, 0.25):
                out[f"sponge_L{lvl}_s{int(sym)}_t{st}"] = SimpleNamespace(coords=coords, dx_coarse=0.125, lvl_scale=s, domain_size=(4.0, 2.0, 2.0),
                                                                        thickness=f32(st), symmetric=sym)
    # Lx = 3.75: outlet_start = 2.8125, the centre of cell 23; Ly = Lz = 1.5: the y and z starts 0.1875 and 1.3125 are the centres of cells
    # 2 and 11. Lx = 3.125: Float64(3.125 * 0.02) = 0.0625 exactly, the centre of cell 1
    out["sponge_on_centres"] = SimpleNamespace(coords=full(4, 2, 2), dx_coarse=0.125, lvl_scale=1, domain_size=(3.75, 1.5, 1.5),
                                               thickness=f32(0.25), symmetric=False)
    out["sponge_inlet_on_centre"] = SimpleNamespace(coords=full(4, 2, 2), dx_coarse=0.125, lvl_scale=1, domain_size=(3.125, 1.5, 1.5),
                                                    thickness=f32(0.25), symmetric=True)
    out["sponge_thin"] = SimpleNamespace(coords=full(4, 2, 2), dx_coarse=0.125, lvl_scale=1, domain_size=(4.0, 2.0, 2.0),
                                         thickness=f32(0.1), symmetric=False)
    return out


# ----------------------------------------------------------------------------------------------------------------
# two planted cases taken through the whole set-up (preprocess.setup_multilevel_domain), for the device test: 2 levels, <= 64 blocks each
# ----------------------------------------------------------------------------------------------------------------
def device_case(name, folder):
    """-> (CaseConfig keyword arguments, path of the binary STL written into `folder`). Lengths in metres, L = 1.
    thin_slab        dx = 2^-5 on the fine level; a closed slab a quarter fine cell thick, tilted about y; wall model and sponge on
    aligned_box_002  dx = 0.02 on the fine level (the fixture cube's): x faces on the cell centre 24.5 and the cell face 37.0, y and z faces
                     on the centres 9.5 and 22.5, so that the axis links have q = 1.0 and q = 0.5; the body keeps clear of the level's min-x
                     blocks, whose fluid cells are seeds of the fill"""
    common = dict(stl_scale=1.0, num_levels=2, output_dir="out", steps=4, ramp_steps=1, output_freq=4, reference_length_for_meshing=1.0,
                  min_coarse_blocks=1, refinement_margin=0, bouzidi_levels=1)
    if name == "thin_slab":
        t = rotate_y(box_mesh((0.0, 0.0, 0.0), (0.3, 0.3, 1.0 / 128)), 0.11, (0.15, 0.15, 0.0))
        kw = dict(common, surface_resolution=32, wall_model_enabled=True, domain_upstream=0.8, domain_downstream=0.85, domain_lateral=0.3,
                  domain_height=0.45)
    elif name == "aligned_box_002":
        t = box_mesh((-0.125, -0.13, -0.13), (0.125, 0.13, 0.13))
        kw = dict(common, surface_resolution=50, wall_model_enabled=False, domain_upstream=0.49, domain_downstream=0.5, domain_lateral=0.18,
                  domain_height=0.18)
    else:
        raise KeyError(name)
    path = str(folder / (name + ".stl"))
    write_binary_stl(path, t)
    return dict(kw, stl_file=name + ".stl"), path
