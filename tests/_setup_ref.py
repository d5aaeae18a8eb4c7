"""A restatement of the five per-cell set-up passes, written from the reference's Julia alone (test infrastructure).

Independent of open_ludwig_amd.preprocess, open_ludwig_amd._setup_lib and open_ludwig_amd.cases (none of them is imported). Inputs are
plain arrays: the block coordinate list, Float64 triangles [T, 3, 3], dx, the mesh offset, the domain parameters as numbers. It never
writes to its inputs.

What it restates (file:line of the reference):
  src/domain_generation.jl:10-32     triangle_intersects_aabb: three box axes, nine cross axes, the 1e-10 skip, NO normal axis
  src/domain_generation.jl:74-112    voxelize_blocks!: box half 0.75 dx, cell centres ((b - 1) 8 + l - 0.5) dx
  src/domain_generation.jl:114-203   perform_flood_fill!
  src/domain_generation.jl:205-289   smooth_sponge_profile, apply_sponge!
  src/domain_generation.jl:371-434   compute_wall_distances!
  src/bouzidi_math.jl:9-47           ray_triangle_intersection (Moeller-Trumbore, EPSILON = 1e-9 on |a| and on t)
  src/bouzidi_math.jl:53-102         compute_q_for_cell: normalised direction, strict t < min_t, q = min_t / (dx norm(dir)), 0 < q <= 1
  src/bouzidi_setup.jl:115-137       Float16(q) where q_vals[k] > 0.0 in Float64; the cell is listed when any is

How it differs in structure from both implementations (preprocess.py's numpy path, csrc/setup_host.cpp):
  voxelizer, q-map   every cell of every block against ALL triangles: one triangle at a time over one flat array of all cells; no
                     binning (the reference: margin 2 dx and 2.5 dx, :46 and bouzidi_setup.jl:25), no bounding-box candidate filter.
                     A link is at most sqrt(3) dx long and a box reaches 0.75075 dx, both inside the reference's margins, so dropping
                     its bins adds no pair that could count; this form shows that the implementations' filters lose none.
  flood fill         stated as a set: the fluid cells that survive are the 6-connected components, through existing blocks only, that
                     hold a fluid cell of a block with the smallest bx; everything else is filled. Computed by merging labels along the
                     edge list to a fixed point (no queue, no image labelling).
  sponge             one scalar function of a cell's centre with the float type as a parameter: float64 defines the expected Float32
                     bits, numpy.longdouble gives reference values.
  wall distance      per fluid cell the SET of its 26 neighbour offsets that land on a solid cell of an existing block; the value is
                     the minimum over that set of sqrt(Float32(d^2)) * Float32(dx); the empty set and solid cells hold 100.0f0.
  neighbours         found by a sorted key of the global cell index, not through a dense volume or a block pointer grid.

Written operand order: dot(a, b) = (a1 b1 + a2 b2) + a3 b3 and cross as StaticArrays writes them, no fused multiply-add. Whether
StaticArrays' dot compiles to that or to muladd cannot be decided without running Julia ("Uncovered").

The exact arm (exact_voxels, exact_qmap) evaluates the same definitions without rounding: every input float is a dyadic rational, so
vertex + offset, the cell centres (n - 1/2) dx and every determinant are integers on a common power-of-two scale (Python integers,
so any case's coordinates allow it; fractions.Fraction only carries the quotients). It uses the unnormalised lattice direction c, so
q = tau / dx with P = o + tau c is a rational. Each inequality is judged three ways: as written, and with its threshold moved by a
relative DELTA to either side. A decision is `robust` when both moved forms agree; otherwise the link (cell) is `borderline`: the exact
quantity lies within DELTA of a threshold or of a Float16 tie. DELTA = 1e-9 is far above the float64 evaluation's own error (measured:
MAX_E_REF_Q), so a robust decision the float64 restatement misses is a defect, not rounding.
"""
from __future__ import annotations

import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

B = 8                                             # src/blocks.jl:14
EPSILON = 1e-9                                    # bouzidi_math.jl:14
SAT_TOL = 1.001                                   # domain_generation.jl:11
SAT_SKIP = 1e-10                                  # domain_generation.jl:25
DIRS = [(cx, cy, cz) for cz in (-1, 0, 1) for cy in (-1, 0, 1) for cx in (-1, 0, 1)]      # bouzidi_setup.jl:78-82, k = index
OPP = [26 - k for k in range(27)]
DELTA = Fraction(1, 10 ** 9)

# SAT exits (census): 0-2 a box axis separates, 3-11 cross axis (i, j) separates, 12 no axis separates (overlap)
SAT_EXITS = 13
# sponge branches (bit set = taken)
SP_OUTLET, SP_INLET, SP_YLOW, SP_YTOP, SP_ZLOW, SP_ZBACK, SP_PROFILE_ONE, SP_PROFILE_ZERO, SP_PROFILE_COS = (1 << i for i in range(9))


# ----------------------------------------------------------------------------------------------------------------
# cells: one flat list, block-major, then z, y, x (the memory order of the reference's [x, y, z, block] arrays)
# ----------------------------------------------------------------------------------------------------------------
def cell_index(coords):
    """global 1-based cell indices n[N, 3] of every cell of every block and the block of each cell"""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    l = np.arange(1, B + 1, dtype=np.int64)
    lz, ly, lx = np.meshgrid(l, l, l, indexing="ij")
    loc = np.stack([lx.ravel(), ly.ravel(), lz.ravel()], axis=1)                  # x fastest
    n = ((c[:, None, :] - 1) * B + loc[None, :, :]).reshape(-1, 3)
    return n, np.repeat(np.arange(c.shape[0]), B ** 3)


def to_blocks(flat, nb):
    """flat [N] (or [N, m]) -> [8, 8, 8, nb(, m)] indexed x, y, z, block"""
    a = np.asarray(flat)
    if a.ndim == 1:
        return a.reshape(nb, B, B, B).transpose(3, 2, 1, 0)
    return a.reshape(nb, B, B, B, a.shape[1]).transpose(3, 2, 1, 0, 4)


def centres(n, dx, T=np.float64):
    """((b - 1) * BLOCK_SIZE + l - 0.5) * dx, domain_generation.jl:89-91"""
    return (n.astype(T) - T(0.5)) * T(dx)


class _Lookup:
    """cells of existing blocks by global index: a sorted key, searched"""

    def __init__(self, n):
        self.span = int(n.max()) + 3
        self.key = self._k(n)
        self.order = np.argsort(self.key)
        self.sorted = self.key[self.order]

    def _k(self, n):
        return (n[:, 2] * self.span + n[:, 1]) * self.span + n[:, 0]

    def find(self, n):
        """index of the cell at global index n[N, 3], -1 where no block holds it"""
        ok = (n >= 1).all(axis=1) & (n < self.span - 1).all(axis=1)
        k = self._k(np.where(ok[:, None], n, 1))
        pos = np.minimum(np.searchsorted(self.sorted, k), len(self.sorted) - 1)
        hit = ok & (self.sorted[pos] == k)
        return np.where(hit, self.order[pos], -1)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


# ----------------------------------------------------------------------------------------------------------------
# voxelizer
# ----------------------------------------------------------------------------------------------------------------
def voxelize(coords, tri, dx, offset):
    """-> (shell bool [8,8,8,nb], census: SAT exits [13], cross axes skipped). domain_generation.jl:10-32, :74-112"""
    n, _ = cell_index(coords)
    c = centres(n, dx)
    cen = (c[:, 0], c[:, 1], c[:, 2])
    v = np.asarray(tri, dtype=np.float64) + np.asarray(offset, dtype=np.float64)           # :97-99
    half = 0.75 * dx                                                                        # :79
    h = half * SAT_TOL                                                                      # :12
    shell = np.zeros(n.shape[0], dtype=bool)
    exits = np.zeros(SAT_EXITS, dtype=np.int64)
    skipped = skipped_nonzero = 0
    unit = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    for t in v:
        t1, t2, t3 = (tuple(t[p, a] - cen[a] for a in range(3)) for p in range(3))          # :13
        live = np.ones(n.shape[0], dtype=bool)
        for a in range(3):                                                                  # :15-17
            lo = np.minimum(np.minimum(t1[a], t2[a]), t3[a])
            hi = np.maximum(np.maximum(t1[a], t2[a]), t3[a])
            out = live & ((lo > h) | (hi < -h))
            exits[a] += int(out.sum())
            live &= ~out
        f = (tuple(t2[a] - t1[a] for a in range(3)), tuple(t3[a] - t2[a] for a in range(3)), tuple(t1[a] - t3[a] for a in range(3)))
        for i in range(3):
            for j in range(3):
                if not live.any():
                    break
                ax = _cross(unit[i], f[j])                                                  # :24
                use = ~(_dot(ax, ax) < SAT_SKIP)                                            # :25
                skipped += int((live & ~use).sum())
                skipped_nonzero += int((live & ~use & (_dot(ax, ax) > 0.0)).sum())
                p1, p2, p3 = _dot(t1, ax), _dot(t2, ax), _dot(t3, ax)                       # :26
                r = h * np.abs(ax[0]) + h * np.abs(ax[1]) + h * np.abs(ax[2])               # :27
                sep = (np.minimum(p1, np.minimum(p2, p3)) > r) | (np.maximum(p1, np.maximum(p2, p3)) < -r)
                out = live & use & sep
                exits[3 + 3 * i + j] += int(out.sum())
                live &= ~out
        exits[12] += int(live.sum())
        shell |= live
    return to_blocks(shell, len(coords)).copy(), SimpleNamespace(exits=exits, skipped=skipped, skipped_nonzero=skipped_nonzero)


# ----------------------------------------------------------------------------------------------------------------
# flood fill, as a set
# ----------------------------------------------------------------------------------------------------------------
def _components(n_nodes, a, b):
    """labels of the connected components of the graph with edges (a[i], b[i]): minimum-label merging to a fixed point"""
    lab = np.arange(n_nodes)
    while True:
        m = np.minimum(lab[a], lab[b])
        new = lab.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        while True:                                  # follow every label to its own label
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            return lab
        lab = new


def flood_fill(coords, shell):
    """-> (obstacle bool [8,8,8,nb] after the fill, fill count). domain_generation.jl:114-203"""
    n, blk = cell_index(coords)
    nb = len(coords)
    solid = np.asarray(shell).transpose(3, 2, 1, 0).reshape(-1).astype(bool)
    look = _Lookup(n)
    ea, eb = [], []
    for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):                                                                       # :137-139, one of each +/- pair
        j = look.find(n + np.asarray(d))
        ok = (j >= 0) & ~solid
        ok[ok] &= ~solid[j[ok]]
        ea.append(np.flatnonzero(ok))
        eb.append(j[ok])
    lab = _components(n.shape[0], np.concatenate(ea), np.concatenate(eb))
    bx = np.asarray(coords, dtype=np.int64).reshape(-1, 3)[:, 0]
    seed = (bx[blk] == bx.min()) & ~solid                                                   # :121-134
    alive = np.isin(lab, np.unique(lab[seed])) & ~solid
    fill = ~solid & ~alive                                                                  # :195-201
    return to_blocks(solid | fill, nb).copy(), int(fill.sum())


# ----------------------------------------------------------------------------------------------------------------
# sponge
# ----------------------------------------------------------------------------------------------------------------
def sponge_value(px, py, pz, Lx, Ly, Lz, thickness, symmetric, T=np.float64):
    """-> (sponge value in T before the Float32 rounding, branch bits). domain_generation.jl:205-289. `thickness` is
    Float64(SPONGE_THICKNESS), the widened Float32 setting (config_loader.jl:171)."""
    px, py, pz, Lx, Ly, Lz, st = (T(x) for x in (px, py, pz, Lx, Ly, Lz, thickness))
    pi = T(math.pi) if T is np.float64 else T(4) * np.arctan(T(1))      # `π * x` is Float64(π) * x in the reference
    bits = 0

    def profile(x, thick):                            # :205-213
        nonlocal bits
        if x <= T(0):
            bits |= SP_PROFILE_ONE
            return T(1)
        if x >= thick:
            bits |= SP_PROFILE_ZERO
            return T(0)
        bits |= SP_PROFILE_COS
        return T(0.5) * (T(1) + np.cos(pi * x / thick))

    outlet_t = Lx * max(st, T(0.15))                  # :223
    inlet_t = Lx * T(0.02)                            # :225
    y_t = Ly * st * T(0.5)                            # :226
    z_t = Lz * st * T(0.5)                            # :227
    outlet_start, y_top, z_back = Lx - outlet_t, Ly - y_t, Lz - z_t
    val = T(0)
    if px > outlet_start:                             # :247
        bits |= SP_OUTLET
        val = max(val, profile(outlet_t - (px - outlet_start), outlet_t) * T(1.0))
    if px < inlet_t:                                  # :253
        bits |= SP_INLET
        val = max(val, profile(px, inlet_t) * T(0.05))
    if (not symmetric) and py < y_t:                  # :258
        bits |= SP_YLOW
        val = max(val, profile(py, y_t) * T(0.1))
    if py > y_top:                                    # :263
        bits |= SP_YTOP
        val = max(val, profile(y_t - (py - y_top), y_t) * T(0.1))
    if pz < z_t:                                      # :269
        bits |= SP_ZLOW
        val = max(val, profile(pz, z_t) * T(0.1))
    if pz > z_back:                                   # :274
        bits |= SP_ZBACK
        val = max(val, profile(z_t - (pz - z_back), z_t) * T(0.1))
    return val, bits


def sponge(coords, dx_coarse, lvl_scale, domain_size, thickness, symmetric, T=np.float64):
    """-> (values of type T [8,8,8,nb] BEFORE the Float32 rounding, branch bits [8,8,8,nb]); dx = dx_coarse / lvl_scale (:217)"""
    n, _ = cell_index(coords)
    dx = T(dx_coarse) / T(lvl_scale)
    c = centres(n, dx, T)
    val = np.zeros(n.shape[0], dtype=T)
    bits = np.zeros(n.shape[0], dtype=np.int64)
    for i in range(n.shape[0]):
        val[i], bits[i] = sponge_value(c[i, 0], c[i, 1], c[i, 2], *domain_size, thickness, symmetric, T)
    return to_blocks(val, len(coords)).copy(), to_blocks(bits, len(coords)).copy()


# ----------------------------------------------------------------------------------------------------------------
# wall distance
# ----------------------------------------------------------------------------------------------------------------
def wall_distance(coords, obstacle, dx, absent_box=None):
    """-> (Float32 [8,8,8,nb], census: cells per nearest d^2 {1, 2, 3}, neighbours skipped for an absent block).
    domain_generation.jl:371-434"""
    n, blk = cell_index(coords)
    solid = np.asarray(obstacle).transpose(3, 2, 1, 0).reshape(-1).astype(bool)
    look = _Lookup(n)
    best = np.full(n.shape[0], np.float32(100.0), dtype=np.float32)                         # :394
    d2min = np.zeros(n.shape[0], dtype=np.int64)
    skipped = skipped_in_box = 0
    for d in DIRS:
        d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if d2 == 0:
            continue
        j = look.find(n + np.asarray(d))
        skipped += int(((j < 0) & ~solid).sum())                                            # :414-416
        if absent_box is not None:                  # census only: skipped neighbours inside a given box of global cell indices
            m = n + np.asarray(d)
            skipped_in_box += int(((j < 0) & ~solid & (m >= np.asarray(absent_box[0])).all(axis=1) & (m <= np.asarray(absent_box[1])).all(axis=1)).sum())
        lands = (j >= 0) & ~solid
        lands[lands] &= solid[j[lands]]                                                     # :419
        dist = np.sqrt(np.float32(d2)) * np.float32(dx)                          # :421
        better = lands & (dist < best)
        best = np.where(lands, np.minimum(best, dist), best)                                # :422
        d2min = np.where(better, d2, d2min)
    census = SimpleNamespace(nearest={k: int((d2min == k).sum()) for k in (1, 2, 3)}, skipped=skipped, skipped_in_box=skipped_in_box)
    return to_blocks(best, len(coords)).copy(), census


# ----------------------------------------------------------------------------------------------------------------
# Bouzidi q-map
# ----------------------------------------------------------------------------------------------------------------
def qmap(coords, tri, dx, offset):
    """-> namespace(q64 Float64 [8,8,8,nb,27] (0 where no link), q16 Float16 [8,8,8,nb,27], listed bool [8,8,8,nb], cells: the set of
    (block, x, y, z), 1-based). bouzidi_math.jl:9-102, bouzidi_setup.jl:100-137"""
    n, blk = cell_index(coords)
    N = n.shape[0]
    c = centres(n, dx)
    org = (c[:, 0], c[:, 1], c[:, 2])
    v = np.asarray(tri, dtype=np.float64) + np.asarray(offset, dtype=np.float64)           # bouzidi_math.jl:78-80
    min_t = np.full((27, N), np.inf)
    dirn = []
    for k, d in enumerate(DIRS):
        dv = np.array(d, dtype=np.float64)
        nrm = math.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])
        dirn.append(tuple(dv / nrm) if k != 13 else None)                                   # :73
    for t in v:
        v1, v2, v3 = t
        e1 = tuple(v2 - v1)                                                                 # :16
        e2 = tuple(v3 - v1)                                                                 # :17
        s = tuple(org[a] - v1[a] for a in range(3))                                         # :26
        qv = _cross(s, e1)                                                                  # :33
        tq = _dot(e2, qv)                                                                   # :40, before f
        for k in range(27):
            if k == 13:
                continue
            dn = dirn[k]
            h = _cross(dn, e2)                                                              # :18
            a = _dot(e1, h)                                                                 # :19
            if abs(a) < EPSILON:                                                            # :21
                continue
            f = 1.0 / a                                                                     # :25
            u = f * _dot(s, h)                                                              # :27
            w = f * _dot(dn, qv)                                                            # :34
            tt = f * tq
            hit = ~((u < 0.0) | (u > 1.0)) & ~((w < 0.0) | (u + w > 1.0)) & (tt > EPSILON)  # :29, :36, :42
            mt = min_t[k]
            better = hit & (tt < mt)                                                        # :84
            mt[better] = tt[better]
    q64 = np.zeros((N, 27))
    for k, d in enumerate(DIRS):
        if k == 13:
            continue
        dv = np.array(d, dtype=np.float64)
        cmag = math.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])                   # :91
        with np.errstate(invalid="ignore"):
            q = min_t[k] / (dx * cmag)                                                      # :92
        keep = np.isfinite(min_t[k]) & (q > 0.0) & (q <= 1.0)                               # :90, :94
        q64[keep, k] = q[keep]
    q16 = np.where(q64 > 0.0, q64, 0.0).astype(np.float16)                                  # bouzidi_setup.jl:127-128
    listed = (q64 > 0.0).any(axis=1)                                                        # :127, :130
    nb = len(coords)
    loc = n - (np.asarray(coords, dtype=np.int64).reshape(-1, 3)[blk] - 1) * B
    cells = {(int(blk[i]) + 1, int(loc[i, 0]), int(loc[i, 1]), int(loc[i, 2])) for i in np.flatnonzero(listed)}
    return SimpleNamespace(q64=to_blocks(q64, nb).copy(), q16=to_blocks(q16, nb).copy(), listed=to_blocks(listed, nb).copy(), cells=cells)


# ----------------------------------------------------------------------------------------------------------------
# the exact arm
# ----------------------------------------------------------------------------------------------------------------
def _scale(*groups):
    """the power of two M with x * M an integer for every float in the groups"""
    m = 1
    for g in groups:
        for x in np.asarray(g, dtype=np.float64).ravel():
            m = max(m, Fraction(float(x)).denominator)
    return m


def _int(x, M):
    y = Fraction(float(x)) * M
    assert y.denominator == 1
    return y.numerator


class _Exact:
    """integer geometry on the scale 2 M: vertices 2 M (v + offset), cell centres (2 n - 1) (M dx)"""

    def __init__(self, tri, dx, offset):
        self.M = _scale(tri, [dx], offset)
        M = self.M
        off = [_int(x, M) for x in offset]
        self.V = [[[2 * (_int(t[p][a], M) + off[a]) for a in range(3)] for p in range(3)] for t in np.asarray(tri, dtype=np.float64)]
        self.dxI = _int(dx, M)
        self.S = 2 * M
        self.dx = float(dx)
        self.vf = np.asarray(tri, dtype=np.float64) + np.asarray(offset, dtype=np.float64)

    def centre(self, n):
        return [(2 * int(n[a]) - 1) * self.dxI for a in range(3)]

    def near(self, n, reach):
        """(cell, triangle) pairs with the cell centre within `reach` (in dx) of the triangle's bounding box: a float filter with a
        margin far above any rounding, used only to leave out pairs that cannot matter"""
        c = centres(n, self.dx)
        lo, hi = self.vf.min(axis=1), self.vf.max(axis=1)
        out = []
        for t in range(self.vf.shape[0]):
            ok = ((c >= lo[t] - reach * self.dx) & (c <= hi[t] + reach * self.dx)).all(axis=1)
            out.append(np.flatnonzero(ok))
        return out


def _idot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def exact_voxels(coords, tri, dx, offset):
    """-> namespace(shell bool [N] as written in exact arithmetic, borderline bool [N]) over the flat cell list, and the [8,8,8,nb]
    views. The SAT of domain_generation.jl:10-32 on exact inputs: h = 0.75 dx 1.001 as the product of the three floats' exact values."""
    n, _ = cell_index(coords)
    ex = _Exact(tri, dx, offset)
    S = ex.S
    h = Fraction(0.75) * Fraction(float(dx)) * Fraction(SAT_TOL) * S
    skip = Fraction(SAT_SKIP) * S * S
    lo_f, hi_f = 1 - DELTA, 1 + DELTA
    N = n.shape[0]
    yes = np.zeros(N, dtype=bool)                    # as written
    robust_yes = np.zeros(N, dtype=bool)
    maybe = np.zeros(N, dtype=bool)                  # some triangle overlaps under the loose reading
    pairs = ex.near(n, 1.0)                          # the box axes alone separate every other pair: 0.75075 dx < 1 dx
    for t, cells in enumerate(pairs):
        V = ex.V[t]
        for i in cells:
            c = ex.centre(n[i])
            T = [[V[p][a] - c[a] for a in range(3)] for p in range(3)]
            f = [[T[1][a] - T[0][a] for a in range(3)], [T[2][a] - T[1][a] for a in range(3)], [T[0][a] - T[2][a] for a in range(3)]]
            written = robust_sep = False
            loose_sep = False
            tests = []
            for a in range(3):
                mn, mx = min(T[0][a], T[1][a], T[2][a]), max(T[0][a], T[1][a], T[2][a])
                tests.append((max(mn, -mx), h, True, True, True))
            for a in range(3):
                for j in range(3):
                    u = [0, 0, 0]
                    u[a] = 1
                    ax = _cross(u, f[j])
                    a2 = _idot(ax, ax)
                    p = [_idot(T[k], ax) for k in range(3)]
                    r = h * (abs(ax[0]) + abs(ax[1]) + abs(ax[2]))
                    # the axis is used as written / under both moved readings of the skip / under at least one
                    tests.append((max(min(p), -max(p)), r, not a2 < skip, (not a2 < skip * hi_f), (not a2 < skip * lo_f)))
            for gap, r, used, used_all, used_any in tests:
                if used and gap > r:
                    written = True
                if used_all and gap > r * hi_f:
                    robust_sep = True
                if used_any and gap > r * lo_f:
                    loose_sep = True
            if not written:
                yes[i] = True
            if not loose_sep:
                robust_yes[i] = True
            if not robust_sep:
                maybe[i] = True
    borderline = maybe & ~robust_yes                 # solid under one reading, not under the other
    nb = len(coords)
    return SimpleNamespace(shell=to_blocks(yes, nb).copy(), borderline=to_blocks(borderline, nb).copy())


def round_to_f16(q: Fraction):
    """-> (the Float16 nearest to q, ties to even, as numpy.float16; whether q (1 +- DELTA) round differently). 0 < q <= 1"""
    def rnd(x):
        e = -14
        if x >= Fraction(1, 2 ** 14):
            e = x.numerator.bit_length() - x.denominator.bit_length()
            if Fraction(2) ** e > x:
                e -= 1
        ulp = Fraction(2) ** (e - 10)
        m = x / ulp
        fl = m.numerator // m.denominator
        rem = m - fl
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
            fl += 1
        return fl * ulp
    r = rnd(q)
    out = np.float16(float(r))
    assert Fraction(float(out)) == r
    return out, rnd(q * (1 - DELTA)) != rnd(q * (1 + DELTA))


def exact_qmap(coords, tri, dx, offset, cells=None):
    """The q-map of bouzidi_math.jl:9-102 in exact arithmetic with the unnormalised direction c.
    -> dict (flat cell index, k) -> namespace(q Fraction or None as written, robust bool): every link that exists under ANY reading
    (as written, or with a threshold moved by DELTA). `cells`: flat indices to evaluate (default: every cell within 2 dx of a triangle)."""
    n, _ = cell_index(coords)
    ex = _Exact(tri, dx, offset)
    S = ex.S
    eps = Fraction(EPSILON)
    D9 = DELTA.denominator
    pairs = ex.near(n, 2.0)                          # a link reaches sqrt(3) dx
    want = None if cells is None else set(int(i) for i in cells)
    cf = centres(n, ex.dx)
    hits = {}                                        # (cell, k) -> list of (tau Fraction, written, robust)
    for t, cand in enumerate(pairs):
        if want is not None:
            cand = np.array([i for i in cand if int(i) in want], dtype=np.int64)
        if cand.size == 0:
            continue
        V = ex.V[t]
        e1 = [V[1][a] - V[0][a] for a in range(3)]
        e2 = [V[2][a] - V[0][a] for a in range(3)]
        # float pre-filter: barycentrics with the unnormalised c; a pair is dropped only when it misses by 1e-6 of the triangle AND
        # the ray is not near-parallel (|a| above 1e-6 of |e1| |c x e2|), so that float64's error (1e-16 times that ratio) is nowhere near
        vf = ex.vf[t]
        fe1, fe2 = vf[1] - vf[0], vf[2] - vf[0]
        sf = cf[cand] - vf[0]
        qf = np.cross(sf, fe1)
        for k, d in enumerate(DIRS):
            if k == 13:
                continue
            dv = np.array(d, dtype=np.float64)
            hf = np.cross(dv, fe2)
            af = float(fe1 @ hf)
            flat = abs(af) <= 1e-6 * np.linalg.norm(fe1) * np.linalg.norm(hf)
            if flat:
                sel = cand
            else:
                uf, wf, tf = sf @ hf / af, qf @ dv / af, qf @ fe2 / af
                keep = (uf > -1e-6) & (uf < 1 + 1e-6) & (wf > -1e-6) & (uf + wf < 1 + 1e-6) & (tf > -1e-6 * ex.dx) & (tf < 1.5 * ex.dx)
                sel = cand[keep]
            if sel.size == 0:
                continue
            c2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            h = _cross(d, e2)
            a = _idot(e1, h)
            # |a / (|c| S^2)| < EPSILON  <=>  a^2 < EPSILON^2 c2 S^4
            a_thr = eps * eps * c2 * S ** 4
            a_written = not a * a < a_thr
            a_all = not a * a < a_thr * (1 + DELTA) ** 2
            a_any = not a * a < a_thr * (1 - DELTA) ** 2
            if not a_any or a == 0:
                continue
            sg = 1 if a > 0 else -1
            A = a * sg
            for i in sel:
                o = ex.centre(n[i])
                s = [o[b] - V[0][b] for b in range(3)]
                U = _idot(s, h) * sg
                qv = _cross(s, e1)
                W = _idot(d, qv) * sg
                Tn = _idot(e2, qv) * sg
                # as written: 0 <= u <= 1, v >= 0, u + v <= 1, t > EPSILON with t = (Tn / A) |c| / S
                t_thr = eps * eps * A * A * S * S
                tw = Tn > 0 and Tn * Tn * c2 > t_thr
                written = a_written and U >= 0 and U <= A and W >= 0 and U + W <= A and tw
                robust = (a_all and U * D9 >= A and U * D9 <= A * (D9 - 1) and W * D9 >= A and (U + W) * D9 <= A * (D9 - 1)
                          and Tn > 0 and Tn * Tn * c2 > t_thr * (1 + DELTA) ** 2)
                loose = (U * D9 >= -A and U * D9 <= A * (D9 + 1) and W * D9 >= -A and (U + W) * D9 <= A * (D9 + 1)
                         and Tn > 0 and Tn * Tn * c2 > t_thr * (1 - DELTA) ** 2)
                if loose:
                    hits.setdefault((int(i), k), []).append((Fraction(Tn, A), written, robust))
    out = {}
    for key, lst in hits.items():
        scale = 2 * ex.dxI                           # tau is on the scale S = 2 M: q = tau / (S dx) = tau / (2 dxI)
        w = [h[0] for h in lst if h[1]]
        r = [h[0] for h in lst if h[2]]
        q_w = min(w) / scale if w else None
        if q_w is not None and not (q_w > 0 and q_w <= 1):
            q_w = None
        q_l = min(h[0] for h in lst) / scale         # nearest hit under the loose reading
        q_r = min(r) / scale if r else None
        if q_l > 1 + DELTA:
            continue                                 # whatever hits under any reading is out of range: robustly no link
        out[key] = SimpleNamespace(q=q_w, robust=q_r is not None and q_r == q_l and q_r <= 1 - DELTA)
    return out
