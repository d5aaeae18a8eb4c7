"""Geometry and states for the surface-force tests (tests/test_force_reference_host.py, tests/test_gpu_force_reference.py).

Three small levels, triangle centres planted where the nearest-fluid-cell search can go wrong, and for every planted centre the cell
the search must end on, TYPED BY HAND from the reading of src/forces/surface.jl:138-240 below - no code computes an expectation.
Spacings are 0.5 and 1 and every coordinate is dyadic, so distances and ties are exact in float32 and in float64.

Levels (global cells are 1-based, cell g spans [(g - 1) dx, g dx), centre (g - 0.5) dx; block ids are 0-based positions in the sorted
block list, bx slowest, bz fastest):
  full   4 x 3 x 2 blocks, dx = 0.5 (a level 2), 32 x 24 x 16 cells; id = 6 bx0 + 2 by0 + bz0. No two grid dimensions are equal.
         Solid: the single cell (12,12,4); the single cell (16,4,4) on a block face; a plus of (20,12,4) with its -z, -y, -x, +x
         neighbours; the block-corner cell (8,8,8) with its -z, -y, -x neighbours; the 3 x 3 x 3 cube 27..29 x 19..21 x 11..13
         without its centre (28,20,12).
  boxes  6 x 3 x 3 blocks, dx = 1, 48 x 24 x 24 cells; id = 9 bx0 + 3 by0 + bz0. Solid cubes around a base cell, each with ONE corner
         cell left fluid, so the first shell that holds fluid holds only that corner and the next shell holds a strictly nearer face
         cell that must not be scanned: side 11 at 2..12 (corner (12,12,12)), side 7 at x 28..34, y, z 2..8 (corner (28,8,2)), side 5
         at x 37..41, y, z 2..6 (corner (41,2,6)); and a full side-11 cube at x 15..25, y, z 2..12: nothing within 5, fluid at 6.
  holes  _topology_cases._level1_holes(): 6 x 3 x 3 blocks, dx = 1, blocks (1,1,1) (2,3,1) (3,3,1) (4,2,2) (6,3,3) absent: full index
         f = 9 bx0 + 3 by0 + bz0 minus the number of absent blocks before it (f = 0, 15, 24, 31, 53).

A row: name, level, centre, search radius, mesh offset, the expected cell (None: no cell; else block, lx, ly, lz, all 0-based), the
situations it stands for, and `tie`: the winner is decided by order among equal distances or by a threshold (compared with ref32 and
this table only, never with ref64).
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from open_ludwig_amd import cases

import _force_ref as ref
import _surface_common as common
import _topology_cases as topo

F32 = np.float32
Row = namedtuple("Row", "name level centre radius offset expect tags tie")
NO_OFFSET = (0.0, 0.0, 0.0)
OFFSET = (0.25, -0.5, 0.125)
TAU = 0.5006

# every situation the table must hold (asserted by the host test)
SITUATIONS = ("generic", "on_face", "wd_below_half", "wd_half", "wd_above_half", "solid_six_fluid", "solid_two_fluid", "block_corner",
              "block_face", "first_at_2", "first_at_3", "first_at_5", "enclosed_at_0", "none_within_5", "fluid_at_6", "absent_block",
              "low_1", "low_2", "low_3", "high_1", "high_2", "high_3", "far", "radius_0", "radius_1", "radius_5", "radius_16",
              "offset_across_face", "equidistant")

ROWS = (
    # ---- full: 4 x 3 x 2, dx = 0.5 ----
    Row("generic", "full", (10.125, 7.375, 2.625), 5, NO_OFFSET, (14, 4, 6, 5), ("generic", "wd_below_half", "radius_5"), False),
    Row("generic_r0", "full", (10.125, 7.375, 2.625), 0, NO_OFFSET, (14, 4, 6, 5), ("radius_0",), False),
    # x = 10.0 is the face between cells 20 and 21: the base cell is the upper one, the lower one ties in shell 1 and loses
    Row("on_face", "full", (10.0, 7.375, 2.625), 5, NO_OFFSET, (14, 4, 6, 5), ("on_face", "wd_above_half", "equidistant"), True),
    Row("face_centred", "full", (10.0, 7.25, 2.75), 5, NO_OFFSET, (14, 4, 6, 5), ("on_face", "wd_half", "equidistant"), True),
    Row("cell_centre", "full", (10.25, 7.25, 2.75), 5, NO_OFFSET, (14, 4, 6, 5), ("wd_below_half",), False),
    # the point where eight blocks meet: base (9,9,9) in block (2,2,2); seven cells tie with it, one of them solid
    Row("corner_point", "full", (4.0, 4.0, 4.0), 5, NO_OFFSET, (9, 0, 0, 0), ("on_face", "block_corner", "equidistant"), True),
    # centre of the solid cell (12,12,4), six fluid face neighbours at equal distance: the first in dz, dy, dx order is (12,12,3)
    Row("solid_six", "full", (5.75, 5.75, 1.75), 5, NO_OFFSET, (8, 3, 3, 2), ("solid_six_fluid", "equidistant"), True),
    Row("solid_six_r1", "full", (5.75, 5.75, 1.75), 1, NO_OFFSET, (8, 3, 3, 2), ("radius_1", "equidistant"), True),
    Row("solid_six_r0", "full", (5.75, 5.75, 1.75), 0, NO_OFFSET, None, ("radius_0",), False),
    # centre of the solid cell (20,12,4): of the six only +y and +z are fluid; dz = 0 comes before dz = +1, so (20,13,4)
    Row("solid_two", "full", (9.75, 5.75, 1.75), 5, NO_OFFSET, (14, 3, 4, 3), ("solid_two_fluid", "equidistant"), True),
    # centre of the solid corner cell (8,8,8) of block (1,1,1): -z, -y, -x are solid, the first fluid face cell is +x, (9,8,8) in
    # block (2,1,1); the 26 neighbours lie in eight blocks
    Row("solid_corner", "full", (3.75, 3.75, 3.75), 5, NO_OFFSET, (6, 0, 7, 7), ("block_corner", "equidistant"), True),
    # centre of the solid cell (16,4,4) on the +x face of block (2,1,1): the first fluid face cell is (16,4,3)
    Row("solid_face", "full", (7.75, 1.75, 1.75), 5, NO_OFFSET, (6, 7, 3, 2), ("block_face", "equidistant"), True),
    # the fluid cell (28,20,12) whose 26 neighbours are all solid: found at radius 0, shell 1 is still scanned, nothing changes
    Row("enclosed", "full", (13.875, 9.875, 5.625), 5, NO_OFFSET, (23, 3, 3, 3), ("enclosed_at_0",), False),
    Row("enclosed_r0", "full", (13.875, 9.875, 5.625), 0, NO_OFFSET, (23, 3, 3, 3), ("enclosed_at_0", "radius_0"), False),
    # outside the domain: negative coordinates, base index <= 0; the cells at positive indices are still candidates
    Row("low_x1", "full", (-0.25, 5.125, 2.125), 5, NO_OFFSET, (2, 0, 2, 4), ("low_1",), False),
    Row("low_x2", "full", (-0.75, 5.125, 2.125), 5, NO_OFFSET, (2, 0, 2, 4), ("low_2", "first_at_2"), False),
    Row("low_x2_r1", "full", (-0.75, 5.125, 2.125), 1, NO_OFFSET, None, ("low_2", "radius_1"), False),
    Row("low_y3", "full", (5.125, -1.25, 2.125), 5, NO_OFFSET, (6, 2, 0, 4), ("low_3", "first_at_3"), False),
    Row("high_x1", "full", (16.25, 5.125, 2.125), 5, NO_OFFSET, (20, 7, 2, 4), ("high_1",), False),
    Row("high_y2", "full", (5.125, 12.75, 2.125), 5, NO_OFFSET, (10, 2, 7, 4), ("high_2",), False),
    Row("high_z3", "full", (5.125, 5.125, 9.25), 5, NO_OFFSET, (9, 2, 2, 7), ("high_3",), False),
    Row("far_high", "full", (516.125, 5.125, 2.125), 16, NO_OFFSET, None, ("far", "radius_16"), False),
    Row("far_low", "full", (5.125, -500.125, 2.125), 16, NO_OFFSET, None, ("far", "radius_16"), False),
    Row("generic_r16", "full", (10.125, 7.375, 2.625), 16, NO_OFFSET, (14, 4, 6, 5), ("radius_16",), False),
    # (9.875, 7.875, 2.5) lies in cell (20,16,6); the offset moves it across three faces into (21,15,6)
    Row("offset", "full", (9.875, 7.875, 2.5), 5, OFFSET, (14, 4, 6, 5), ("offset_across_face",), False),
    # ---- boxes: 6 x 3 x 3, dx = 1 ----
    # base (7,7,7) at the centre of the side-11 cube: shell 5 holds one fluid cell, the corner (12,12,12) at d2 = 75; (13,7,7) in
    # shell 6 is at d2 = 36 and is not scanned
    Row("first_at_5", "boxes", (6.5, 6.5, 6.5), 5, NO_OFFSET, (13, 3, 3, 3), ("first_at_5",), False),
    Row("first_at_5_r16", "boxes", (6.5, 6.5, 6.5), 16, NO_OFFSET, (13, 3, 3, 3), ("first_at_5", "radius_16"), False),
    Row("none_within_5", "boxes", (19.5, 6.5, 6.5), 5, NO_OFFSET, None, ("none_within_5",), False),
    # the same centre with radius 16: shell 6 is all fluid, six face cells at d2 = 36, the first in order is dz = -6: (20,7,1)
    Row("fluid_at_6", "boxes", (19.5, 6.5, 6.5), 16, NO_OFFSET, (18, 3, 6, 0), ("fluid_at_6", "radius_16", "equidistant"), True),
    Row("first_at_3", "boxes", (30.5, 4.5, 4.5), 5, NO_OFFSET, (27, 3, 7, 1), ("first_at_3",), False),
    Row("first_at_2", "boxes", (38.5, 3.5, 3.5), 5, NO_OFFSET, (45, 0, 1, 5), ("first_at_2",), False),
    Row("first_at_2_r1", "boxes", (38.5, 3.5, 3.5), 1, NO_OFFSET, None, ("radius_1",), False),
    # ---- holes: 6 x 3 x 3 with five blocks absent, dx = 1 ----
    # base (27,13,13) in the absent block (4,2,2) = cells 25..32 x 9..16 x 9..16: the first valid cells are in the plane x = 24
    Row("absent_r3", "holes", (26.5, 12.5, 12.5), 5, NO_OFFSET, (20, 7, 4, 4), ("absent_block", "first_at_3"), False),
    Row("absent_beside", "holes", (24.5, 12.5, 12.5), 1, NO_OFFSET, (20, 7, 4, 4), ("absent_block", "radius_1"), False),
    # base (-1,3,3): two cells below the domain AND beside the absent corner block (1,1,1): the first valid cells have gy = 9 or gz = 9,
    # in shell 6; (1,9,3) and (1,3,9) tie at d2 = 40 and dz = 0 comes before dz = +6
    Row("corner_low_r5", "holes", (-1.5, 2.5, 2.5), 5, NO_OFFSET, None, ("absent_block", "low_2", "none_within_5"), False),
    Row("corner_low", "holes", (-1.5, 2.5, 2.5), 16, NO_OFFSET, (2, 0, 0, 2), ("absent_block", "low_2", "fluid_at_6", "equidistant"), True),
    # base (50,21,21): two cells beyond the domain AND beside the absent corner block (6,3,3): (48,21,16) and (48,16,21) tie at
    # d2 = 29 in shell 5 and dz = -5 comes before dz = 0
    Row("corner_high", "holes", (49.5, 20.5, 20.5), 5, NO_OFFSET, (48, 7, 4, 7), ("absent_block", "high_2", "first_at_5", "equidistant"), True),
    Row("holes_generic", "holes", (37.25, 5.75, 19.5), 5, NO_OFFSET, (34, 5, 5, 3), ("generic",), False),
)

# the `full` level read with dx = float32(0.1): 0.5 / dx and 1.5 / dx round up to 5 and 15, so the base cell is (6,16,3), while the
# float32 distances put (5,15,3) strictly nearer: block (1,2,1) = id 2, local (4,6,2)
NON_DYADIC_DX = 0.1
NON_DYADIC_CENTRE = (0.5, 1.5, 0.25)
NON_DYADIC_EXPECT = (2, 4, 6, 2)

FULL_DIMS, BOXES_DIMS = (4, 3, 2), (6, 3, 3)
FULL_SOLID = ((12, 12, 4), (16, 4, 4),
              (20, 12, 4), (20, 12, 3), (20, 11, 4), (19, 12, 4), (21, 12, 4),
              (8, 8, 8), (8, 8, 7), (8, 7, 8), (7, 8, 8))
FULL_SHELL = ((27, 29), (19, 21), (11, 13), (28, 20, 12))                          # cube ranges (inclusive), the cell left fluid
BOXES_CUBES = (((2, 12), (2, 12), (2, 12), (12, 12, 12)),
               ((15, 25), (2, 12), (2, 12), None),
               ((28, 34), (2, 8), (2, 8), (28, 8, 2)),
               ((37, 41), (2, 6), (2, 6), (41, 2, 6)))


def _set_solid(level, g, value=True):
    gx, gy, gz = (int(v) - 1 for v in g)
    b = int(level.block_pointer[gx // 8, gy // 8, gz // 8]) - 1
    assert b >= 0, g
    level.obstacle[gx % 8, gy % 8, gz % 8, b] = value


def _fill_cube(level, xr, yr, zr, hole):
    for gx in range(xr[0], xr[1] + 1):
        for gy in range(yr[0], yr[1] + 1):
            for gz in range(zr[0], zr[1] + 1):
                _set_solid(level, (gx, gy, gz))
    if hole is not None:
        _set_solid(level, hole, False)


def random_fields(level, seed=11):
    """rho / vel / vel_temp seeded as the uploaded fixture of tests/test_gpu_force_series.py"""
    rng = np.random.default_rng(seed)
    return {"rho": np.asfortranarray((1.0 + 0.02 * rng.standard_normal(level.rho.shape)).astype(F32)),
            "vel": np.asfortranarray((0.05 * rng.standard_normal(level.vel.shape)).astype(F32)),
            "vel_temp": np.asfortranarray((0.05 * rng.standard_normal(level.vel.shape)).astype(F32))}


def build_level(name):
    """a fresh host level of the table"""
    if name == "full":
        g = cases.make_level(2, cases.full_box_coords(*FULL_DIMS), FULL_DIMS, 0.5 + (TAU - 0.5) / 2)
        for c in FULL_SOLID:
            _set_solid(g, c)
        _fill_cube(g, *FULL_SHELL)
    elif name == "boxes":
        g = cases.make_level(1, cases.full_box_coords(*BOXES_DIMS), BOXES_DIMS, TAU)
        for cube in BOXES_CUBES:
            _fill_cube(g, *cube)
    elif name == "holes":
        g = topo._level1_holes()[0][0]
    else:
        raise KeyError(name)
    assert g.n_blocks <= 54
    return g


def params(offset=NO_OFFSET, pressure_scale=None, moment_center=(3.0, -2.0, 5.0)):
    """the physical scales the surface path reads; pressure_scale (a float32 value) overrides rho_physical * velocity_scale^2"""
    if pressure_scale is None:
        rho_phys, vscale = 1.225, 40.0
    else:
        rho_phys, vscale = float(F32(pressure_scale)), 1.0
    return SimpleNamespace(mesh_offset=np.array(offset, dtype=np.float64), rho_physical=rho_phys, velocity_scale=vscale, u_physical=2.0,
                           reference_area=10.0, reference_chord=3.0, moment_center=tuple(moment_center), time_scale=0.01)


def pressure_scale_of(p) -> np.float32:
    return F32(p.rho_physical * p.velocity_scale * p.velocity_scale)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v)).astype(F32)


def row_normals(n):
    """deterministic non-dyadic unit normals for the table's triangles"""
    rng = np.random.default_rng(5)
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def mesh_of(centres, normals, areas=None):
    n = len(centres)
    return SimpleNamespace(centers=np.asarray(centres, dtype=np.float64).reshape(n, 3), normals=np.asarray(normals, dtype=np.float64).reshape(n, 3),
                           areas=np.full(n, 0.25) if areas is None else np.asarray(areas, dtype=np.float64))


def groups(level_name):
    """the table's rows of one level grouped into calls: {(radius, offset): [rows]}"""
    out = {}
    for r in ROWS:
        if r.level == level_name:
            out.setdefault((r.radius, r.offset), []).append(r)
    return out


# ---- planted states: one triangle each, in its own generic fluid cell of `full` ----
State = namedtuple("State", "name normal rho u ref64")        # ref64: compared with the float64 reference too


def _umag32(x):
    x = F32(x)
    return np.sqrt(x * x)


def _threshold_speeds():
    """float32 speeds x with sqrt(x * x) just below, at and just above 1.0f-10 (u = (x, 0, 0), normal (0, 0, 1): u_t = u)"""
    gate = F32(1.0e-10)
    cand = [gate]
    for _ in range(4):
        cand = [np.nextafter(cand[0], F32(0.0))] + cand + [np.nextafter(cand[-1], F32(1.0))]
    below = max(x for x in cand if _umag32(x) < gate)
    at = [x for x in cand if _umag32(x) == gate]
    above = min(x for x in cand if _umag32(x) > gate)
    assert at and np.nextafter(below, F32(1.0)) <= at[0] and at[-1] <= np.nextafter(above, F32(0.0))
    return below, at[0], above


def planted_states():
    below, at, above = _threshold_speeds()
    n123 = _unit((1.0, 2.0, 3.0))
    slant = np.array([0.6, 0.0, 0.8], dtype=F32)
    z = np.array([0.0, 0.0, 1.0], dtype=F32)
    eps = F32(2.0 ** -23)
    return (
        State("parallel_dyadic_x", (1.0, 0.0, 0.0), 1.01, (0.0625, 0.0, 0.0), True),          # u_t exactly 0: no shear
        State("parallel_dyadic_minus_z", (0.0, 0.0, -1.0), 0.99, (0.0, 0.0, 0.03125), True),
        State("parallel_non_dyadic", n123, 1.01, tuple(F32(0.05) * n123), False),          # the rounding residue decides the gate
        State("ut_below_gate", z, 1.01, (below, 0.0, 0.0), False),
        State("ut_at_gate", z, 1.01, (at, 0.0, 0.0), False),
        State("ut_above_gate", z, 1.01, (above, 0.0, 0.0), False),
        State("rho_one", slant, 1.0, (0.03, -0.02, 0.01), True),                              # p = 0: not covered
        State("rho_below_one_ny0", slant, F32(1.0) - eps, (0.03, -0.02, 0.01), True),         # -p n_y A is a signed zero
        State("rho_above_one_ny0", slant, F32(1.0) + eps, (0.03, -0.02, 0.01), True),
        State("rho_nan", slant, np.nan, (0.03, -0.02, 0.01), False),
        State("rho_inf", slant, np.inf, (0.03, -0.02, 0.01), False),
        State("u_nan", slant, 1.01, (0.03, np.nan, 0.01), False),
        State("plain", n123, 0.98, (0.04, 0.01, -0.02), True),
    )


def state_cell(k):
    """global cell (1-based) of planted state k on `full`: a row of fluid cells away from every solid one"""
    return (3 + 2 * k, 18, 10)


def state_centre(k):
    g = state_cell(k)
    return tuple((v - 0.5) * 0.5 + d for v, d in zip(g, (0.0625, -0.125, 0.03125)))


def plant(level, fields, states):
    """write the planted states into copies of `fields` (both velocity buffers) -> (fields, mesh of the state triangles)"""
    out = {k: v.copy(order="F") for k, v in fields.items()}
    for k, s in enumerate(states):
        gx, gy, gz = (v - 1 for v in state_cell(k))
        b = int(level.block_pointer[gx // 8, gy // 8, gz // 8]) - 1
        assert b >= 0 and not level.obstacle[gx % 8, gy % 8, gz % 8, b]
        out["rho"][gx % 8, gy % 8, gz % 8, b] = F32(s.rho)
        for name in ("vel", "vel_temp"):
            out[name][gx % 8, gy % 8, gz % 8, b, :] = np.asarray(s.u, dtype=F32)
    mesh = mesh_of([state_centre(k) for k in range(len(states))], [s.normal for s in states],
                   areas=[0.25 + 0.125 * k for k in range(len(states))])
    return out, mesh


# ---- the coverage threshold ----
def threshold_pressure_scale():
    """a float32 pressure_scale near 2.5e-3 at which rho = 1 + 2^-23 gives |p| == float32(1e-10) exactly, or None. float32(1e-10) is
    1.00000001335e-10: the reference's Float64 comparison with 1e-10 counts that triangle, a float32 comparison with 1e-10f does not."""
    target = F32(1.0e-10)
    q = (F32(1.0) + F32(2.0 ** -23) - F32(1.0)) / F32(3.0)
    s = F32(float(target) / float(q))
    lo = s
    for _ in range(8):
        lo = np.nextafter(lo, F32(0.0))
    for _ in range(17):
        if F32(q * lo) == target:
            return lo
        lo = np.nextafter(lo, F32(1.0))
    return None


# ---- the realistic sets ----
def sphere_case():
    """the 322-triangle icosphere on the finest level of tunnel_with_sphere((4, 2, 2), levels=2): dx = 0.5"""
    grids, sparams = cases.tunnel_with_sphere((4, 2, 2), levels=2, wall_model=True)
    mesh, center, radius = common.tunnel_sphere_mesh(grids, 2)
    return grids, sparams, mesh, common.tunnel_params(center, radius)


# ---- evaluation against the restatement, shared by the host and the device test ----
LEVELS = ("full", "boxes", "holes")


def ref_pair(g, fields, vel_name, mesh, params, radius, tau, dx=None):
    """(ref32, ref64) of map_stresses_kernel! for one call; ref64 remembers tau and pressure_scale for the e_ref scales"""
    ps = pressure_scale_of(params)
    a = (mesh.centers, mesh.normals, params.mesh_offset, g.dx if dx is None else dx, tau, ps, fields["rho"], fields[vel_name], g.obstacle,
         g.block_pointer, radius)
    with np.errstate(all="ignore"):
        r32, r64 = ref.map_stresses(*a, ft=np.float32), ref.map_stresses(*a, ft=np.float64)
    r64.tau_used, r64.ps_used = tau, ps
    return r32, r64


def e_ref_and_errors(got, r32, r64, compare):
    """-> (e_ref p, e_ref tau, err p, err tau, excluded): maxima over the triangles `compare` (bool) on which ref32 and ref64 agree
    on the cell and on both gates; e_ref is |ref32 - ref64| / scale, err is |got - ref64| / scale (got = four float32 arrays)"""
    same = (r32.cells.found == r64.cells.found) & (r32.cells.block == r64.cells.block) & (r32.cells.local == r64.cells.local).all(axis=1)
    same &= (r32.gates == r64.gates).all(axis=1)
    use = compare & same
    sp, st = ref.scales(r64.rho, r64.u, r64.cells.wall_dist, r64.tau_used, r64.ps_used)
    out = []
    for p, t in ((r32.p, r32.tau), (got[0], np.stack(got[1:], axis=1))):
        with np.errstate(invalid="ignore"):                                        # NaN / Inf states outside `use`
            dp = np.abs(p.astype(np.float64) - r64.p)[use] / sp[use]
            dt = np.abs(t.astype(np.float64) - r64.tau)[use]
        live = st[use] > 0
        assert not dt[~live].any()                                                 # u = 0 or nu = 0: no shear on either side
        out += [dp.max() if dp.size else 0.0, (dt[live] / st[use][live, None]).max() if live.any() else 0.0]
    return out[0], out[1], out[2], out[3], int((compare & ~same).sum())


def table_calls(levels):
    """every (what, level, fields, mesh, params, radius, compare-with-ref64 mask) of the table, the planted states included;
    levels = {name: (host level, fields)}"""
    for name in LEVELS:
        g, fields = levels[name]
        for (radius, offset), rows in groups(name).items():
            mesh = mesh_of([r.centre for r in rows], row_normals(len(rows)))
            yield f"{name} r{radius} {offset}", g, fields, mesh, params(offset), radius, np.array([not r.tie for r in rows])
    g, fields = levels["full"]
    states = planted_states()
    planted, mesh = plant(g, fields, states)
    yield "planted states", g, planted, mesh, params(), 5, np.array([s.ref64 for s in states])


def first_order_bound(contrib):
    """any float32 summation order of n terms is within n 2^-23 sum|x_i| of the exact sum to first order (derived in
    tests/test_force_series_host.py::test_tree_record_agrees_with_float32_sums_within_the_first_order_bound)"""
    c = np.asarray(contrib, dtype=np.float64)
    return c.shape[0] * 2.0 ** -23 * np.abs(c).sum(axis=0)
