"""The case set-up (open_ludwig_amd/preprocess.py method="numpy", csrc/setup_host.cpp method="native") against the restatement
written from the reference's Julia alone (tests/_setup_ref.py) and against exact geometry. CPU only.

  bit for bit   both methods equal the float64 restatement on every case of tests/_setup_cases.py: the shell, the fill count, the
                obstacle after the fill, the wall_dist Float32 bits, the q_map Float16 bits, the boundary list as a set, the sponge bits
  by hand       both methods and the restatement equal every typed-in expectation of the planted cases
  exact arm     on the non-planted cases every voxel and link decision of the restatement is the exact one and every Float16 q is the
                exact q correctly rounded, except where the exact quantity lies within DELTA = 1e-9 (relative) of a threshold or of a
                Float16 tie; those are counted and capped by the step tests' MAX_EXCLUDED_SHARE
  accuracy      e_ref = |q_float64 - q_exact| and the sponge's |float64 - longdouble| in Float32 ulps, recorded with under 10 % on top

Measured (profiles/setup_reference.txt): e_ref 9.1e-14 at most (icosphere320_nested); excluded links and cells: 0 in each of the eight
non-planted cases; the sponge's float64 value lies within 8.1e-8 Float32 ulps of the longdouble one.
"""
import functools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import _setup_cases as C
import _setup_ref as R
from open_ludwig_amd import preprocess as pp

MAX_EXCLUDED_SHARE = 0.005           # tests/_step_ref.py: per case, of its cut links (of its shell cells)
MAX_E_REF_Q = 1.0e-13                # measured 9.1e-14 (|q_float64 - q_exact| over every non-planted link), under 10 % on top
MAX_SPONGE_ULP = 8.9e-8              # measured 8.1e-8: |float64 - longdouble| in Float32 ulps of the value, before the Float32 rounding
METHODS = ("native", "numpy")
MESH = C.mesh_cases()
SHELL = C.shell_cases()
SPONGE = C.sponge_cases()
# the planted knife-edges, by name: judged by the by-hand table and by the restatement's bits only, never by the exact arm's cap
PLANTED = ["box_dyadic", "box_002", "height_below_epsilon", "height_above_epsilon", "height_rounds_to_zero", "vertex_hit", "edge_triangles"]
NON_PLANTED = [n for n, c in MESH.items() if not c.planted]
assert sorted(PLANTED) == sorted(n for n, c in MESH.items() if c.planted)


@functools.lru_cache(maxsize=None)
def ref(name):
    """the restatement of one mesh case, computed once and shared"""
    c = MESH[name]
    shell, sat = R.voxelize(c.coords, c.tri, c.dx, c.offset)
    obstacle, fill = R.flood_fill(c.coords, shell)
    wall, wc = R.wall_distance(c.coords, obstacle, c.dx)
    q = R.qmap(c.coords, c.tri, c.dx, c.offset)
    for a in (shell, obstacle, wall, q.q64, q.q16, q.listed):
        a.setflags(write=False)
    return SimpleNamespace(shell=shell, sat=sat, obstacle=obstacle, fill=fill, wall=wall, wall_census=wc, q=q)


@functools.lru_cache(maxsize=None)
def impl(name, method):
    c = MESH[name]
    mesh = SimpleNamespace(triangles=c.tri)
    shell = pp.voxelize_blocks(c.coords, mesh, c.dx, c.offset, method=method)
    obstacle = np.array(shell, dtype=bool, order="F")
    fill = pp.perform_flood_fill(obstacle, c.coords, method=method)
    wall = pp.compute_wall_distances(c.coords, obstacle, c.dx, method=method)
    q, cb, cx, cy, cz, nbc = pp.compute_bouzidi_qmap_sparse(c.coords, mesh, c.dx, c.offset, shell, method=method)
    cells = {(int(b), int(x), int(y), int(z)) for b, x, y, z in zip(cb, cx, cy, cz)}
    assert len(cells) == nbc == len(cb)
    return SimpleNamespace(shell=np.asarray(shell), obstacle=obstacle, fill=fill, wall=wall, q16=q, cells=cells)


def bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ----------------------------------------------------------------------------------------------------------------
# bit for bit
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", list(MESH))
def test_mesh_case_equals_the_restatement_bit_for_bit(name, method):
    r, g = ref(name), impl(name, method)
    assert np.array_equal(g.shell, r.shell), f"shell: {int((g.shell != r.shell).sum())} cells differ"
    assert g.fill == r.fill
    assert np.array_equal(g.obstacle, r.obstacle)
    assert g.wall.dtype == np.float32 and np.array_equal(bits(g.wall), bits(r.wall))
    assert g.q16.dtype == np.float16 and g.q16.shape == r.q.q16.shape
    diff = bits(g.q16) != bits(r.q.q16)
    assert not diff.any(), f"q_map: {int(diff.sum())} links differ, first {np.argwhere(diff)[:3].tolist()}"
    assert g.cells == r.q.cells, (len(g.cells), len(r.q.cells))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", list(SHELL))
def test_shell_case_fill_and_wall_distance(name, method):
    c = SHELL[name]
    want, fill = R.flood_fill(c.coords, c.shell)
    wall, _ = R.wall_distance(c.coords, want, C.WALL_DX)
    got = np.array(c.shell, dtype=bool, order="F")
    assert pp.perform_flood_fill(got, c.coords, method=method) == fill == c.fill                    # c.fill: by hand
    assert np.array_equal(got, want)
    idx = {tuple(b): i for i, b in enumerate(c.coords)}
    at = lambda n: got[(n[0] - 1) % 8, (n[1] - 1) % 8, (n[2] - 1) % 8, idx[tuple((v - 1) // 8 + 1 for v in n)]]
    for n in c.fluid:
        assert not at(n), n
    for n in c.filled:
        assert at(n), n
    w = pp.compute_wall_distances(c.coords, got, C.WALL_DX, method=method)
    assert np.array_equal(bits(w), bits(wall))
    for d2 in (2, 3):                                  # this dx tells the written Float32 formula from a Float64 one
        assert np.float32(np.sqrt(np.float64(d2)) * C.WALL_DX) != np.sqrt(np.float32(d2)) * np.float32(C.WALL_DX)
        assert (w == np.sqrt(np.float32(d2)) * np.float32(C.WALL_DX)).any() or name in ("absent_block",)


def _sponge_impl(c):
    params = SimpleNamespace(dx_coarse=c.dx_coarse, domain_size=c.domain_size)
    cfg = SimpleNamespace(sponge_thickness=np.float32(c.thickness), symmetric_analysis=c.symmetric)
    return np.asarray(pp.apply_sponge(c.coords, params, c.lvl_scale, cfg))


@functools.lru_cache(maxsize=None)
def sponge_ref(name):
    c = SPONGE[name]
    v64, b64 = R.sponge(c.coords, c.dx_coarse, c.lvl_scale, c.domain_size, c.thickness, c.symmetric, np.float64)
    vld, _ = R.sponge(c.coords, c.dx_coarse, c.lvl_scale, c.domain_size, c.thickness, c.symmetric, np.longdouble)
    return v64, b64, vld


@pytest.mark.parametrize("name", list(SPONGE))
def test_sponge_equals_the_restatement_bit_for_bit(name):
    v64, _, vld = sponge_ref(name)
    got = _sponge_impl(SPONGE[name])
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(v64.astype(np.float32)))
    ulp = np.spacing(np.maximum(np.abs(v64), np.float64(np.finfo(np.float32).tiny)).astype(np.float32)).astype(np.float64)
    err = float((np.abs(v64.astype(np.longdouble) - vld) / ulp).max())
    print(f"\n{name}: |float64 - longdouble| = {err:.3e} Float32 ulps")
    assert err <= MAX_SPONGE_ULP


def test_sponge_cell_centres_sit_exactly_on_the_thresholds():
    """all six comparisons are strict: a centre ON outlet_start, inlet_thickness, the y or z start is outside that layer. (The value
    cannot tell: entered at equality, the profile would return 0.0 through its `x >= thickness` arm; only the branch record differs.)"""
    for name, axis, cell, thr in (("sponge_on_centres", 0, 23, 3.75 - 3.75 * 0.25), ("sponge_inlet_on_centre", 0, 1, 3.125 * 0.02),
                                  ("sponge_on_centres", 1, 2, 1.5 * 0.25 * 0.5), ("sponge_on_centres", 1, 11, 1.5 - 1.5 * 0.25 * 0.5),
                                  ("sponge_on_centres", 2, 2, 0.1875), ("sponge_on_centres", 2, 11, 1.3125)):
        c = SPONGE[name]
        assert (cell - 0.5) * c.dx_coarse == thr, (name, axis, cell)
        # the cell in the middle of the other two axes, where no other layer reaches: on the threshold the value is exactly zero
        n = [12, 8, 8]
        n[axis] = cell
        v, b = R.sponge_value(*[(i - 0.5) * c.dx_coarse for i in n], *c.domain_size, c.thickness, c.symmetric)
        assert v == 0.0 and b == 0, (name, axis, cell, v, b)
        got = _sponge_impl(c)
        assert got[(n[0] - 1) % 8, (n[1] - 1) % 8, (n[2] - 1) % 8, (n[0] - 1) // 8 + 4 * ((n[1] - 1) // 8) + 8 * ((n[2] - 1) // 8)] == 0.0


# ----------------------------------------------------------------------------------------------------------------
# by hand
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, c in MESH.items() if c.by_hand])
def test_by_hand_expectations(name):
    c, h = MESH[name], MESH[name].by_hand
    views = [("restatement", ref(name).obstacle, ref(name).fill, ref(name).wall, ref(name).q.q16, ref(name).q.cells)]
    for m in METHODS:
        g = impl(name, m)
        views.append((m, g.obstacle, g.fill, g.wall, g.q16, g.cells))
    for who, obstacle, fill, wall, q16, cells in views:
        if "fill" in h:
            assert fill == h["fill"], who
        if "n_obstacle_after_fill" in h:
            assert int(obstacle.sum()) == h["n_obstacle_after_fill"], who
        for (cell, k), q in h.get("q", {}).items():
            assert bits(q16[cell + (k,)][None])[0] == bits(np.float16(q)[None])[0], (who, cell, k, float(q16[cell + (k,)]), q)
        for cell, listed in h.get("listed", []):
            assert ((cell[3] + 1, cell[0] + 1, cell[1] + 1, cell[2] + 1) in cells) == listed, (who, cell)
        for cell, solid in h.get("solid", []):
            assert bool(obstacle[cell]) == solid, (who, cell)
        for cell, d2 in h.get("wall", {}).items():
            want = np.float32(100.0) if d2 == 0 else np.sqrt(np.float32(d2)) * np.float32(c.dx)
            assert wall[cell] == want, (who, cell, wall[cell], want)


def test_planted_heights_sit_on_the_side_of_epsilon_the_table_says():
    """t = centre - (0 + offset) in the written float64 order, against EPSILON = 1e-9"""
    for name, above in (("height_below_epsilon", False), ("height_above_epsilon", True), ("height_rounds_to_zero", True)):
        c = MESH[name]
        t = (6 - 0.5) * c.dx - (c.tri[0, 0, 2] + c.offset[2])
        assert (t > R.EPSILON) == above and t > 0.0, (name, t)
    r = ref("height_rounds_to_zero").q
    row = r.q64[5, 5, 5, 0]
    assert (row > 0).sum() == 9 and (row[row > 0] < 2.0 ** -25).all() and not r.q16[5, 5, 5, 0].any() and r.listed[5, 5, 5, 0]


def test_slivers_are_slivers_and_not_points():
    """the two slivers of edge_triangles survive Float32: distinct corners, every |a| and every cross axis non-zero AND under its threshold"""
    c = MESH["edge_triangles"]
    v = c.tri + c.offset
    for i in C.SLIVERS:
        t = v[i]
        assert all(not np.array_equal(t[a], t[b]) for a, b in ((0, 1), (1, 2), (2, 0)))
        e1, e2 = tuple(t[1] - t[0]), tuple(t[2] - t[0])
        for k, d in enumerate(R.DIRS):
            if k != 13:
                dn = tuple(np.array(d, dtype=np.float64) / np.sqrt(float(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])))
                a = R._dot(e1, R._cross(dn, e2))
                assert 0.0 < abs(a) < R.EPSILON, (i, d, a)
        for f in (t[1] - t[0], t[2] - t[1], t[0] - t[2]):          # the same edges up to the centre's cancelling shift
            for u in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)):
                ax = R._cross(u, tuple(f))
                assert 0.0 < R._dot(ax, ax) < R.SAT_SKIP, (i, u, ax)
    # the first lies outside the box of cell (19, 6, 6) by more than a Float32 ulp of its coordinates, its bounding box inside by as much
    t = v[C.SLIVERS[0]]
    h = 0.75 * c.dx * R.SAT_TOL
    corner = ((19 - 0.5) * c.dx + h, (6 - 0.5) * c.dx + h)
    assert ((t[:, 0] - corner[0]) + (t[:, 1] - corner[1])).min() > 1.0e-6 and t[:, 0].min() < corner[0] - 1.0e-6 and t[:, 1].min() < corner[1] - 1.0e-6
    # the second holds the -z link line of cell (6, 18, 18) well inside: barycentric coordinates of the centre's foot all above 0.2
    t = v[C.SLIVERS[1]]
    p = np.array([5.5 * c.dx, 17.5 * c.dx])
    m = np.array([[t[1, 0] - t[0, 0], t[2, 0] - t[0, 0]], [t[1, 1] - t[0, 1], t[2, 1] - t[0, 1]]])
    uv = np.linalg.solve(m, p - t[0, :2])
    assert uv.min() > 0.2 and uv.sum() < 0.8 and 0.3 * c.dx < 17.5 * c.dx - t[:, 2].max() < 0.5 * c.dx


def test_box_at_dx_002_sits_on_the_knife_edges():
    """box_002 has no by-hand table (dx = 0.02 is not dyadic); what makes it the cube fixture's kind of case is asserted here: thousands of
    links whose Float64 q lies within 1e-12 of the branch boundary 0.5 and of the inclusion boundary 1.0, kept and rounded onto them"""
    r = ref("box_002").q
    q64, q16 = r.q64, np.asarray(r.q16)
    for thr in (0.5, 1.0):
        near = np.abs(q64 - thr) < 1e-12               # the x faces (Float32-exact corners); the y and z faces are 2.4e-7 off
        assert near.sum() > 1000, (thr, int(near.sum()))
        assert (q16[near] == np.float16(thr)).all() and (q64[near] != thr).any()      # on the edge by the last bits, not exactly
    assert (q64 <= 1.0).all()
    for m in METHODS:
        assert np.array_equal(bits(impl("box_002", m).q16), bits(q16))


def test_exact_arm_gives_the_dyadic_box_its_by_hand_values_exactly():
    c = MESH["box_dyadic"]
    n, _ = R.cell_index(c.coords)
    flat = lambda cell: cell[3] * 512 + cell[2] * 64 + cell[1] * 8 + cell[0]
    want = {(flat(cell), k): q for (cell, k), q in c.by_hand["q"].items()}
    ex = R.exact_qmap(c.coords, c.tri, c.dx, c.offset, cells={i for i, _ in want})
    for key, q in want.items():
        got = ex.get(key)
        if q == 0.0:
            assert got is None or got.q is None, key
        else:
            assert got is not None and got.q == Fraction(q), (key, got)
            if q == 1.0:
                assert not got.robust                # the inclusion boundary itself: a planted knife-edge, judged by hand only


# ----------------------------------------------------------------------------------------------------------------
# the restatement against the exact arm
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact(name):
    c = MESH[name]
    return R.exact_voxels(c.coords, c.tri, c.dx, c.offset), R.exact_qmap(c.coords, c.tri, c.dx, c.offset)


@pytest.mark.parametrize("name", NON_PLANTED)
def test_restatement_against_exact_geometry(name):
    r = ref(name)
    vox, links = exact(name)
    # voxels
    shell_cells = int(r.shell.sum())
    wrong = (r.shell != vox.shell) & ~vox.borderline
    assert not wrong.any(), f"{int(wrong.sum())} voxel decisions differ from the exact ones away from every threshold"
    vox_share = float(vox.borderline.sum()) / shell_cells
    # links
    q64 = r.q.q64.transpose(3, 2, 1, 0, 4).reshape(-1, 27)
    q16 = np.asarray(r.q.q16).transpose(3, 2, 1, 0, 4).reshape(-1, 27)
    cut = int((q64 > 0).sum())
    excluded, e_ref = 0, 0.0
    seen = set()
    for (i, k), ln in links.items():
        tie = False
        if ln.q is not None:
            want16, tie = R.round_to_f16(ln.q)
        if not ln.robust or tie:
            excluded += 1
            continue
        seen.add((i, k))
        assert ln.q is not None and q64[i, k] > 0, (i, k, ln.q, q64[i, k])
        e_ref = max(e_ref, abs(float(Fraction(float(q64[i, k])) - ln.q)))
        assert bits(q16[i, k][None])[0] == bits(want16[None])[0], (i, k, float(ln.q), q16[i, k], want16)
    # a link the restatement holds and the exact arm does not know at all is a defect (one it knows as borderline was counted)
    for i, k in np.argwhere(q64 > 0):
        assert (int(i), int(k)) in links, (i, k, q64[i, k])
    share = excluded / max(1, cut)
    print(f"\n{name}: cut links {cut}, compared {len(seen)}, excluded {excluded} ({share:.4%}); shell cells {shell_cells}, borderline "
          f"{int(vox.borderline.sum())} ({vox_share:.4%}); e_ref {e_ref:.3e}")
    assert len(seen) > 0.9 * cut
    assert share <= MAX_EXCLUDED_SHARE and vox_share <= MAX_EXCLUDED_SHARE
    assert e_ref <= MAX_E_REF_Q


def test_float16_rounding_of_a_fraction():
    for x, want in ((Fraction(1, 2), 0.5), (Fraction(1), 1.0), (Fraction(1, 3), np.float16(1 / 3)), (Fraction(2049, 4096), 0.5),
                    (Fraction(2051, 4096), 0.50098), (Fraction(1, 2 ** 25), 0.0), (Fraction(3, 2 ** 26), 2.0 ** -24), (Fraction(1, 10 ** 7), 1e-7)):
        got, _ = R.round_to_f16(x)
        assert got == np.float16(want), (x, got, want)
    assert R.round_to_f16(Fraction(2049, 4096))[1] and not R.round_to_f16(Fraction(1, 3))[1]


# ----------------------------------------------------------------------------------------------------------------
# census: what the cases reach
# ----------------------------------------------------------------------------------------------------------------
def test_census():
    tot = dict.fromkeys(("q_lt_half", "q_half", "q_gt_half", "q_one", "both_cut", "listed_solid", "behind_solid", "behind_absent", "behind_listed",
                         "wall_1", "wall_2", "wall_3", "wall_skipped_interior_absent_block", "sat_skipped", "sat_skipped_nonzero_axis"), 0)
    exits = np.zeros(R.SAT_EXITS, dtype=np.int64)
    for name, c in MESH.items():
        r = ref(name)
        q = r.q.q64
        tot["q_lt_half"] += int(((q > 0) & (q < 0.5)).sum())
        tot["q_half"] += int((q == 0.5).sum())
        tot["q_gt_half"] += int(((q > 0.5) & (q < 1)).sum())
        tot["q_one"] += int((q == 1.0).sum())
        tot["both_cut"] += int(sum(((q[..., k] > 0) & (q[..., R.OPP[k]] > 0)).sum() for k in range(13)))
        tot["listed_solid"] += int((r.q.listed & r.obstacle).sum())
        n, blk = R.cell_index(c.coords)
        look = R._Lookup(n)
        solid = r.obstacle.transpose(3, 2, 1, 0).reshape(-1)
        listed = r.q.listed.transpose(3, 2, 1, 0).reshape(-1)
        qf = q.transpose(3, 2, 1, 0, 4).reshape(-1, 27)
        for k, d in enumerate(R.DIRS):
            if k == 13:
                continue
            cutk = np.flatnonzero(qf[:, k] > 0)
            j = look.find(n[cutk] - np.asarray(d))                # the cell behind the link
            tot["behind_absent"] += int((j < 0).sum())
            tot["behind_solid"] += int(solid[j[j >= 0]].sum())
            tot["behind_listed"] += int(listed[j[j >= 0]].sum())
        for k2 in (1, 2, 3):
            tot[f"wall_{k2}"] += r.wall_census.nearest[k2]
        exits += r.sat.exits
        tot["sat_skipped"] += r.sat.skipped
        tot["sat_skipped_nonzero_axis"] += r.sat.skipped_nonzero
    for name, c in SHELL.items():
        if name == "absent_block":
            # the only level with a block missing between two others: neighbours that land in block (2, 1, 1), cells 9..16 x 1..8 x 1..8
            tot["wall_skipped_interior_absent_block"] += R.wall_distance(c.coords, R.flood_fill(c.coords, c.shell)[0], C.WALL_DX,
                                                                         absent_box=((9, 1, 1), (16, 8, 8)))[1].skipped_in_box
    print("\ncensus:", tot, "SAT exits:", exits.tolist())
    assert all(v > 0 for v in tot.values()), tot
    assert (exits > 0).all(), exits
    taken = np.zeros(9, dtype=np.int64)
    not_taken = np.zeros(6, dtype=np.int64)
    for name in SPONGE:
        b = sponge_ref(name)[1]
        for i in range(9):
            taken[i] += int(((b >> i) & 1).sum())
        for i in range(6):
            not_taken[i] += int((((b >> i) & 1) == 0).sum())
    print("sponge branches taken:", taken.tolist(), "layers not entered:", not_taken.tolist())
    # the profile's `x >= thickness` arm cannot be reached from apply_sponge!: each call sits behind a strict comparison that excludes it
    assert taken[7] == 0 and (np.delete(taken, 7) > 0).all() and (not_taken > 0).all()


# ----------------------------------------------------------------------------------------------------------------
# STL parsing
# ----------------------------------------------------------------------------------------------------------------
def test_binary_and_ascii_stl_load_to_the_same_triangles(tmp_path):
    c = MESH["icosphere80"]
    C.write_binary_stl(tmp_path / "b.stl", c.tri)
    C.write_ascii_stl(tmp_path / "a.stl", c.tri)
    for scale in (1.0, 0.001):
        b, a = pp.load_mesh(str(tmp_path / "b.stl"), scale), pp.load_mesh(str(tmp_path / "a.stl"), scale)
        assert b.triangles.dtype == np.float64 and np.array_equal(b.triangles, a.triangles)
        assert np.array_equal(b.triangles, c.tri.astype(np.float32).astype(np.float64) * scale)
        assert np.array_equal(b.min_bounds, a.min_bounds) and np.array_equal(b.max_bounds, a.max_bounds)
    # through the files: the same q-map as from the arrays
    m = pp.load_mesh(str(tmp_path / "a.stl"), 1.0)
    q = pp.compute_bouzidi_qmap_sparse(c.coords, m, c.dx, c.offset)[0]
    assert np.array_equal(bits(q), bits(ref("icosphere80").q.q16))
