"""Iso-surfaces, host side: the numpy restatement of the definition (isosurface.extract_host - the checker the device is compared with),
welding, the configuration keys, the PolyData writer and the bindings. No GPU."""
import copy
import os
import re

import numpy as np
import pytest

import _iso_cases as ic
from open_ludwig_amd import _lib, case, isosurface as iso, output, preprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
F32 = np.float32


def _extract(s, nt, coords, value, rho, vel, obstacle=None, skip=None, box=ic.BOX):
    ob = np.zeros(s.shape, bool) if obstacle is None else obstacle
    return iso.extract_host(s, ob, nt, skip, box[0], box[1], value, rho, vel, coords)


def test_case_table_is_wound_from_inside_to_outside_and_complements_reverse():
    """the 16-case table against float geometry on the unit tetrahedron of positive orientation, every case with generic edge
    parameters"""
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    assert np.linalg.det(V[1:] - V[0]) > 0
    C = np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)], float)
    for t in iso.KUHN_TETS:                                               # every tetrahedron of the split has that orientation
        assert np.linalg.det(C[t[1:]] - C[t[0]]) > 0
    rng = np.random.default_rng(3)
    for m in range(16):
        tris = iso.CASE_TRIANGLES[m]
        inside = [k for k in range(4) if (m >> k) & 1]
        n = sum(t[0] >= 0 for t in tris)
        assert n == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[len(inside)]
        assert (tris[0][0] >= 0) or n == 0                                # the first slot is filled first
        if n == 0:
            continue
        outside = [k for k in range(4) if k not in inside]
        tt = rng.uniform(0.2, 0.8, 6)
        P = lambda e: V[iso.TET_EDGES[e, 0]] + tt[e] * (V[iso.TET_EDGES[e, 1]] - V[iso.TET_EDGES[e, 0]])
        for t in tris[:n]:
            for e in t:                                                   # every vertex sits on a cut edge
                assert ((iso.TET_EDGES[e, 0] in inside) != (iso.TET_EDGES[e, 1] in inside))
            nrm = np.cross(P(t[1]) - P(t[0]), P(t[2]) - P(t[0]))
            assert nrm @ (V[outside].mean(0) - V[inside].mean(0)) > 0, m
        # the complement is the same surface with the other side out: the same triangles reversed (up to a rotation of each)
        canon = lambda t: min(tuple(t[i:] + t[:i]) for i in range(3))
        assert sorted(canon(t) for t in iso.CASE_TRIANGLES[15 - m][:n].tolist()) == sorted(canon(t[::-1]) for t in tris[:n].tolist())


@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_sphere_is_closed_oriented_and_close_to_the_sphere(sign):
    """the bounds are derived in _iso_cases.check_sphere's source: interpolation error 3 h^2 / (8 r) and inscribed facets"""
    coords, nt, s, rho, vel = ic.sphere(sign)
    pos, att, keys = _extract(s, nt, coords, sign * ic.SPHERE_R, rho, vel)
    assert pos.shape == (11252, 3, 3) and att.shape == (11252, 3, 4) and keys.shape == (11252, 3, 2)
    assert pos.dtype == F32 and att.dtype == F32 and keys.dtype == np.int32
    ic.check_sphere(pos, keys, outward=sign < 0)
    # every vertex lies between its two cells, and a welded vertex has one position and one attribute set
    first, tri = iso.weld(keys)
    p, a = pos.reshape(-1, 3), att.reshape(-1, 4)
    assert np.array_equal(p[first][tri.reshape(-1)], p) and np.array_equal(a[first][tri.reshape(-1)], a)
    r = np.linalg.norm(p.astype(np.float64) - ic.SPHERE_CENTRE, axis=1)
    assert np.abs(r - ic.SPHERE_R).max() < 3 / 80 + 1e-6                  # 3 h^2 / (8 r) at r = 10 h
    # the interpolated rho is the linear field it was sampled from, up to float32
    assert np.abs(a[:, 0] - (1.0 + 0.001 * p[:, 0] - 0.002 * p[:, 2])).max() < 1e-6


def test_order_is_block_cell_tetrahedron():
    coords, nt, s, rho, vel = ic.sphere(-1.0)
    pos, att, keys = _extract(s, nt, coords, -ic.SPHERE_R, rho, vel)
    # the whole surface is the blocks' own surfaces (every other block skipped) one after the other, in the reference block order
    per_block = [len(_extract(s, nt, coords, -ic.SPHERE_R, rho, vel, skip=(np.arange(27) != b).astype(np.uint8))[0]) for b in range(27)]
    assert sum(per_block) == len(pos)
    start = 0
    for b, n in enumerate(per_block):
        one = _extract(s, nt, coords, -ic.SPHERE_R, rho, vel, skip=(np.arange(27) != b).astype(np.uint8))
        ic.assert_same((pos[start:start + n], att[start:start + n], keys[start:start + n]), one)
        start += n
    # within a block the anchors ascend in x + 8 y + 64 z: the cube a triangle lies in is the floor of its lowest corner, except where
    # a vertex sits exactly on a lattice plane, so compare through the centroid
    one = _extract(s, nt, coords, -ic.SPHERE_R, rho, vel, skip=(np.arange(27) != 4).astype(np.uint8))[0]
    a = np.floor(one.mean(axis=1)).astype(int) - (np.asarray(coords[4]) - 1) * 8
    cell = a[:, 0] + 8 * a[:, 1] + 64 * a[:, 2]
    assert (np.diff(cell) >= 0).all() and len(set(cell.tolist())) > 8


def test_a_corner_equal_to_the_value_keeps_the_surface_closed():
    coords, nt, s, rho, vel = ic.sphere(-1.0)
    s = s.copy()
    d = np.abs(s + F32(ic.SPHERE_R))
    hit = np.unravel_index(np.argsort(d, axis=None)[:5], d.shape)           # the five cells nearest to the surface, on either side
    s[hit] = F32(-ic.SPHERE_R)
    pos, att, keys = _extract(s, nt, coords, F32(-ic.SPHERE_R), rho, vel)
    V, E, F, two, once = ic.topology(keys)
    assert two and once and V - E + F == 2
    assert all(len({tuple(k) for k in t}) == 3 for t in keys.tolist())
    # a vertex on an edge that ends in such a cell sits exactly on the cell
    flat = (np.asarray(hit[3]) * 512 + hit[0] + 8 * hit[1] + 64 * hit[2]).tolist()
    on = np.isin(keys[..., 0], flat) | np.isin(keys[..., 1], flat)
    assert on.any()
    p = pos[on]
    assert np.array_equal(p, np.round(p))


def test_liveness_rules():
    coords, nt, s, rho, vel = ic.sphere(-1.0)
    value = -ic.SPHERE_R
    full = _extract(s, nt, coords, value, rho, vel)
    cell_of = lambda idx: idx[3] * 512 + idx[0] + 8 * idx[1] + 64 * idx[2]
    near = np.argwhere(np.abs(s + F32(ic.SPHERE_R)) < 0.4)

    def touched(keys, cell):
        return (keys == cell).any()

    # an obstacle cell, a NaN, an Inf: no triangle has a corner there, and the hole is bounded by the cubes that held it
    for k, plant in enumerate(("obstacle", "nan", "inf", "-inf")):
        idx = tuple(near[7 + 31 * k])
        assert touched(full[2], cell_of(idx))
        ob = np.zeros(s.shape, bool)
        s2 = s.copy()
        if plant == "obstacle":
            ob[idx] = True
        else:
            s2[idx] = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf}[plant]
        pos, att, keys = _extract(s2, nt, coords, value, rho, vel, obstacle=ob)
        assert not touched(keys, cell_of(idx)) and 0 < len(pos) < len(full[0])
        assert np.isfinite(pos).all() and np.isfinite(att).all()
    # a missing block: nothing is anchored in it, nothing reaches into it
    keep = [i for i in range(27) if i != 4]
    coords2 = [coords[i] for i in keep]
    from open_ludwig_amd.blocks import build_neighbor_table
    nt2 = build_neighbor_table(coords2, 3, 3, 3)
    pos, att, keys = _extract(s[:, :, :, keep], nt2, coords2, value, rho[:, :, :, keep], vel[:, :, :, keep])
    assert 0 < len(pos) < len(full[0])
    gone = np.asarray(coords[4])
    lo, hi = (gone - 1) * 8, gone * 8 - 1
    inside_gone = ((pos > lo) & (pos < hi)).all(axis=2)
    assert not inside_gone.any()
    # a skipped block anchors nothing; its cells still serve as corners of its neighbours' cubes
    skip = np.zeros(27, np.uint8)
    skip[4] = 1
    pos, att, keys = _extract(s, nt, coords, value, rho, vel, skip=skip)
    assert 0 < len(pos) < len(full[0]) and (keys // 512 == 4).any()
    # the box: every triangle lies in the cubes anchored in [lo, hi)
    lo, hi = np.array([3, 0, 5], np.int32), np.array([20, 11, 24], np.int32)
    pos, att, keys = _extract(s, nt, coords, value, rho, vel, box=(lo, hi))
    assert 0 < len(pos) < len(full[0])
    assert (pos.min(axis=1) >= lo).all() and (pos.max(axis=1) <= hi).all()
    assert len(_extract(s, nt, coords, value, rho, vel, box=(lo, lo))[0]) == 0
    # n_owned: ghost blocks anchor nothing
    got = iso.extract_host(s, np.zeros(s.shape, bool), nt, None, *ic.BOX, value, rho, vel, coords, n_owned=9)
    only = _extract(s, nt, coords, value, rho, vel, skip=(np.arange(27) >= 9).astype(np.uint8))
    ic.assert_same(got, only)


def test_periodic_neighbours_continue_the_surface_unwrapped():
    coords, nt = ic.block_grid(2, 1, 1, periodic=(True, False, False))
    x = ic.cell_centres(coords)
    s = np.asfortranarray(np.sin(2 * np.pi * (x[..., 0] - 15.4) / 16).astype(F32))          # periodic over the 16 cells
    rho = np.ones(s.shape, F32, order="F")
    vel = np.zeros(s.shape + (3,), F32, order="F")
    pos, att, keys = _extract(s, nt, coords, F32(0.05), rho, vel)
    assert pos[..., 0].max() > 15 and pos[..., 0].max() <= 16                # the cube anchored at x = 15 reaches x = 16, not 0
    assert (keys[pos[..., 0] > 15][:, 1] // 512 == 0).all()                 # its far corners are cells of block 0


def test_weld_and_to_domain():
    keys = np.array([[[5, 9], [1, 2], [5, 7]], [[1, 2], [5, 9], [0, 3]]], np.int32)
    first, tri = iso.weld(keys)
    assert first.tolist() == [5, 1, 2, 0] and tri.tolist() == [[3, 1, 2], [1, 3, 0]]
    big = np.array([[[2 ** 31 - 1, 0], [2 ** 31 - 1, 1], [0, 2 ** 31 - 1]]], np.int32)
    assert len(iso.weld(big)[0]) == 3
    assert iso.weld(np.zeros((0, 3, 2), np.int32))[1].shape == (0, 3)
    p = iso.to_domain(np.array([[0.0, 1.5, 7.25]], F32), 0.1)
    assert p.dtype == F32 and np.array_equal(p, np.array([[0.05, 0.2, 0.775]]).astype(F32))


def test_cell_box_and_skip_flags():
    lo, hi = iso.cell_box(None, 0.5)
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [iso.CELL_MAX] * 3 and lo.dtype == np.int32
    # cells of size 0.5 with centres 0.25, 0.75, ...: [1.0, 2.5) + 1 holds the centres 2.25 .. 3.25 = cells 4, 5, 6
    lo, hi = iso.cell_box([[1.0, 2.5], [-9.0, 0.26], [0.25, 0.75]], 0.5, (1.0, 0.0, 0.0))
    assert lo.tolist() == [4, 0, 0] and hi.tolist() == [7, 1, 1]
    grids = pp.setup_multilevel_domain(pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"),
                                                                  {"basic": {"num_levels": 3, "surface_resolution": 14}}),
                                       os.path.join(G, "cube1m.stl"))[0]
    skips = iso.skip_flags(grids)
    sel = output.select_export_blocks([g.active_block_coords for g in grids])
    assert [int((s == 0).sum()) for s in skips] == [sum(1 for l, _ in sel if l == i) for i in range(len(grids))] == [380, 1568]


CFG = os.path.join(G, "cube1m_config.yaml")
ONE = {"name": "q", "field": "q_criterion", "value": 0.5}


def _load(iso_cfg):
    return pp.load_case_configuration(CFG, {"advanced": {"isosurfaces": iso_cfg}})


def test_configuration_defaults_and_parsing():
    for name in ("ball1m_config.yaml", "cube1m_config.yaml", "bunny_config.yaml"):
        cfg = pp.load_case_configuration(os.path.join(G, name))
        assert not cfg.isosurfaces_enabled and cfg.isosurfaces_surfaces == () and cfg.isosurfaces_max_triangles == 50_000_000
    assert not _load({"enabled": False, "surfaces": [{"name": "", "field": "nope"}]}).isosurfaces_enabled
    cfg = _load({"enabled": True, "start_step": 3, "interval": 7, "max_triangles": 1000,
                 "surfaces": [ONE, {"name": "rho-1", "field": "density", "value": 1, "bounds": [[0, 1], [-1, 1], [2, 3.5]]}]})
    assert cfg.isosurfaces_enabled and (cfg.isosurfaces_start_step, cfg.isosurfaces_interval, cfg.isosurfaces_max_triangles) == (3, 7, 1000)
    a, b = cfg.isosurfaces_surfaces
    assert (a.name, a.field, a.value, a.bounds) == ("q", "q_criterion", 0.5, None)
    assert (b.name, b.field, b.value, b.bounds) == ("rho-1", "density", 1.0, ((0.0, 1.0), (-1.0, 1.0), (2.0, 3.5)))
    assert pp.ISOSURFACE_FIELDS == iso.FIELDS == tuple(sorted(_lib.ISO_NAMES, key=_lib.ISO_NAMES.get))


@pytest.mark.parametrize("iso_cfg, key", [
    ({"enabled": True, "surfaces": [{**ONE, "field": "pressure"}]}, "advanced.isosurfaces.surfaces[0].field"),
    ({"enabled": True, "surfaces": [{**ONE, "value": float("nan")}]}, "advanced.isosurfaces.surfaces[0].value"),
    ({"enabled": True, "surfaces": [{**ONE, "value": float("inf")}]}, "advanced.isosurfaces.surfaces[0].value"),
    ({"enabled": True, "surfaces": [{"field": "density", "value": 1.0}]}, "advanced.isosurfaces.surfaces[0].name"),
    ({"enabled": True, "surfaces": [ONE, {**ONE, "value": 2.0}]}, "advanced.isosurfaces.surfaces[1].name"),
    ({"enabled": True, "interval": 0, "surfaces": [ONE]}, "advanced.isosurfaces.interval"),
    ({"enabled": True, "start_step": 0, "surfaces": [ONE]}, "advanced.isosurfaces.start_step"),
    ({"enabled": True, "max_triangles": 0, "surfaces": [ONE]}, "advanced.isosurfaces.max_triangles"),
    ({"enabled": True, "surfaces": []}, "advanced.isosurfaces.surfaces"),
    ({"enabled": True, "surfaces": [{"name": "q", "field": "density"}]}, "advanced.isosurfaces.surfaces[0].value"),
    ({"enabled": True, "surfaces": [{**ONE, "bounds": [[0, 1], [0, 1]]}]}, "advanced.isosurfaces.surfaces[0].bounds"),
    ({"enabled": True, "surfaces": [{**ONE, "bounds": [[0, 1], [0, 1], [2, 1]]}]}, "advanced.isosurfaces.surfaces[0].bounds"),
])
def test_configuration_errors_name_their_key(iso_cfg, key):
    with pytest.raises(ValueError) as e:
        _load(iso_cfg)
    assert key in str(e.value), str(e.value)


def test_write_vtp_round_trip(tmp_path):
    coords, nt, s, rho, vel = ic.sphere(-1.0)
    pos, att, keys = _extract(s, nt, coords, -ic.SPHERE_R, rho, vel)
    half = len(pos) // 2
    surf = iso.merge_levels([(0, 0.25, pos[:half], att[:half], keys[:half]), (1, 0.125, pos[half:], att[half:], keys[half:])])
    assert surf.points.dtype == F32 and surf.triangles.max() == len(surf.points) - 1
    for compress in (True, False):
        path = output.write_vtp(str(tmp_path / f"s{int(compress)}"), surf.points, surf.triangles, surf.rho, surf.vel, surf.level, compress)
        assert path.endswith(".vtp") and not os.path.exists(path + ".part")
        text = open(path).read()
        assert 'type="PolyData"' in text and ("vtkZLibDataCompressor" in text) == compress
        arr = iso.read_vtp(path)
        assert int(arr["NumberOfPoints"]) == len(surf.points) and int(arr["NumberOfPolys"]) == len(pos)
        assert np.array_equal(arr["Points"], surf.points) and arr["Points"].dtype == F32
        assert np.array_equal(arr["connectivity"], surf.triangles.reshape(-1)) and arr["connectivity"].dtype == np.int64
        assert np.array_equal(arr["offsets"], 3 * np.arange(1, len(pos) + 1))
        assert np.array_equal(arr["Density"], surf.rho) and np.array_equal(arr["Velocity"], surf.vel)
        v = surf.vel
        assert np.array_equal(arr["VelocityMagnitude"], np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))
        assert np.array_equal(arr["Level"], np.r_[np.full(half, 1), np.full(len(pos) - half, 2)]) and arr["Level"].dtype == np.int32
    # the triangles the file describes are the extracted ones, in the domain frame of their level
    tri_pts = arr["Points"][arr["connectivity"].reshape(-1, 3)]
    assert np.array_equal(tri_pts[:half], iso.to_domain(pos[:half], 0.25)) and np.array_equal(tri_pts[half:], iso.to_domain(pos[half:], 0.125))
    # an empty surface is a valid file
    e = iso.merge_levels([])
    arr = iso.read_vtp(output.write_vtp(str(tmp_path / "empty"), e.points, e.triangles, e.rho, e.vel, e.level))
    assert int(arr["NumberOfPolys"]) == 0 and arr["Points"].size == 0


def test_run_case_with_a_stepper_without_isosurface_extracts_on_the_host(tmp_path):
    """the CPU oracle behind run_case: files at the sampled steps from extract_host, every other file unchanged"""
    import filecmp
    import _gradient_ref as ref
    from _steppers import OracleStepper
    from oracle import oracle
    oracle.set_num_threads(min(8, os.cpu_count() or 1))

    class GradOracleStepper(OracleStepper):
        def gradient_fields(self, level, vel_name, scale):
            g = self.grids[level]
            return ref.gradient_fields(getattr(g, vel_name), g.neighbor_table, g.obstacle, scale)

    base = {"basic": {"num_levels": 1, "surface_resolution": 7, "simulation": {"steps": 6, "output_freq": 8, "ramp_steps": 4}},
            "advanced": {"boundary": {"method": "bounce_back"}, "high_re": {"wall_model": {"enabled": False}},
                         "numerics": {"c_wale": 0.0, "nu_sgs_background": 0.0}, "diagnostics": {"freq": 4}}}
    surfaces = [{"name": "front", "field": "density", "value": 1.000001}, {"name": "speed", "field": "velocity_magnitude", "value": 1e-4},
                {"name": "huge", "field": "vorticity_magnitude", "value": 1e9}]
    outs, lines = {}, []
    for on in (False, True):
        over = copy.deepcopy(base)
        if on:
            over["advanced"]["isosurfaces"] = {"enabled": True, "start_step": 2, "interval": 3, "surfaces": surfaces}
        cfg = pp.load_case_configuration(CFG, over)
        outs[on] = str(tmp_path / ("on" if on else "off"))
        case.run_case(cfg, GradOracleStepper, stl_path=os.path.join(G, "cube1m.stl"), out_dir=outs[on], log=lines.append)
    new = [f"iso_{s['name']}_{t:06d}.vtp" for s in surfaces for t in (2, 5)] + [f"iso_{s['name']}.pvd" for s in surfaces]
    assert sorted(os.listdir(outs[True])) == sorted(os.listdir(outs[False]) + new)
    for name in os.listdir(outs[False]):
        if name != "convergence.csv":
            assert filecmp.cmp(os.path.join(outs[False], name), os.path.join(outs[True], name), shallow=False), name
    front = iso.read_vtp(os.path.join(outs[True], "iso_front_000005.vtp"))
    assert int(front["NumberOfPolys"]) > 0 and set(front["Level"].tolist()) == {1}
    assert np.abs(front["Density"] - 1.000001).max() < 1e-6                 # interpolated to the value it was cut at
    assert int(iso.read_vtp(os.path.join(outs[True], "iso_speed_000002.vtp"))["NumberOfPolys"]) > 0
    assert int(iso.read_vtp(os.path.join(outs[True], "iso_huge_000005.vtp"))["NumberOfPolys"]) == 0


def test_distributed_stepper_refuses_and_names_the_key():
    st = object.__new__(case.DistributedStepper)                           # the refusal needs no device and no process group
    with pytest.raises(RuntimeError, match=r"advanced\.isosurfaces"):
        st.isosurfaces_setup(1, 1)
    cfg = pp.load_case_configuration(CFG, {"basic": {"num_levels": 1, "surface_resolution": 7},
                                           "advanced": {"isosurfaces": {"enabled": True, "surfaces": [ONE]}}})
    closed = []

    class Refusing:
        def __init__(self, grids):
            pass

        isosurfaces_setup = case.DistributedStepper.isosurfaces_setup

        def close(self):
            closed.append(True)
    with pytest.raises(RuntimeError, match=r"advanced\.isosurfaces"):
        case.run_case(cfg, Refusing, stl_path=os.path.join(G, "cube1m.stl"), steps=1)
    assert closed == [True]


def test_header_exports_and_julia_list_the_isosurface_calls():
    new = ["ludwig_level_isosurface_extract", "ludwig_level_isosurface_download"]
    header = open(os.path.join(ROOT, "include", "ludwig_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "LudwigHIP.jl")).read()
    lib = _lib.load()
    for name in new:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert f"(:{name}, LIB)" in jl, name
    assert lib.ludwig_abi_version() == 1
    assert re.search(r"#define\s+LUDWIG_ISO_REFUSED\s+1\b", header) and _lib.ISO_REFUSED == 1
    for name, k in _lib.ISO_NAMES.items():
        assert re.search(r"LUDWIG_ISO_" + name.upper() + r"\s*=\s*%d\b" % k, header), name
    # the device's case table is the restatement's, packed: bits 18.. the count, 3 bits per vertex
    src = open(os.path.join(ROOT, "open_ludwig_amd", "csrc", "kernels.hpp")).read()
    words = [int(w, 16) for w in re.search(r"cases\[16\] = \{([^}]*)\}", src).group(1).replace("\n", " ").split(",")]
    for m, w in enumerate(words):
        tris = [t for t in iso.CASE_TRIANGLES[m].tolist() if t[0] >= 0]
        assert w >> 18 == len(tris)
        assert [(w >> (3 * q)) & 7 for q in range(3 * len(tris))] == [e for t in tris for e in t], m


def test_calls_reject_bad_arguments_without_a_device():
    import ctypes as C
    lib = _lib.load()
    n = C.c_int64(7)
    lo = np.zeros(3, np.int32)
    assert lib.ludwig_level_isosurface_extract(None, 0, _lib.VEL, 1.0, 0.5, None, lo.ctypes.data, lo.ctypes.data, 10, C.byref(n)) == -1
    assert lib.ludwig_level_isosurface_download(None, None, 0, None, 0, None, 0) == -1
    assert b"null" in lib.ludwig_last_error()
