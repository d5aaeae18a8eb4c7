"""Host side of the velocity-gradient fields: the float32 restatement (_gradient_ref), the output_fields keys, the derived arrays of
the flow VTU, and the argument checks of the two C entry points (no device needed)."""
import glob
import os
import re

import numpy as np
import pytest
import yaml

import _gradient_ref as ref
from open_ludwig_amd import _lib, cases, output, preprocess as pp
from test_gpu_statistics import read_vtu_with_field_data

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


def _box(dims=(3, 2, 2), periodic=(False, False, False)):
    return cases.make_level(1, cases.full_box_coords(*dims), dims, 0.51, periodic=periodic, temporal=False)


def _linear(level, A):
    """u_i = sum_j A_ij x_j at the 0-based global cell position: exact in float32 for the small dyadic A used here"""
    gx, gy, gz = cases.global_cell_coords(level)
    x = [gx - 1, gy - 1, gz - 1]
    return np.stack([sum(A[i][j] * x[j] for j in range(3)) for i in range(3)], axis=-1).astype(F32)


A = np.array([[0.25, -0.5, 0.125], [0.75, -0.375, 1.0], [-0.625, 0.5, 0.125]])


def test_linear_field_gives_its_matrix_where_all_face_neighbours_exist():
    lvl = _box()
    u = _linear(lvl, A)
    scale = F32(0.5)
    g = ref.gradient_tensor(u, lvl.neighbor_table, scale)
    gx, gy, gz = cases.global_cell_coords(lvl)
    n = (3 * 8, 2 * 8, 2 * 8)
    inner = (gx > 1) & (gx < n[0]) & (gy > 1) & (gy < n[1]) & (gz > 1) & (gz < n[2])
    for i in range(3):
        for j in range(3):
            assert g[i][j].dtype == F32
            assert np.array_equal(g[i][j][inner], np.full(inner.sum(), A[i, j] * 0.5, F32)), (i, j)
    w, q = ref.gradient_fields(u, lvl.neighbor_table, np.zeros(gx.shape, bool), scale)
    As = A * 0.5
    want_w = [As[2, 1] - As[1, 2], As[0, 2] - As[2, 0], As[1, 0] - As[0, 1]]
    for k in range(3):
        assert np.allclose(w[..., k][inner], want_w[k], rtol=0, atol=1e-6)
    assert np.allclose(q[inner], -0.5 * np.trace(As @ As), rtol=1e-6, atol=1e-7)
    # and Q is (|Omega|^2 - |S|^2) / 2
    S, W = 0.5 * (As + As.T), 0.5 * (As - As.T)
    assert np.isclose(-0.5 * np.trace(As @ As), 0.5 * ((W * W).sum() - (S * S).sum()))


def test_missing_face_neighbour_uses_the_own_value():
    """at the domain edge the stencil's outer value is the cell itself: a one-sided half difference"""
    lvl = _box()
    u = _linear(lvl, A)
    g = ref.gradient_tensor(u, lvl.neighbor_table, F32(1.0))
    gx, gy, gz = cases.global_cell_coords(lvl)
    lo_x = (gx == 1) & (gy > 1) & (gy < 16) & (gz > 1) & (gz < 16)
    hi_z = (gz == 16) & (gx > 1) & (gx < 24) & (gy > 1) & (gy < 16)
    for i in range(3):
        assert np.array_equal(g[i][0][lo_x], np.full(lo_x.sum(), F32(0.5 * A[i, 0]))), i
        assert np.array_equal(g[i][1][lo_x], np.full(lo_x.sum(), F32(A[i, 1]))), i
        assert np.array_equal(g[i][2][hi_z], np.full(hi_z.sum(), F32(0.5 * A[i, 2]))), i


def test_periodic_box_has_no_edge():
    lvl = _box((2, 2, 2), periodic=(True, True, True))
    gx, gy, gz = cases.global_cell_coords(lvl)
    k = 2 * np.pi / 16
    u = np.stack([np.sin(k * (gy - 1)), np.zeros(gx.shape), np.zeros(gx.shape)], axis=-1).astype(F32)
    g = ref.gradient_tensor(u, lvl.neighbor_table, F32(1.0))
    # du_x/dy = 0.5 (sin(k(y+1)) - sin(k(y-1))) wrapped, everywhere - no one-sided value at the box faces
    ywrap = lambda d: np.sin(k * ((gy - 1 + d) % 16)).astype(F32)
    assert np.array_equal(g[0][1], (F32(0.5) * (ywrap(1) - ywrap(-1))) * F32(1.0))


def test_restatement_equals_the_literal_neighbour_rule():
    """the vectorised halo against get_velocity_neighbor cell by cell, on random values and a table with holes"""
    rng = np.random.default_rng(5)
    coords = [c for c in cases.full_box_coords(3, 3, 2) if c not in ((2, 2, 1), (3, 1, 2))]     # interior holes
    lvl = cases.make_level(1, coords, (3, 3, 2), 0.51, temporal=False)
    nb = lvl.n_blocks
    u = rng.standard_normal((8, 8, 8, nb, 3)).astype(F32)
    obst = rng.random((8, 8, 8, nb)) < 0.1
    scale = F32(1.0 / 0.37)
    w, q = ref.gradient_fields(u, lvl.neighbor_table, obst, scale)
    for b in range(nb):
        for (x, y, z) in [(0, 0, 0), (7, 3, 5), (4, 7, 0), (2, 5, 7), (7, 7, 7), (3, 4, 4)]:
            nv = lambda d: ref.neighbor_value(u, lvl.neighbor_table, x, y, z, b, *d)
            e = np.eye(3, dtype=int)
            g = [[(F32(0.5) * (nv(e[j])[i] - nv(-e[j])[i])) * scale for j in range(3)] for i in range(3)]
            if obst[x, y, z, b]:
                want_w, want_q = [F32(0)] * 3, F32(0)
            else:
                want_w = [g[2][1] - g[1][2], g[0][2] - g[2][0], g[1][0] - g[0][1]]
                want_q = F32(-0.5) * (((g[0][0] * g[0][0] + g[1][1] * g[1][1]) + g[2][2] * g[2][2])
                                      + F32(2.0) * ((g[0][1] * g[1][0] + g[0][2] * g[2][0]) + g[1][2] * g[2][1]))
            assert [w[x, y, z, b, k] for k in range(3)] == want_w, (b, x, y, z)
            assert q[x, y, z, b] == want_q, (b, x, y, z)


def test_obstacle_cells_are_zero():
    lvl = _box()
    u = _linear(lvl, A)
    obst = np.zeros((8, 8, 8, lvl.n_blocks), bool)
    obst[2:5, 3, 4, 1] = True
    w, q = ref.gradient_fields(u, lvl.neighbor_table, obst, F32(1.0))
    assert not w[obst].any() and not q[obst].any()
    assert np.abs(w[~obst]).max() > 0 and np.abs(q[~obst]).max() > 0 and w.dtype == F32 and q.dtype == F32


# ---- configuration ----
def _golden_configs():
    paths = sorted(glob.glob(os.path.join(G, "*_config.yaml")))
    assert len(paths) >= 4
    return paths


def _old_output_fields(path):
    """the rule before the derived arrays existed: the five reference arrays, each on unless its key says false"""
    of = yaml.safe_load(open(path))["basic"]["simulation"].get("output_fields", {}) or {}
    return tuple(n for k, n in (("density", "Density"), ("velocity", "Velocity"), ("velocity_magnitude", "VelocityMagnitude"),
                                ("obstacle", "Obstacle"), ("level", "Level")) if bool(of.get(k, True)))


def test_golden_configs_keep_their_output_fields():
    for p in _golden_configs():
        cfg = pp.load_case_configuration(p)
        assert cfg.output_fields == _old_output_fields(p), p
        assert "Vorticity" not in cfg.output_fields and "QCriterion" not in cfg.output_fields


def test_gradient_keys_add_names_in_order_and_nothing_else_moves(tmp_path):
    p = os.path.join(G, "ball1m_config.yaml")
    base = pp.load_case_configuration(p)
    of = lambda **kw: {"basic": {"simulation": {"output_fields": kw}}}
    both = pp.load_case_configuration(p, of(vorticity=True, q_criterion=True))
    assert both.output_fields == base.output_fields + ("Vorticity", "QCriterion")
    assert pp.load_case_configuration(p, of(vorticity=True)).output_fields == base.output_fields + ("Vorticity",)
    assert pp.load_case_configuration(p, of(q_criterion=True)).output_fields == base.output_fields + ("QCriterion",)
    for name in base.__dataclass_fields__:
        if name != "output_fields":
            assert repr(getattr(both, name)) == repr(getattr(base, name)), name
    # both keys absent: off (the reference's loader defaults vorticity to true, but never writes it)
    d = yaml.safe_load(open(p))
    del d["basic"]["simulation"]["output_fields"]["vorticity"]
    q = tmp_path / "no_vorticity_key.yaml"
    q.write_text(yaml.safe_dump(d))
    assert pp.load_case_configuration(str(q)).output_fields == base.output_fields


# ---- the flow VTU ----
def _levels_and_fields():
    grids, _ = cases.tunnel_with_sphere((4, 2, 2), levels=2)
    rng = np.random.default_rng(9)
    state = {}
    for lvl, g in enumerate(grids):
        sh = (8, 8, 8, g.n_blocks)
        state[lvl] = {"rho": np.asfortranarray(rng.standard_normal(sh).astype(F32)),
                      "vel": np.asfortranarray(rng.standard_normal(sh + (3,)).astype(F32)),
                      "vel_temp": np.asfortranarray(rng.standard_normal(sh + (3,)).astype(F32)),
                      "w": np.asfortranarray(rng.standard_normal(sh + (3,)).astype(F32)),
                      "q": np.asfortranarray(rng.standard_normal(sh).astype(F32))}
        state[lvl]["q"][0, 0, 0, 0] = np.nan                         # scrubbed like the reference's arrays
    fields = lambda lvl, name: grids[lvl].obstacle if name == "obstacle" else state[lvl][name]
    derived = [("Vorticity", lambda lvl: state[lvl]["w"], 3), ("QCriterion", lambda lvl: state[lvl]["q"], 1)]
    return grids, state, fields, derived


@pytest.mark.parametrize("compress", [True, False])
def test_flow_file_without_derived_arrays_is_unchanged(tmp_path, compress):
    grids, _, fields, _ = _levels_and_fields()
    p = output.export_merged_mesh(7, grids, fields, str(tmp_path), compress=compress)
    m = output.build_flow_mesh(7, grids, fields)
    assert "Vorticity" not in m and "QCriterion" not in m
    q = output.write_vtu(str(tmp_path / "direct"), m["points"], m["connectivity"], m["offsets"], m["types"],
                         [(n, m[n]) for n in output.DEFAULT_FLOW_FIELDS], compress)
    assert open(p, "rb").read() == open(q, "rb").read()


@pytest.mark.parametrize("compress", [True, False])
def test_flow_file_with_derived_arrays_round_trips(tmp_path, compress):
    grids, state, fields, derived = _levels_and_fields()
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain = output.export_merged_mesh(8, grids, fields, str(tmp_path / "a"), compress=compress)
    p = output.export_merged_mesh(8, grids, fields, str(tmp_path / "b"), compress=compress, derived=derived)
    txt, base = open(p).read(), open(plain).read()
    # the same file with two more arrays after the reference's five
    cut = base.index("</CellData>")
    assert txt.startswith(base[:cut]) and txt.endswith(base[cut:])
    assert re.findall(r'Name="(\w+)"', txt[cut:txt.index("</CellData>")]) == ["Vorticity", "QCriterion"]
    d = read_vtu_with_field_data(p)
    sel = output.select_export_blocks([g.active_block_coords for g in grids])
    assert d["n_cells"] == 512 * len(sel)
    want_w = np.concatenate([state[l]["w"][:, :, :, b].reshape(512, 3, order="F") for l, b in sel])
    want_q = np.concatenate([state[l]["q"][:, :, :, b].reshape(512, order="F") for l, b in sel])
    want_q[~np.isfinite(want_q)] = 0
    assert d["cells"]["Vorticity"].dtype == F32 and np.array_equal(d["cells"]["Vorticity"], want_w)
    assert np.array_equal(d["cells"]["QCriterion"], want_q)
    assert np.array_equal(d["cells"]["Level"], read_vtu_with_field_data(plain)["cells"]["Level"])


# ---- the C entry points reject bad arguments without a device ----
def test_entry_points_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    assert lib.ludwig_level_gradient_fields_compute(None, _lib.VEL, 1.0) == -1
    assert lib.ludwig_level_gradient_fields_compute(None, _lib.VEL_TEMP, float("nan")) == -1
    buf = np.zeros(4, F32)
    assert lib.ludwig_level_gradient_fields_download(None, _lib.GRAD_VORTICITY, buf.ctypes.data, buf.nbytes) == -1
    assert lib.ludwig_level_gradient_fields_download(None, 7, None, 0) == -1
    assert _lib.GRAD_NAMES == {"vorticity": (0, 3), "q": (1, 1)}
