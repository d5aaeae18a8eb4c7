"""Host side of the time-averaged statistics: configuration keys, finalisation maths, sample schedule, FieldData in the VTU writer."""
import glob
import os
import re

import numpy as np
import pytest

from open_ludwig_amd import output, preprocess as pp, statistics
from test_gpu_statistics import read_vtu_with_field_data

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_shipped_configs_parse_with_statistics_off():
    paths = sorted(glob.glob(os.path.join(G, "*_config.yaml")))
    assert len(paths) >= 4
    for p in paths:
        cfg = pp.load_case_configuration(p)
        assert cfg.statistics_enabled is False
        assert cfg.statistics_start_step == max(cfg.ramp_steps, 1) and cfg.statistics_interval == 10


def test_statistics_keys_parse_when_given():
    p = os.path.join(G, "ball1m_config.yaml")
    base = pp.load_case_configuration(p)
    cfg = pp.load_case_configuration(p, {"advanced": {"statistics": {"enabled": True, "start_step": 1234, "interval": 7}}})
    assert (cfg.statistics_enabled, cfg.statistics_start_step, cfg.statistics_interval) == (True, 1234, 7)
    only = pp.load_case_configuration(p, {"advanced": {"statistics": {"enabled": True}}})
    assert (only.statistics_start_step, only.statistics_interval) == (base.ramp_steps, 10)
    for name in base.__dataclass_fields__:            # nothing else moves
        if not name.startswith("statistics_"):
            assert repr(getattr(cfg, name)) == repr(getattr(base, name)), name
    with pytest.raises(ValueError):
        pp.load_case_configuration(p, {"advanced": {"statistics": {"interval": 0}}})


def test_sub_step_of_each_level_after_a_coarse_step():
    # level l (1-based) finishes t_sub = 2^(l-1) t + 2^(l-1) - 1
    assert [statistics.t_sub_after(0, t) for t in (1, 2, 7)] == [1, 2, 7]
    assert [statistics.t_sub_after(1, t) for t in (1, 2, 7)] == [3, 5, 15]
    assert [statistics.t_sub_after(2, t) for t in (1, 2)] == [7, 11]


def test_sample_schedule():
    assert statistics.sample_steps(1, 8, 5, 3) == [5, 8]
    assert statistics.sample_steps(9, 16, 5, 3) == [11, 14]
    assert statistics.sample_steps(1, 4, 5, 3) == []
    assert statistics.sample_steps(6, 7, 5, 3) == []
    got = [s for a in range(1, 100, 8) for s in statistics.sample_steps(a, min(a + 7, 99), 20, 10)]
    assert got == list(range(20, 100, 10)) and all(statistics.is_sample_step(s, 20, 10) for s in got)


def test_finalisation_matches_direct_numpy_on_a_series():
    rng = np.random.default_rng(11)
    n, shape = 37, (8, 8, 8, 3)
    rho = (1.0 + 0.01 * rng.standard_normal((n,) + shape)).astype(np.float32)
    u = (0.05 * rng.standard_normal((n,) + shape + (3,)) + [0.03, 0.0, -0.01]).astype(np.float32)
    r64, u64 = rho.astype(np.float64), u.astype(np.float64)
    s_rho, s_u = np.zeros(shape), np.zeros(shape + (3,))
    s_uu = np.zeros(shape + (6,))
    for i in range(n):                                   # the device's sums: sequential, in sample order
        s_rho += r64[i]
        s_u += u64[i]
        s_uu += np.stack([u64[i][..., a] * u64[i][..., b] for a, b in statistics.PAIRS], axis=-1)
    fin = statistics.finalize(s_rho, s_u, s_uu, n)
    assert np.allclose(fin["mean_rho"], r64.mean(axis=0), rtol=0, atol=1e-14)
    assert np.allclose(fin["mean_u"], u64.mean(axis=0), rtol=0, atol=1e-15)
    for m, (a, b) in enumerate(statistics.PAIRS):
        cov = ((u64[..., a] - u64[..., a].mean(axis=0)) * (u64[..., b] - u64[..., b].mean(axis=0))).mean(axis=0)
        assert np.allclose(fin["reynolds_stress"][..., m], cov, rtol=1e-9, atol=1e-15), m
    k = 0.5 * sum(u64[..., a].var(axis=0) for a in range(3))
    assert np.allclose(fin["tke"], k, rtol=1e-9, atol=1e-15)
    assert np.isnan(statistics.finalize(s_rho, s_u, s_uu, 0)["mean_rho"]).all()


def _mesh():
    pts = np.arange(24, dtype=np.float32).reshape(8, 3)
    return pts, np.arange(8, dtype=np.int64), np.array([8], dtype=np.int64), np.array([output.VTK_VOXEL], dtype=np.uint8)


@pytest.mark.parametrize("compress", [True, False])
def test_write_vtu_field_data_round_trip(tmp_path, compress):
    pts, conn, off, types = _mesh()
    cd = [("A", np.array([1.5], dtype=np.float32)), ("B", np.array([[1.0, 2.0, 3.0]], dtype=np.float32))]
    fd = [("StatisticsSamples", np.array([12], dtype=np.int64)), ("StatisticsFirstStep", np.array([2000], dtype=np.int64)),
          ("Window", np.array([1.0, 2.5], dtype=np.float64))]
    p = output.write_vtu(str(tmp_path / "x"), pts, conn, off, types, cd, compress, field_data=fd)
    d = read_vtu_with_field_data(p)
    assert set(d["fields"]) == {n for n, _ in fd}
    for n, a in fd:
        assert d["fields"][n].dtype == a.dtype and np.array_equal(d["fields"][n], a), n
    assert np.array_equal(d["cells"]["A"], cd[0][1]) and np.array_equal(d["cells"]["B"], cd[1][1])
    txt = open(p).read()
    assert txt.index("<FieldData>") < txt.index("<Piece")


@pytest.mark.parametrize("compress", [True, False])
def test_write_vtu_without_field_data_is_unchanged(tmp_path, compress):
    """byte for byte what the writer produced before FieldData existed (the text below is that writer's format)"""
    pts, conn, off, types = _mesh()
    cd = [("A", np.array([1.5], dtype=np.float32))]
    p = output.write_vtu(str(tmp_path / "x"), pts, conn, off, types, cd, compress)
    q = output.write_vtu(str(tmp_path / "y"), pts, conn, off, types, cd, compress, field_data=None)
    txt = open(p).read()
    assert txt == open(q).read() and "FieldData" not in txt
    enc = lambda a: output._encode(a, compress)
    comp = ' compressor="vtkZLibDataCompressor"' if compress else ""
    want = ('<?xml version="1.0" encoding="utf-8"?>\n'
            f'<VTKFile type="UnstructuredGrid" version="1.0" byte_order="LittleEndian" header_type="UInt64"{comp}>\n'
            '<UnstructuredGrid>\n<Piece NumberOfPoints="8" NumberOfCells="1">\n'
            f'<Points>\n<DataArray type="Float32" Name="Points" NumberOfComponents="3" format="binary">{enc(pts)}</DataArray>\n</Points>\n'
            f'<Cells>\n<DataArray type="Int64" Name="connectivity" format="binary">{enc(conn)}</DataArray>\n'
            f'<DataArray type="Int64" Name="offsets" format="binary">{enc(off)}</DataArray>\n'
            f'<DataArray type="UInt8" Name="types" format="binary">{enc(types)}</DataArray>\n'
            f'</Cells>\n<CellData>\n<DataArray type="Float32" Name="A" format="binary">{enc(cd[0][1])}</DataArray>\n'
            '</CellData>\n</Piece>\n</UnstructuredGrid>\n</VTKFile>\n')
    assert txt == want


def test_mean_mesh_on_host_levels(tmp_path):
    """export_mean_mesh: the flow file's blocks and cell order, Float32 statistics, Int64 window"""
    from open_ludwig_amd import cases
    grids, _ = cases.tunnel_with_sphere((4, 2, 2), levels=2)
    rng = np.random.default_rng(3)
    fins = {}
    for lvl, g in enumerate(grids):
        sh = (8, 8, 8, g.n_blocks)
        fins[lvl] = {"mean_rho": rng.standard_normal(sh), "mean_u": rng.standard_normal(sh + (3,)),
                     "reynolds_stress": rng.standard_normal(sh + (6,)), "tke": rng.standard_normal(sh)}
    p = output.export_mean_mesh(40, grids, fins.__getitem__, (4, 10, 40), str(tmp_path))
    assert os.path.basename(p) == "flow_mean_000040.vtu"
    d = read_vtu_with_field_data(p)
    assert [int(d["fields"][k][0]) for k in ("StatisticsSamples", "StatisticsFirstStep", "StatisticsLastStep")] == [4, 10, 40]
    sel = output.select_export_blocks([g.active_block_coords for g in grids])
    assert d["n_cells"] == 512 * len(sel)
    l, b = sel[-1]
    assert np.array_equal(d["cells"]["ReynoldsStress"][-512:], fins[l]["reynolds_stress"][:, :, :, b].astype(np.float32).reshape(512, 6, order="F"))
    assert np.array_equal(d["cells"]["MeanDensity"][:512], fins[0]["mean_rho"][:, :, :, sel[0][1]].astype(np.float32).reshape(-1, order="F"))
    assert d["cells"]["Level"].dtype == np.int32 and d["cells"]["Obstacle"].dtype == np.uint8
    assert re.search(r'Name="TurbulentKineticEnergy"', open(p).read())
