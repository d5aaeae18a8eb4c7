"""Time-averaged statistics accumulated on the device (ludwig_level_stats_*, HipStepper.stats_*, run_case's flow_mean_%06d.vtu).

Each device sum is a sequential Float64 addition in sample order of values that are exact in Float64 (a float, or the product of
two floats), so the same additions in numpy give the same bits: the checks here are np.array_equal, not tolerances."""
import base64
import copy
import os
import re
import zlib

import numpy as np
import pytest

from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, output, preprocess as pp, statistics

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")


def _host_sums(n_levels):
    return [[None, None, None] for _ in range(n_levels)]


def _add(acc, rho, vel):
    r, u = rho.astype(np.float64), vel.astype(np.float64)
    uu = np.stack([u[..., i] * u[..., j] for i, j in statistics.PAIRS], axis=-1)
    for k, v in enumerate((r, u, uu)):
        acc[k] = v.copy() if acc[k] is None else acc[k] + v


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [2, 3])
def test_device_sums_equal_numpy_float64(gpu, levels):
    """Tunnel with sphere: temporal interpolation, Bouzidi on the finest level, wall model, default rho policy (the finest level
    elides its rho store, so the sample replays it). Sampled at odd and even coarse steps, with gaps and back to back."""
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    assert grids[-1].bouzidi_enabled and params.use_temporal_interp
    dev = [adapt(g, 0) for g in grids]
    for d in dev:
        d.stats_reset()
    samples = {2, 3, 6, 9, 11, 12}
    acc = _host_sums(levels)
    for t in range(1, 13):
        execute_timestep_batch(dev, t, 1, np.float32(0.05), params)
        if t not in samples:
            continue
        for lvl, d in enumerate(dev):
            t_sub = statistics.t_sub_after(lvl, t)
            assert lvl == 0 or t_sub % 2 == 1
            d.stats_accumulate(t_sub)                  # first, so that an elided rho is replayed by the sample itself
            _add(acc[lvl], d.download("rho"), d.download("vel_temp" if t_sub % 2 == 0 else "vel"))
    for lvl, d in enumerate(dev):
        for k, name in enumerate(("rho", "vel", "vel2")):
            got, n = d.stats_download(name)
            assert n == len(samples)
            assert got.shape == acc[lvl][k].shape
            assert np.array_equal(got, acc[lvl][k]), f"level {lvl + 1} {name}"
        assert np.abs(acc[lvl][1]).max() > 1e-3                       # a flow, not a zero field
    for d in dev:
        d.close()


@pytest.mark.gpu
def test_sampling_does_not_perturb_the_flow(gpu):
    grids, params = cases.tunnel_with_sphere(levels=3, wall_model=True)
    runs = []
    for sample in (False, True):
        dev = [adapt(g, 0) for g in grids]
        if sample:
            for d in dev:
                d.stats_reset()
        for t in range(1, 11):
            execute_timestep_batch(dev, t, 1, np.float32(0.05), params)
            if sample and t % 3 != 1:
                for lvl, d in enumerate(dev):
                    d.stats_accumulate(statistics.t_sub_after(lvl, t))
        runs.append([{n: d.download(n) for n in STATES} for d in dev])
        for d in dev:
            d.close()
    for lvl, (a, b) in enumerate(zip(*runs)):
        for n in STATES:
            assert np.array_equal(a[n], b[n]), f"level {lvl + 1} {n}"


@pytest.mark.gpu
def test_error_paths_and_reset(gpu):
    grids, params = cases.tunnel_with_sphere(levels=1)
    d = adapt(grids[0], 0)
    for call in (lambda: d.stats_accumulate(1), lambda: d.stats_download("rho")):
        with pytest.raises(_lib.LudwigError) as e:
            call()
        assert e.value.code == -5                                   # LUDWIG_ERR_STATE
    with pytest.raises(_lib.LudwigError) as e:
        _lib.check(_lib.load().ludwig_level_stats_download(d.handle, 7, None, 0, None))
    assert e.value.code == -1
    d.stats_reset()
    execute_timestep_batch([d], 1, 2, np.float32(0.05), params)
    d.stats_accumulate(2)
    d.stats_accumulate(2)
    s, n = d.stats_download("vel2")
    assert n == 2 and np.abs(s).max() > 0
    d.stats_reset()
    for name in ("rho", "vel", "vel2"):
        s, n = d.stats_download(name)
        assert n == 0 and not s.any(), name
    d.close()


@pytest.mark.gpu
def test_downloads_do_not_depend_on_the_internal_block_order(gpu, monkeypatch):
    """The statistics and gradient-field downloads place every block of the internal order back into the reference order. A periodic
    3 x 2 x 2 block box - block counts that differ per axis, where a wrong permutation shows - stepped twice from a non-uniform state:
    all three statistics and both gradient fields are bit-identical between a level in the library's own block order and one
    created under LUDWIG_REFERENCE_BLOCK_ORDER=1 (read when the level is created)."""
    grids, params = cases.periodic_box((3, 2, 2), init=False)
    cases.init_perturbed(grids[0], 7)
    got, orders = [], []
    for keep_reference_order in (False, True):
        if keep_reference_order:
            monkeypatch.setenv("LUDWIG_REFERENCE_BLOCK_ORDER", "1")
        else:
            monkeypatch.delenv("LUDWIG_REFERENCE_BLOCK_ORDER", raising=False)
        d = adapt(grids[0], 0)
        monkeypatch.undo()                                           # the switch is as it was once the level exists
        orders.append(d.block_order())
        execute_timestep_batch([d], 1, 2, np.float32(0.0), params)
        d.stats_reset()
        d.stats_accumulate(statistics.t_sub_after(0, 2))
        arrays = [d.stats_download(name)[0] for name in ("rho", "vel", "vel2")]
        arrays += list(d.gradient_fields("vel_temp", np.float32(1.0)))  # coarse step 2 is even: its output is vel_temp
        got.append(arrays)
        d.close()
    assert np.array_equal(orders[1], np.arange(12)) and not np.array_equal(orders[0], orders[1]), "the two levels share one block order"
    for name, a, b in zip(("rho", "vel", "vel2", "vorticity", "q"), *got):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32),
                              b.view(np.uint64 if a.dtype == np.float64 else np.uint32)), name
        assert np.abs(a).max() > 0, name                            # a flow, not a zero field


# ---- run_case end to end ----
_NP ={"Float32": np.float32, "Float64": np.float64, "Int32": np.int32, "Int64": np.int64, "UInt8": np.uint8}


def _decode(payload, dtype, compressed):
    b64 = lambda n: 4 * ((n + 2) // 3)
    if compressed:
        nblk = int(np.frombuffer(base64.b64decode(payload[:b64(24)]), dtype=np.uint64)[0])
        hl = b64(8 * (3 + nblk))
        sizes = np.frombuffer(base64.b64decode(payload[:hl]), dtype=np.uint64)[3:]
        blob, raw, o = base64.b64decode(payload[hl:]), b"", 0
        for s in sizes:
            raw += zlib.decompress(blob[o:o + int(s)])
            o += int(s)
    else:
        n = int(np.frombuffer(base64.b64decode(payload[:b64(8)]), dtype=np.uint64)[0])
        raw = base64.b64decode(payload[b64(8):])[:n]
    return np.frombuffer(raw, dtype=dtype)


def read_vtu_with_field_data(path):
    """{'cells': {name: array}, 'fields': {name: array}, 'n_cells': int} - cell arrays and VTK FieldData of a VTU file"""
    txt = open(path).read()
    compressed = 'compressor="vtkZLibDataCompressor"' in txt
    out = {"n_cells": int(re.search(r'NumberOfCells="(\d+)"', txt).group(1)), "cells": {}, "fields": {}}
    fd = re.search(r"<FieldData>(.*?)</FieldData>", txt, re.S)
    if fd:
        for m in re.finditer(r'<DataArray type="(\w+)" Name="(\w+)" NumberOfTuples="(\d+)" format="binary">([^<]*)</DataArray>', fd.group(1)):
            out["fields"][m.group(2)] = _decode(m.group(4), _NP[m.group(1)], compressed)
    cd = re.search(r"<CellData>(.*?)</CellData>", txt, re.S).group(1)
    for m in re.finditer(r'<DataArray type="(\w+)" Name="(\w+)"( NumberOfComponents="(\d+)")? format="binary">([^<]*)</DataArray>', cd):
        a = _decode(m.group(5), _NP[m.group(1)], compressed)
        k = int(m.group(4) or 1)
        out["cells"][m.group(2)] = a.reshape(-1, k) if k > 1 else a
    return out


@pytest.mark.gpu
def test_run_case_writes_mean_flow_and_leaves_everything_else_alone(gpu, tmp_path):
    """ball1m, 3 levels, 48 steps in batches of 8, inside the inlet ramp (the batches cut at sample steps keep their inlet speed);
    samples at 5, 8, ..., 47; output at 24 and 48."""
    base = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}}})
    base.diag_freq, base.output_freq = 16, 24
    assert base.async_depth == 8 and base.ramp_steps > 48
    stl = os.path.join(G, "ball1m.stl")
    on = copy.copy(base)
    on.statistics_enabled, on.statistics_start_step, on.statistics_interval = True, 5, 3
    holder = {}

    def keep(grids):
        holder["st"] = case.HipStepper(grids)
        holder["st"].close = lambda: None
        return holder["st"]
    d_off, d_on = tmp_path / "off", tmp_path / "on"
    case.run_case(base, case.HipStepper, steps=48, setup=pp.setup_multilevel_domain(base, stl), out_dir=str(d_off))
    setup = pp.setup_multilevel_domain(on, stl)
    case.run_case(on, keep, steps=48, setup=setup, out_dir=str(d_on))
    st, grids = holder["st"], setup[0]
    try:
        assert sorted(os.listdir(d_on)) == sorted(os.listdir(d_off) + ["flow_mean_000024.vtu", "flow_mean_000048.vtu"])
        for name in os.listdir(d_off):
            a, b = open(d_off / name, "rb").read(), open(d_on / name, "rb").read()
            if name == "convergence.csv":               # Walltime and MLUPS differ from run to run
                strip = lambda t: [",".join(c for i, c in enumerate(l.split(",")) if i not in (1, 5)) for l in t.decode().splitlines()]
                assert strip(a) == strip(b)
            else:
                assert a == b, name
        w24 = read_vtu_with_field_data(str(d_on / "flow_mean_000024.vtu"))["fields"]
        assert (w24["StatisticsSamples"][0], w24["StatisticsFirstStep"][0], w24["StatisticsLastStep"][0]) == (7, 5, 23)
        m = read_vtu_with_field_data(str(d_on / "flow_mean_000048.vtu"))
        assert {k: (v.dtype, v[0]) for k, v in m["fields"].items()} == {
            "StatisticsSamples": (np.int64, 15), "StatisticsFirstStep": (np.int64, 5), "StatisticsLastStep": (np.int64, 47)}
        sel = output.select_export_blocks([g.active_block_coords for g in grids])
        assert m["n_cells"] == 512 * len(sel)
        want = {k: [] for k in ("MeanDensity", "MeanVelocity", "ReynoldsStress", "TurbulentKineticEnergy")}
        for lvl in sorted({l for l, _ in sel}):
            fin = st.statistics(lvl)
            blocks = [b for l, b in sel if l == lvl]
            for name, key, k in (("MeanDensity", "mean_rho", 1), ("MeanVelocity", "mean_u", 3), ("ReynoldsStress", "reynolds_stress", 6),
                                 ("TurbulentKineticEnergy", "tke", 1)):
                a = fin[key].astype(np.float32)[:, :, :, blocks]                  # [8,8,8,nsel(,K)] -> cells x fastest, block by block
                want[name].append(a.reshape((512, len(blocks), k), order="F").transpose(1, 0, 2).reshape(-1, k))
        for name, parts in want.items():
            got, exp = m["cells"][name], np.concatenate(parts)
            assert got.dtype == np.float32
            assert np.array_equal(got.reshape(exp.shape), exp), name
        assert np.abs(m["cells"]["MeanVelocity"]).max() > 1e-6 and (m["cells"]["TurbulentKineticEnergy"] >= -1e-12).all()   # early in the ramp
        flow = read_vtu_with_field_data(str(d_on / "flow_000048.vtu"))
        assert not flow["fields"]
        for name in ("Obstacle", "Level"):
            assert np.array_equal(m["cells"][name], flow["cells"][name])
    finally:
        for d in st.dev:
            d.close()
