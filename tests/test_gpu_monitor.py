"""The flow monitor on the device (ludwig_level_monitor, DeviceLevel.monitor, HipStepper.monitor, run_case's flow_monitor.csv).
k_monitor_blocks / k_monitor_combine evaluate monitor.host_monitor's float32 expression and its balanced Float64 tree in the same order
with -ffp-contract=off, so every check against the restatement is exact: counts, extremes, cells and both sums."""
import ctypes as C
import os

import numpy as np
import pytest

from open_ludwig_amd import _lib, adapt, case, cases, monitor as mon, preprocess as pp
from open_ludwig_amd.statistics import t_sub_after

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
U = F32(0.05)
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")


def _same(a: mon.Record, b: mon.Record, what=""):
    assert a == b, f"{what}\n{a}\n{b}"
    for name in ("rho_min", "rho_max", "v2_max", "sum_rho", "sum_rho_v2"):        # == lets -0.0 pass for +0.0: the bits too
        x, y = getattr(a, name), getattr(b, name)
        if x != 0:
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (what, name)


def _host(d, g, t_sub):
    return mon.host_monitor(d.download("rho"), d.download("vel_temp" if t_sub % 2 == 0 else "vel"), g.obstacle, g.active_block_coords)


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_stepped_levels_equal_restatement_after_odd_and_even_steps(gpu, levels):
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    st = case.HipStepper(grids)                                        # the default rho policy: the monitor call replays an elided rho
    try:
        for t in (1, 2, 3, 4):
            st.batch(t, 1, U, params)
            if t < 3:
                continue
            for lvl, g in enumerate(grids):
                got = st.monitor(lvl, t)                               # before any download: the call itself has to produce rho
                want = _host(st.dev[lvl], g, t_sub_after(lvl, t))
                _same(got, want, f"level {lvl + 1} step {t}")
                assert got.n_bad == 0 and got.n_fluid == int((~g.obstacle).sum()) and 0.5 < float(got.rho_min) <= float(got.rho_max) < 1.5
                assert got.rho_min == F32(st.dev[lvl].rho_min())
    finally:
        st.close()


def _uploaded(shape, seed):
    """an unstepped periodic box whose vel and vel_temp hold different perturbed states"""
    grids, _ = cases.periodic_box(shape, init=False)
    g = grids[0]
    cases.init_perturbed(g, seed + 100)
    other = g.vel.copy(order="F")
    cases.init_perturbed(g, seed)
    g.vel_temp[...] = other
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 1, 1), (9, 8, 8)])        # a lone block, an odd count, 576 blocks: past one 512-chunk
def test_uploaded_levels_equal_restatement_for_both_buffers(gpu, shape):
    g = _uploaded(shape, 3)
    d = adapt(g, 0)
    try:
        recs = []
        for t_sub in (0, 1, 2, 5):
            got = d.monitor(t_sub)
            _same(got, mon.host_monitor(g.rho, g.vel_temp if t_sub % 2 == 0 else g.vel, g.obstacle, g.active_block_coords), f"t_sub {t_sub}")
            recs.append(got)
        assert recs[0] == recs[2] and recs[1] == recs[3] and recs[0].sum_rho_v2 != recs[1].sum_rho_v2
    finally:
        d.close()


@pytest.mark.gpu
def test_planted_states(gpu):
    g = _uploaded((3, 2, 2), 8)
    g.obstacle[:, :, :, 7] = True                                      # an all-obstacle block
    g.obstacle[4, 4, 4, 6] = g.obstacle[4, 4, 5, 6] = g.obstacle[4, 5, 5, 6] = True
    d = adapt(g, 0)
    try:
        order = d.block_order()
        pairs = [(a, b) for a in range(g.n_blocks) for b in range(a + 1, g.n_blocks) if order[a] > order[b] and 7 not in (a, b) and 6 not in (a, b)]
        assert pairs, "the internal block order should differ from the reference order on a 3 x 2 x 2 box"
        a, b = pairs[0]
        rho, vel = g.rho.copy(order="F"), g.vel.copy(order="F")
        rho[7, 7, 7, a] = rho[0, 0, 0, b] = F32(0.125)                 # equal minima: the reference order says a, the internal order b
        vel[6, 7, 7, a, :] = vel[1, 0, 0, b, :] = F32(0.2)             # equal maxima of v2 likewise
        rho[4, 4, 4, 6], rho[4, 4, 5, 6], rho[4, 5, 5, 6] = F32(1e-9), F32(77.0), np.nan      # hidden in obstacle cells
        vel[4, 4, 5, 6, :] = F32(9.0)
        d.upload("rho", rho)
        d.upload("vel", vel)
        clean = d.monitor(1)
        _same(clean, mon.host_monitor(rho, vel, g.obstacle, g.active_block_coords), "ties")
        ca = tuple(g.active_block_coords[a])
        assert clean.n_bad == 0 and clean.rho_min == F32(0.125) and clean.cell_rho_min == ca + (511,) and clean.cell_v2_max == ca + (510,)
        assert float(clean.rho_max) < 2.0 and clean.n_fluid == 11 * 512 - 3
        # non-finite states: uploads only, nothing is stepped
        rho[3, 2, 1, 5] = np.nan
        vel[1, 1, 1, 2, 0] = np.inf
        vel[1, 1, 2, 2, 2] = -np.inf
        vel[5, 5, 5, 9, 1] = F32(3e19)                                 # finite, its square is not
        vel[2, 0, 0, 4, :] = F32(1.1e19)                               # every square finite, their sum is not
        vel[0, 0, 0, 1, :] = F32(-0.0)
        d.upload("rho", rho)
        d.upload("vel", vel)
        got = d.monitor(3)
        _same(got, mon.host_monitor(rho, vel, g.obstacle, g.active_block_coords), "planted")
        assert got.n_bad == 5 and got.first_bad == tuple(g.active_block_coords[2]) + (1 + 8 + 64,)
        assert np.isfinite(got.sum_rho) and np.isfinite(got.sum_rho_v2) and float(got.v2_max) == float(F32(F32(0.2) * F32(0.2) * 2) + F32(0.2) * F32(0.2))
        # every fluid cell bad
        rho[...] = np.nan
        d.upload("rho", rho)
        none = d.monitor(1)
        _same(none, mon.host_monitor(rho, vel, g.obstacle, g.active_block_coords), "all bad")
        assert none.n_counted == 0 and none.cell_rho_min is None and none.rho_min == F32(np.inf) and none.first_bad == (1, 1, 1, 0)
    finally:
        d.close()


@pytest.mark.gpu
def test_monitoring_leaves_every_state_array_alone(gpu):
    grids, params = cases.tunnel_with_sphere(levels=3, wall_model=True)
    a, b = case.HipStepper(grids), case.HipStepper(grids)
    try:
        for t in (1, 3, 5, 7, 9):
            a.batch(t, 2, U, params)
            b.batch(t, 2, U, params)
            for lvl in range(len(grids)):
                b.monitor(lvl, t + 1)
        for li in range(len(grids)):
            for n in STATES:
                assert np.array_equal(a.field(li, n), b.field(li, n)), f"level {li + 1} {n}: the monitor changed the flow"
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_error_paths(gpu, hip_lib):
    counts, cells = np.zeros(2, np.int64), np.zeros(16, np.int64)
    ext, sums = np.zeros(3, F32), np.zeros(2, np.float64)
    args = (counts.ctypes.data, cells.ctypes.data, ext.ctypes.data, sums.ctypes.data)
    assert hip_lib.ludwig_level_monitor(None, 0, *args) == -1 and b"null" in hip_lib.ludwig_last_error()
    grids, _ = cases.periodic_box((2, 1, 1))
    d = adapt(grids[0], 0)
    try:
        assert hip_lib.ludwig_level_monitor(d.handle, -1, *args) == -1 and b"t_sub" in hip_lib.ludwig_last_error()
        assert hip_lib.ludwig_level_monitor(d.handle, 0, None, *args[1:]) == -1
        with pytest.raises(_lib.LudwigError):
            d.monitor(-3)
        assert d.monitor(0).n_fluid == 1024
    finally:
        d.close()


RE266K = {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}, "simulation": {"steps": 12, "output_freq": 12}},
          "advanced": {"diagnostics": {"freq": 6}}}


def _cfg(**monitor):
    return pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), {**RE266K, "advanced": {**RE266K["advanced"], "flow_monitor": monitor}})


@pytest.fixture(scope="module")
def ball_setup():
    return pp.setup_multilevel_domain(_cfg(), os.path.join(G, "ball1m.stl"))


def _rows(path):
    lines = open(path).read().splitlines()
    assert lines[0] == mon.CSV_HEADER
    return [l.split(",") for l in lines[1:]]


@pytest.mark.gpu
def test_ball1m_run_case_rows_and_untouched_files(gpu, tmp_path, ball_setup):
    kept = []

    class Kept(case.HipStepper):
        def __init__(self, grids):
            super().__init__(grids)
            kept.append(self)

        def close(self):
            pass
    grids, _, params, _ = ball_setup
    out, logs = {}, []
    for on in (False, True):
        d = os.path.join(tmp_path, "on" if on else "off")
        case.run_case(_cfg(enabled=on), Kept, setup=ball_setup, out_dir=d, log=logs.append)
        out[on] = d
    try:
        names = sorted(os.listdir(out[False]))
        assert sorted(os.listdir(out[True])) == sorted(names + ["flow_monitor.csv"])
        for n in names:
            a, b = (open(os.path.join(out[k], n), "rb").read() for k in (False, True))
            if n == "convergence.csv":                                     # wall time and MLUPS columns
                strip = lambda raw: [[c for i, c in enumerate(l.split(",")) if i not in (1, 5)] for l in raw.decode().splitlines()]
                a, b = strip(a), strip(b)
            assert a == b, n
        rows = _rows(os.path.join(out[True], "flow_monitor.csv"))
        assert [(r[0], r[1], r[2]) for r in rows] == [(s, e, str(g.level_id)) for s, e in (("6", "8"), ("12", "12")) for g in grids]
        st = kept[1]
        for lvl, g in enumerate(grids):                                    # the kept stepper still holds the state after step 12
            rec = st.monitor(lvl, 12)
            assert ",".join(rows[len(grids) + lvl]) == mon.csv_row(12, 12, g.level_id, rec, g.dx, params.mesh_offset)
            _same(rec, _host(st.dev[lvl], g, t_sub_after(lvl, 12)), f"level {lvl + 1}")
            assert rec.n_bad == 0 and rows[len(grids) + lvl][-3:] == ["", "", ""]
        conv = [l.split(",") for l in open(os.path.join(out[True], "convergence.csv")).read().splitlines()[1:]]
        assert [c[0] for c in conv] == ["6", "12"]
        for c in conv:
            (lvl1,) = [r for r in rows if r[0] == c[0] and r[2] == str(grids[0].level_id)]
            assert lvl1[5] == c[4]                                          # level 1's RhoMin is convergence.csv's rho_min
        assert not [l for l in logs if "WARNING" in l]
    finally:
        for st in kept:
            case.HipStepper.close(st)


@pytest.mark.gpu
@pytest.mark.parametrize("stop", [True, False])
def test_divergence_is_reported_and_stops_the_run_when_asked(gpu, tmp_path, ball_setup, stop):
    grids, _, params, _ = ball_setup
    fin = len(grids) - 1
    cell = (3, 2, 1, int(np.flatnonzero(~grids[fin].obstacle[3, 2, 1, :])[5]))       # i, j, k, reference block

    class Poisoned(case.HipStepper):
        def batch(self, t_start, n, u_curr, params):
            super().batch(t_start, n, u_curr, params)
            if t_start + n - 1 == 8:                                    # the end of the first batch: the state diagnostics step 6 looks at
                rho = self.field(fin, "rho")
                rho[cell] = np.nan
                self.dev[fin].upload("rho", rho)
    want = tuple(grids[fin].active_block_coords[cell[3]]) + (cell[0] + 8 * cell[1] + 64 * cell[2],)
    d, logs = str(tmp_path), []
    cfg = _cfg(enabled=True, stop_on_divergence=stop)
    if stop:
        with pytest.raises(mon.FlowDiverged) as err:
            case.run_case(cfg, Poisoned, setup=ball_setup, out_dir=d, log=logs.append)
        e = err.value
        assert (e.step, e.level, e.cell, e.n_bad) == (6, grids[fin].level_id, want, 1)
        assert e.coordinates == mon.cell_coordinates(want, grids[fin].dx, params.mesh_offset)
    else:
        case.run_case(cfg, Poisoned, setup=ball_setup, out_dir=d, log=logs.append)
    rows = _rows(os.path.join(d, "flow_monitor.csv"))
    first = rows[: len(grids)]
    assert [(r[0], r[1]) for r in first] == [("6", "8")] * len(grids)
    assert [r[4] for r in first] == ["0"] * fin + ["1"]
    assert first[fin][-3:] == [mon._num(np.float64(v)) for v in mon.cell_coordinates(want, grids[fin].dx, params.mesh_offset)]
    assert len(rows) == (len(grids) if stop else 2 * len(grids))
    assert len(open(os.path.join(d, "convergence.csv")).read().splitlines()) == (2 if stop else 3)
    if not stop:
        # the run went on to the last step (rho is an output of the step: the next one overwrites the planted cell)
        assert [r[0] for r in rows[len(grids):]] == ["12"] * len(grids) and rows[-1][4] == "0"
    assert any("Non-finite cells: 1" in l for l in logs)
