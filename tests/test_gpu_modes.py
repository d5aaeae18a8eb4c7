"""Fourier modes accumulated on the device (ludwig_modes_*, the LUDWIG_OBSERVE_MODES entry of ludwig_execute_timestep_batch_observed,
HipStepper.modes_*, run_case's flow_modes_%06d.vtu and flow_modes.csv).

A device sum is S = S + W[r, m] * float64(v): one Float64 multiply and one Float64 add per sample, never fused. The same two operations
in numpy give the same bits, so every comparison here is np.array_equal (NaN meeting NaN counts as equal), not a tolerance."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, modes, output, preprocess as pp, statistics
from test_gpu_statistics import read_vtu_with_field_data

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")
U = np.float32(0.05)


def _table(n_rows=6, n_columns=5, seed=11):
    """a seeded table with an exact 0.0, a negative weight and a weight of 2^-60"""
    W = np.random.default_rng(seed).uniform(-1.0, 1.0, (n_rows, n_columns))
    W[1, n_columns // 2], W[2 % n_rows, 0], W[n_rows - 1, n_columns - 1] = 0.0, -0.75, 2.0 ** -60
    assert (W < 0).any()
    return np.ascontiguousarray(W)


def _state(dev):
    return [{n: d.download(n) for n in STATES} for d in dev]


def _assert_same_state(a, b, what):
    for lvl, (x, y) in enumerate(zip(a, b)):
        for n in STATES:
            assert np.array_equal(x[n].view(np.uint32), y[n].view(np.uint32)), f"{what}: level {lvl + 1} {n}"


def _sample_fields(d, t_sub):
    """[8,8,8,nb,4] float32: rho, ux, uy, uz of the state sub-step t_sub wrote"""
    return np.concatenate([d.download("rho")[..., None], d.download("vel_temp" if t_sub % 2 == 0 else "vel")], axis=-1)


def _downloads(S, n_levels):
    return [[S.download(lvl, m) for m in range(S.n_columns)] for lvl in range(n_levels)]


def _assert_same_sums(a, b, what):
    for lvl, (la, lb) in enumerate(zip(a, b)):
        for m, ((x, nx), (y, ny)) in enumerate(zip(la, lb)):
            assert nx == ny, f"{what}: level {lvl + 1} samples {nx} != {ny}"
            assert np.array_equal(x, y, equal_nan=True), f"{what}: level {lvl + 1} column {m}"


# ---- 1. device sums equal numpy ----
@pytest.mark.gpu
@pytest.mark.parametrize("levels", [2, 3])
def test_device_sums_equal_numpy_float64(gpu, levels):
    """Tunnel with sphere, wall model, default rho policy before the set is made. Stand-alone samples after coarse steps 2, 3, 6, 9, 11,
    12: odd and even, with gaps and back to back."""
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    dev = [adapt(g, 0) for g in grids]
    W = _table()
    S = _lib.ModeSet(dev, W)
    try:
        samples = (2, 3, 6, 9, 11, 12)
        acc = [np.zeros((W.shape[1], 8, 8, 8, g.n_blocks, 4)) for g in grids]
        for t in range(1, 13):
            execute_timestep_batch(dev, t, 1, U, params)
            if t not in samples:
                continue
            row = samples.index(t)
            for lvl, d in enumerate(dev):
                t_sub = statistics.t_sub_after(lvl, t)
                S.accumulate(lvl, t_sub, row)
                modes.host_accumulate(acc[lvl], W[row], _sample_fields(d, t_sub))
        for lvl in range(levels):
            for m in range(W.shape[1]):
                got, n = S.download(lvl, m)
                assert n == 6 and got.dtype == np.float64 and got.shape == acc[lvl][m].shape
                assert np.array_equal(got, acc[lvl][m], equal_nan=True), f"level {lvl + 1} column {m}"
            assert np.abs(acc[lvl][0][..., 1:]).max() > 1e-4             # a flow, not a zero field
    finally:
        S.close()
        for d in dev:
            d.close()


# ---- 2. inside the batch ----
@pytest.mark.gpu
def test_in_batch_equals_stand_alone_and_perturbs_nothing(gpu):
    """A: a MODES entry (start 2, interval 3) through batches of 8 and then 4 steps; B: one step at a time with stand-alone samples at
    the same steps; C: unobserved"""
    grids, params = cases.tunnel_with_sphere(levels=3, wall_model=True)
    W = _table()
    runs = {}
    for how in ("batch", "alone", "plain"):
        dev = [adapt(g, 0) for g in grids]
        S = _lib.ModeSet(dev, W, 2, 3) if how != "plain" else None
        try:
            if how == "batch":
                execute_timestep_batch(dev, 1, 8, U, params, modes=S)
                execute_timestep_batch(dev, 9, 4, U, params, modes=S)
            elif how == "alone":
                for t in range(1, 13):
                    execute_timestep_batch(dev, t, 1, U, params)
                    if t >= 2 and (t - 2) % 3 == 0:
                        for lvl in range(3):
                            S.accumulate(lvl, statistics.t_sub_after(lvl, t), S.row_of(t))
            else:
                execute_timestep_batch(dev, 1, 12, U, params)
            runs[how] = (_downloads(S, 3) if S is not None else None, _state(dev))
        finally:
            if S is not None:
                S.close()
            for d in dev:
                d.close()
    assert all(n == 4 for lvl in runs["batch"][0] for _, n in lvl)       # steps 2, 5, 8, 11
    assert all(np.abs(a[..., 1:]).max() > 0 for lvl in runs["batch"][0] for a, _ in lvl[:1])
    _assert_same_sums(runs["batch"][0], runs["alone"][0], "in-batch against stand-alone")
    _assert_same_state(runs["batch"][1], runs["plain"][1], "a batch with the set against one without")
    _assert_same_state(runs["alone"][1], runs["plain"][1], "batches of one against one batch")


# ---- 3. rows and windows ----
@pytest.mark.gpu
def test_rows_windows_and_refusals(gpu):
    lib = _lib.load()
    grids, params = cases.tunnel_with_sphere(levels=2, wall_model=True)
    dev, other = [adapt(g, 0) for g in grids], [adapt(g, 0) for g in grids]
    fl = params.to_c()
    W = _table(4, 3)
    S, Y, fresh = _lib.ModeSet(dev, W), _lib.ModeSet(other, W), None

    def observed(levels, t0, n, entries):
        arr = (C.c_void_p * len(levels))(*[d.handle for d in levels])
        obs = (_lib.BatchObserver * len(entries))(*entries)
        return lib.ludwig_execute_timestep_batch_observed(arr, len(levels), t0, n, float(U), C.byref(fl), obs, len(entries))

    def entry(s, start=1, interval=1):
        return _lib.BatchObserver(_lib.OBSERVE_MODES, s.handle.value, start, interval)
    try:
        for lvl in range(2):                                             # download before any sample: zeros, n = 0
            for m in range(3):
                a, n = S.download(lvl, m)
                assert n == 0 and not a.any()
        assert observed(dev, 1, 1, []) == 0
        before = _state(dev)
        assert observed(dev, 2, 5, [entry(S, 2, 1)]) == -5 and b"window" in lib.ludwig_last_error()      # rows 0..4 of a window of 4
        assert observed(dev, 3, 2, [entry(S, 2, 1)]) == -5 and b"samples" in lib.ludwig_last_error()     # step 3 is row 1, count is 0
        assert observed(dev, 2, 1, [entry(S, 2, 0)]) == -1 and b"interval" in lib.ludwig_last_error()
        assert observed(dev, 2, 1, [entry(Y, 2, 1)]) == -1 and b"other levels" in lib.ludwig_last_error()
        assert observed(dev[:1], 2, 1, [entry(S, 2, 1)]) == -1 and b"modes" in lib.ludwig_last_error()
        assert observed(dev, 2, 1, [entry(S, 2, 1), entry(S, 2, 1)]) == -1 and b"observer" in lib.ludwig_last_error()
        assert observed(dev, 2, 1, [_lib.BatchObserver(7, S.handle.value, 1, 1)]) == -1 and b"observer" in lib.ludwig_last_error()
        _assert_same_state(_state(dev), before, "after the refusals")    # nothing was stepped
        assert all(S.download(lvl, 0)[1] == 0 for lvl in range(2))       # and nothing was sampled
        # stand-alone rows: in order, none skipped, inside the table
        for row, code, word in ((1, -5, b"rows come in order"), (4, -1, b"row"), (-1, -1, b"row")):
            assert lib.ludwig_modes_accumulate(S.handle, 0, 1, row) == code and word in lib.ludwig_last_error(), row
        assert lib.ludwig_modes_accumulate(S.handle, 0, 1, 1) == -5
        assert b"row 1" in lib.ludwig_last_error() and b"0 samples" in lib.ludwig_last_error()      # the message names both numbers
        assert lib.ludwig_modes_accumulate(S.handle, 2, 1, 0) == -1 and lib.ludwig_modes_download(S.handle, 0, 3, None, 0, None) == -1
        # the window's 4 samples in one batch (steps 2..5); a fifth is refused in a batch and stand-alone
        assert observed(dev, 2, 4, [entry(S, 2, 1)]) == 0, lib.ludwig_last_error()
        assert all(S.download(lvl, 0)[1] == 4 for lvl in range(2))
        assert observed(dev, 6, 1, [entry(S, 2, 1)]) == -5
        assert lib.ludwig_modes_accumulate(S.handle, 0, 11, 4) == -1
        # after a reset the next window's sums are a fresh set's
        S.reset()
        assert all(S.download(lvl, 0)[1] == 0 and not S.download(lvl, 2)[0].any() for lvl in range(2))
        fresh = _lib.ModeSet(dev, W, 6, 1)
        for t in (6, 7):                                                 # the reset set inside the batch, the fresh one right behind it
            assert observed(dev, t, 1, [entry(S, 6, 1)]) == 0, lib.ludwig_last_error()
            for lvl in range(2):
                fresh.accumulate(lvl, statistics.t_sub_after(lvl, t), fresh.row_of(t))
        got = _downloads(S, 2)
        assert all(n == 2 for lvl in got for _, n in lvl)
        _assert_same_sums(got, _downloads(fresh, 2), "a reset set against a fresh one")
        assert np.abs(S.download(1, 0)[0]).max() > 0
    finally:
        for s in (S, Y, fresh):
            if s is not None:
                s.close()
        for d in dev + other:
            d.close()


# ---- 4. block order ----
@pytest.mark.gpu
def test_downloads_do_not_depend_on_the_internal_block_order(gpu, monkeypatch):
    grids, params = cases.periodic_box((3, 2, 2), init=False)
    cases.init_perturbed(grids[0], 7)
    W = _table(2, 3)
    got, orders = [], []
    for keep_reference_order in (False, True):
        if keep_reference_order:
            monkeypatch.setenv("LUDWIG_REFERENCE_BLOCK_ORDER", "1")
        else:
            monkeypatch.delenv("LUDWIG_REFERENCE_BLOCK_ORDER", raising=False)
        d = adapt(grids[0], 0)
        monkeypatch.undo()                                               # the switch is as it was once the level exists
        orders.append(d.block_order())
        S = _lib.ModeSet([d], W)
        for t in (1, 2):
            execute_timestep_batch([d], t, 1, np.float32(0.0), params)
            S.accumulate(0, t, t - 1)
        got.append([S.download(0, m) for m in range(3)])
        S.close()
        d.close()
    assert np.array_equal(orders[1], np.arange(12)) and not np.array_equal(orders[0], orders[1]), "the two levels share one block order"
    for m, ((a, na), (b, nb)) in enumerate(zip(*got)):
        assert na == nb == 2 and np.array_equal(a.view(np.uint64), b.view(np.uint64)), m
        assert np.abs(a).max() > 0


# ---- 5. non-finite values ----
@pytest.mark.gpu
def test_non_finite_values_propagate_as_in_numpy(gpu):
    grids, params = cases.periodic_box((1, 1, 1))
    d = adapt(grids[0], 0)
    W = np.array([[1.0, 0.0, -2.0], [0.5, 3.0, -1.0]])
    S = _lib.ModeSet([d], W)
    try:
        vel = d.download("vel")
        vel[3, 4, 5, 0, 1] = np.nan
        vel[6, 1, 2, 0, 2] = np.inf
        d.upload("vel", vel)
        acc = np.zeros((3, 8, 8, 8, 1, 4))
        for row, t_sub in ((0, 1), (1, 3)):                              # odd sub-steps: the sample reads `vel`
            S.accumulate(0, t_sub, row)
            modes.host_accumulate(acc, W[row], _sample_fields(d, t_sub))
        for m in range(3):
            got, n = S.download(0, m)
            assert n == 2 and np.array_equal(got, acc[m], equal_nan=True), m
            assert np.array_equal(np.isnan(got), np.isnan(acc[m]))
        assert np.isnan(acc[1][6, 1, 2, 0, 3]) and np.isnan(acc[1][3, 4, 5, 0, 2])      # 0 x Inf and 0 x NaN
        assert np.isposinf(acc[0][6, 1, 2, 0, 3]) and np.isneginf(S.download(0, 2)[0][6, 1, 2, 0, 3])
        assert np.isnan(acc).sum() == 3 + 1 and np.isinf(acc).sum() == 2             # nowhere else
    finally:
        S.close()
        d.close()


# ---- 6. run_case end to end ----
class _Recording(case.HipStepper):
    """keeps what run_case downloads at the first window's end"""
    taken = None

    def modes_sums(self, level):
        got = super().modes_sums(level)
        type(self).taken.setdefault(level, ([a.copy() for a in got[0]], got[1]))
        return got


@pytest.mark.gpu
def test_run_case_writes_modes_and_leaves_everything_else_alone(gpu, tmp_path):
    """ball1m, 3 levels, 48 steps in batches of 8. Samples at 5, 8, ...: the first window of 8 ends at step 26, the second is unfinished
    at step 48 and writes nothing."""
    base = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}}})
    base.diag_freq, base.output_freq = 16, 24
    assert base.async_depth == 8
    stl = os.path.join(G, "ball1m.stl")
    on = copy.copy(base)
    on.fourier_modes_enabled, on.fourier_modes_start_step, on.fourier_modes_interval, on.fourier_modes_samples = True, 5, 3, 8
    on.fourier_modes_strouhal, on.fourier_modes_repeat = (0.2, 0.5), True
    both, stats_only = copy.copy(on), copy.copy(base)
    for c in (both, stats_only):
        c.statistics_enabled, c.statistics_start_step, c.statistics_interval = True, 5, 3
    d_off, d_on, d_both, d_stats = (tmp_path / n for n in ("off", "on", "both", "stats"))
    setup = pp.setup_multilevel_domain(base, stl)
    grids, params = setup[0], setup[2]
    case.run_case(base, case.HipStepper, steps=48, setup=setup, out_dir=str(d_off))
    _Recording.taken = {}
    lines = []
    case.run_case(on, _Recording, steps=48, setup=setup, out_dir=str(d_on), log=lines.append)
    taken = _Recording.taken
    case.run_case(stats_only, case.HipStepper, steps=48, setup=setup, out_dir=str(d_stats))
    case.run_case(both, case.HipStepper, steps=48, setup=setup, out_dir=str(d_both))

    assert sorted(os.listdir(d_on)) == sorted(os.listdir(d_off) + ["flow_modes_000026.vtu", "flow_modes.csv"])
    assert any("unfinished" in l and "step 29" in l for l in lines)
    for name in os.listdir(d_off):
        a, b = open(d_off / name, "rb").read(), open(d_on / name, "rb").read()
        if name == "convergence.csv":                   # Walltime and MLUPS differ from run to run
            strip = lambda t: [",".join(c for i, c in enumerate(l.split(",")) if i not in (1, 5)) for l in t.decode().splitlines()]
            assert strip(a) == strip(b)
        else:
            assert a == b, name
    means = [n for n in os.listdir(d_stats) if n.startswith("flow_mean_")]
    assert len(means) == 2 and sorted(os.listdir(d_both)) == sorted(os.listdir(d_stats) + ["flow_modes_000026.vtu", "flow_modes.csv"])
    for name in means:
        assert open(d_stats / name, "rb").read() == open(d_both / name, "rb").read(), name
    assert open(d_both / "flow_modes_000026.vtu", "rb").read() == open(d_on / "flow_modes_000026.vtu", "rb").read()

    plan = modes.plan_modes(on, params)
    m = read_vtu_with_field_data(str(d_on / "flow_modes_000026.vtu"))
    assert {k: (v.dtype, v[0]) for k, v in m["fields"].items() if k != "ModesFrequencyHz"} == {
        "ModesFirstStep": (np.int64, 5), "ModesLastStep": (np.int64, 26), "ModesSamples": (np.int64, 8), "ModesInterval": (np.int64, 3)}
    assert m["fields"]["ModesFrequencyHz"].dtype == np.float64 and tuple(m["fields"]["ModesFrequencyHz"]) == plan.frequencies_hz
    names = ["DensityMean", "VelocityMean"] + [f"{q}{kind}_{k}" for k in range(2) for kind in ("Amp", "Phase") for q in ("Density", "Velocity")]
    assert list(m["cells"]) == names + ["Obstacle", "Level"]
    sel = output.select_export_blocks([g.active_block_coords for g in grids])
    assert m["n_cells"] == 512 * len(sel) and sorted(taken) == [0, 1, 2] and all(n == 8 for _, n in taken.values())
    want = {n: [] for n in names}
    for lvl in sorted({l for l, _ in sel}):
        mean, amp, phase = modes.finalize(np.stack(taken[lvl][0]), plan.W)
        blocks = [b for l, b in sel if l == lvl]
        per = {"DensityMean": mean[..., 0:1], "VelocityMean": mean[..., 1:4]}
        for k in range(2):
            per.update({f"DensityAmp_{k}": amp[k][..., 0:1], f"VelocityAmp_{k}": amp[k][..., 1:4],
                        f"DensityPhase_{k}": phase[k][..., 0:1], f"VelocityPhase_{k}": phase[k][..., 1:4]})
        for name, a in per.items():
            a = a.astype(np.float32)[:, :, :, blocks]                     # [8,8,8,nsel,K] -> cells x fastest, block by block
            want[name].append(a.reshape((512, len(blocks), a.shape[-1]), order="F").transpose(1, 0, 2).reshape(-1, a.shape[-1]))
    for name, parts in want.items():
        got, exp = m["cells"][name], np.concatenate(parts)
        assert got.dtype == np.float32 and np.array_equal(got.reshape(exp.shape), exp, equal_nan=True), name
    assert np.abs(m["cells"]["VelocityMean"]).max() > 1e-6 and m["cells"]["VelocityAmp_0"].max() > 0
    flow = read_vtu_with_field_data(str(d_on / "flow_000024.vtu"))
    for name in ("Obstacle", "Level"):
        assert np.array_equal(m["cells"][name], flow["cells"][name])
    rows = open(d_on / "flow_modes.csv").read().splitlines()
    assert rows[0] == modes.CSV_HEADER and len(rows) == 1 + 2 * 3
    for i, line in enumerate(rows[1:]):
        k, lvl = divmod(i, 3)
        c = line.split(",")
        assert c[:6] == ["26", "5", "8", "3", "hann", str(k)] and int(c[8]) == lvl + 1
        assert float(c[6]) == pytest.approx(plan.frequencies_hz[k], rel=1e-9) and float(c[7]) == pytest.approx((0.2, 0.5)[k], rel=1e-9)
        n_fluid, energy = modes.level_energy(modes.finalize(np.stack(taken[lvl][0]), plan.W)[1][k], grids[lvl].obstacle)
        assert int(c[9]) == n_fluid == int((~np.asarray(grids[lvl].obstacle).astype(bool)).sum())
        assert float(c[10]) == pytest.approx(energy, rel=1e-9) and energy > 0
