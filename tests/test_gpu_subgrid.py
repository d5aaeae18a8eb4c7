"""The subgrid observer on the device (ludwig_level_subgrid_*, DeviceLevel / HipStepper.subgrid_*, run_case's EddyViscosityRatio and
the subgrid arrays of flow_mean_%06d.vtu).

The device evaluates the float32 expressions of tests/_subgrid_ref.py in the same order with -ffp-contract=off and adds the same
Float64 values in the same order, so every check against the restatement is equality of bits; NaN must meet NaN
(tests/_edge_states.assert_nan_aware_equal)."""
import copy
import os

import numpy as np
import pytest

import _subgrid_cases as sc
import _subgrid_ref as ref
from _edge_states import assert_nan_aware_equal
from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, output, preprocess as pp, statistics, subgrid
from test_gpu_statistics import read_vtu_with_field_data

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")
ERR_STATE = -5


def _check_fields(d, g, vel_name, params, what):
    nu, code = d.subgrid_fields(vel_name)
    rn, rc = ref.fields(d.download(vel_name), g.neighbor_table, g.obstacle, params.c_wale, params.nu_sgs_bg)
    assert nu.dtype == F32 and code.dtype == F32 and nu.shape == rn.shape == code.shape
    assert_nan_aware_equal(nu, rn, f"{what} {vel_name}: nu_t")
    assert_nan_aware_equal(code, rc, f"{what} {vel_name}: code")
    return nu, code


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.BOXES))
def test_uploaded_boxes_match_restatement(gpu, name):
    """planted velocities that reach every code, obstacle cells on block faces, one NaN and two infinite velocities; fields and two
    samples of the sums. One step first: a level takes c_wale and nu_sgs_background from its own step."""
    grids, params, vel = sc.uploaded_box(name)
    g = grids[0]
    d = adapt(g, 0)
    try:
        execute_timestep_batch([d], 1, 1, F32(0.0), params)
        for vel_name in ("vel", "vel_temp"):
            d.upload(vel_name, vel)
        nu, code = _check_fields(d, g, "vel", params, name)
        _check_fields(d, g, "vel_temp", params, name)
        fluid = ~g.obstacle
        assert not nu[g.obstacle].any() and not code[g.obstacle].any()
        assert np.isfinite(nu).all() and (nu[fluid] >= F32(params.nu_sgs_bg)).all()
        want_codes = (0, 1, 2) if name == "three_in_an_L" else (0, 1, 2, 3)
        assert all((code[fluid] == k).any() for k in want_codes)
        d.subgrid_stats_reset()
        sums = ref.zero_sums(g.n_blocks)
        for t_sub in (4, 7):                                   # vel_temp, then vel
            d.subgrid_stats_accumulate(t_sub)
            ref.accumulate(sums, vel, g.neighbor_table, g.obstacle, params.c_wale, params.nu_sgs_bg)
        _, s2, _ = ref.state(vel, g.neighbor_table, params.c_wale, params.nu_sgs_bg)
        for which, want in zip(("nu", "nunu", "eps"), sums):
            got, n = d.subgrid_stats_download(which)
            assert n == 2 and got.dtype == np.float64
            assert_nan_aware_equal(got, want, f"{name} S_{which}")
            if which != "eps":
                assert np.isfinite(got).all()
            else:                                              # non-finite only where |S|^2 is
                assert np.array_equal(~np.isfinite(got), ~np.isfinite(s2) & fluid) and (~np.isfinite(got)).any()
    finally:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_stepped_tunnels_match_restatement_for_both_buffers(gpu, levels):
    """Bouzidi, wall model, sponge, level edges: every level, both velocity buffers, after an odd and after an even coarse step"""
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    dev = [adapt(g, 0) for g in grids]
    try:
        for t in (1, 2, 3, 4):
            execute_timestep_batch(dev, t, 1, F32(0.05), params)
            if t < 3:
                continue
            for d, g in zip(dev, grids):
                for vel_name in ("vel", "vel_temp"):
                    nu, code = _check_fields(d, g, vel_name, params, f"step {t} level {g.level_id}")
                    assert (code == 3).any() and nu.max() > F32(params.nu_sgs_bg)
                assert g.obstacle.any() and not nu[g.obstacle].any()
    finally:
        for d in dev:
            d.close()


@pytest.mark.gpu
def test_sums_of_three_samples_equal_sequential_float64(gpu):
    """samples after coarse steps 2, 5 and 7 of a 3-level tunnel; n counted; reset zeroes; both state errors"""
    grids, params = cases.tunnel_with_sphere(levels=3, wall_model=True)
    st = case.HipStepper(grids)
    lib = _lib.load()
    try:
        buf = np.zeros((8, 8, 8, grids[0].n_blocks), np.float64, order="F")
        d0 = st.dev[0]
        assert lib.ludwig_level_subgrid_stats_download(d0.handle, 0, buf.ctypes.data, buf.nbytes, None) == ERR_STATE      # before reset
        assert lib.ludwig_level_subgrid_stats_accumulate(d0.handle, 1) == ERR_STATE
        fbuf = np.zeros((8, 8, 8, grids[0].n_blocks), F32, order="F")
        assert lib.ludwig_level_subgrid_fields_download(d0.handle, 0, fbuf.ctypes.data, fbuf.nbytes) == ERR_STATE        # before compute
        assert lib.ludwig_level_subgrid_fields_compute(d0.handle, _lib.VEL) == ERR_STATE                               # never stepped
        assert b"c_wale" in lib.ludwig_last_error()
        st.subgrid_stats_reset()
        assert lib.ludwig_level_subgrid_stats_accumulate(d0.handle, 1) == ERR_STATE                                    # never stepped
        sums = [ref.zero_sums(g.n_blocks) for g in grids]
        sampled = (2, 5, 7)
        for t in range(1, 8):
            st.batch(t, 1, F32(0.05), params)
            if t in sampled:
                st.subgrid_stats_sample(t)
                for lvl, (d, g) in enumerate(zip(st.dev, grids)):
                    t_sub = statistics.t_sub_after(lvl, t)
                    u = d.download("vel_temp" if t_sub % 2 == 0 else "vel")
                    ref.accumulate(sums[lvl], u, g.neighbor_table, g.obstacle, params.c_wale, params.nu_sgs_bg)
        for lvl, g in enumerate(grids):
            got = st.subgrid_stats_sums(lvl)
            assert got[3] == 3
            for a, want, which in zip(got[:3], sums[lvl], ("nu", "nunu", "eps")):
                assert a.dtype == np.float64 and np.array_equal(a.view(np.uint64), want.view(np.uint64)), f"level {lvl + 1} S_{which}"
            assert got[0].max() > 3 * params.nu_sgs_bg and got[2].max() > 0 and not got[0][g.obstacle].any()
        assert lib.ludwig_level_subgrid_stats_accumulate(d0.handle, -1) == -1
        assert lib.ludwig_level_subgrid_stats_download(d0.handle, 3, buf.ctypes.data, buf.nbytes, None) == -1
        assert lib.ludwig_level_subgrid_stats_download(d0.handle, 0, buf.ctypes.data, buf.nbytes - 8, None) == -1
        assert lib.ludwig_level_subgrid_fields_compute(d0.handle, _lib.RHO) == -1
        with pytest.raises(ValueError):
            d0.subgrid_fields("rho")
        st.subgrid_stats_reset()
        for lvl in range(len(grids)):
            got = st.subgrid_stats_sums(lvl)
            assert got[3] == 0 and not any(a.any() for a in got[:3])
    finally:
        st.close()
    # a level that owns no block: every call accepted, nothing computed, zeros downloaded
    ghost = copy.copy(grids[0])
    ghost.n_owned = 0
    d = adapt(ghost, 0)
    try:
        nu, code = d.subgrid_fields("vel")
        d.subgrid_stats_reset()
        d.subgrid_stats_accumulate(3)
        s, n = d.subgrid_stats_download("eps")
        assert not nu.any() and not code.any() and not s.any() and n == 0
    finally:
        d.close()


@pytest.mark.gpu
def test_bystanders_keep_their_bits(gpu):
    """the observer shares its staging with the gradient fields and runs beside the flow statistics: after subgrid calls the flow, the
    vorticity / Q-criterion and the statistics' sums equal those of a run without them"""
    grids, params = cases.tunnel_with_sphere(levels=2, wall_model=True)
    runs = []
    for observe in (False, True):
        st = case.HipStepper(grids)
        st.stats_reset()
        if observe:
            st.subgrid_stats_reset()
        for t in range(1, 5):
            st.batch(t, 1, F32(0.05), params)
            st.stats_sample(t)
            if observe:
                st.subgrid_stats_sample(t)
                for lvl in range(len(grids)):
                    st.subgrid_fields(lvl, "vel_temp" if t % 2 == 0 else "vel")
        got = []
        for lvl, g in enumerate(grids):
            one = {n: st.field(lvl, n) for n in STATES}
            one["w"], one["q"] = st.gradient_fields(lvl, "vel", F32(1.0 / g.dx))
            one["s_rho"], one["s_u"], one["s_uu"], one["n"] = st.stats_sums(lvl)
            got.append(one)
        runs.append(got)
        st.close()
    for lvl, (a, b) in enumerate(zip(*runs)):
        for k in a:
            assert np.array_equal(a[k], b[k]), f"level {lvl + 1} {k}"
        assert np.abs(a["w"]).max() > 0 and a["n"] == 4


def _cells(arr, blocks):
    return arr[:, :, :, blocks].reshape((512, len(blocks)), order="F").T.reshape(-1)


@pytest.mark.gpu
def test_run_case_writes_the_arrays_and_keeps_every_byte_with_the_keys_off(gpu, tmp_path):
    """ball1m, 3 levels, 16 steps in batches of 8; flow statistics from step 3 every 3 steps; output at 8 and 16 (even: vel_temp). One
    set-up serves the three runs: the steppers only read the host levels."""
    stl = os.path.join(G, "ball1m.stl")
    common = {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}}, "advanced": {"statistics": {"enabled": True, "start_step": 3, "interval": 3}}}

    def load(eddy=None, sgs=None):
        over = copy.deepcopy(common)
        if eddy is not None:
            over["basic"]["simulation"] = {"output_fields": {"eddy_viscosity": eddy}}
        if sgs is not None:
            over["advanced"]["statistics"]["subgrid"] = sgs
        cfg = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), over)
        cfg.diag_freq, cfg.output_freq = 8, 8
        return cfg
    holder = {}

    def keep(grids):
        holder["st"] = case.HipStepper(grids)
        holder["st"].close = lambda: None
        return holder["st"]
    dirs = {k: tmp_path / k for k in ("absent", "off", "on")}
    absent, off, on = load(), load(False, False), load(True, True)
    assert absent.async_depth == 8 and on.statistics_subgrid and "EddyViscosityRatio" in on.output_fields
    setup = pp.setup_multilevel_domain(on, stl)
    case.run_case(absent, case.HipStepper, steps=16, setup=setup, out_dir=str(dirs["absent"]))
    case.run_case(off, case.HipStepper, steps=16, setup=setup, out_dir=str(dirs["off"]))
    case.run_case(on, keep, steps=16, setup=setup, out_dir=str(dirs["on"]))
    st, grids = holder["st"], setup[0]
    try:
        names = sorted(os.listdir(dirs["absent"]))
        assert names == sorted(os.listdir(dirs["off"])) == sorted(os.listdir(dirs["on"]))
        assert {"flow_000008.vtu", "flow_000016.vtu", "flow_mean_000008.vtu", "flow_mean_000016.vtu"} <= set(names)
        for name in names:
            a, b, c = (open(dirs[k] / name, "rb").read() for k in ("absent", "off", "on"))
            if name == "convergence.csv":                   # Walltime and MLUPS differ from run to run
                strip = lambda t: [",".join(v for i, v in enumerate(l.split(",")) if i not in (1, 5)) for l in t.decode().splitlines()]
                assert strip(a) == strip(b) == strip(c)
            else:
                assert a == b, f"{name}: the keys set to false changed the file"
                if not name.startswith("flow_"):
                    assert a == c, name
        sel = output.select_export_blocks([g.active_block_coords for g in grids])
        levels = sorted({l for l, _ in sel})
        for out_step in (8, 16):
            for stem, extra in (("flow_%06d.vtu", ["EddyViscosityRatio"]), ("flow_mean_%06d.vtu", [n for n, _ in subgrid.MEAN_ARRAYS])):
                name = stem % out_step
                t_off, t_on = open(dirs["off"] / name).read(), open(dirs["on"] / name).read()
                cut = t_off.index("</CellData>")             # the same file with the new arrays after the others
                assert t_on.startswith(t_off[:cut]) and t_on.endswith(t_off[cut:])
                a, b = read_vtu_with_field_data(str(dirs["off"] / name)), read_vtu_with_field_data(str(dirs["on"] / name))
                assert list(b["cells"]) == list(a["cells"]) + extra
                assert all(b["cells"][k].dtype == F32 for k in extra)
        # the last files against the stepper's own values (the state is that of step 16; an even step: the file takes vel_temp)
        flow = read_vtu_with_field_data(str(dirs["on"] / "flow_000016.vtu"))["cells"]
        want = [_cells(subgrid.ratio_field(st.subgrid_fields(l, "vel_temp")[0], grids[l].tau), [b for lv, b in sel if lv == l]) for l in levels]
        assert np.array_equal(flow["EddyViscosityRatio"], np.concatenate(want)) and flow["EddyViscosityRatio"].max() > 0
        mean = read_vtu_with_field_data(str(dirs["on"] / "flow_mean_000016.vtu"))
        assert mean["fields"]["StatisticsSamples"][0] == 5
        want = {n: [] for n, _ in subgrid.MEAN_ARRAYS}
        for l in levels:
            sums = st.subgrid_stats_sums(l)
            assert sums[3] == 5
            fin = subgrid.finalize(*sums, subgrid.level_viscosity(grids[l].tau), on.statistics_subgrid_ck, st.statistics(l)["tke"])
            for n, k in subgrid.MEAN_ARRAYS:
                want[n].append(_cells(fin[k].astype(F32), [b for lv, b in sel if lv == l]))
        for n, parts in want.items():
            assert np.array_equal(mean["cells"][n], np.concatenate(parts)), n
        share = mean["cells"]["ResolvedTkeShare"]
        assert (share <= 1).all() and (share > 0).any() and mean["cells"]["EddyViscosityRatioMean"].max() > 0     # early in the ramp
        assert (mean["cells"]["SubgridTke"] > 0).any() and (mean["cells"]["SubgridDissipation"] > 0).any()
    finally:
        for d in st.dev:
            d.close()
