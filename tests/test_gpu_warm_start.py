"""Warm start on the device: ludwig_flow_source_* and ludwig_level_init_from_source against warm_start.init_host bit for bit, the
library's bookkeeping after the call against twin levels that had the same arrays uploaded, and advanced.state_files /
advanced.initial_condition through run_case. Nothing here claims that a warm-started run is close to a continued one: it is not."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _warm_start_cases as wc                             # noqa: E402
from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, preprocess as pp, streamlines as sl, warm_start as ws   # noqa: E402
from open_ludwig_amd.statistics import t_sub_after         # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDENTITY = np.array([1, 1, 1, 0, 0, 0], F32)
REST = (1.0, 0.0, 0.0, 0.0)


def close_all(*groups):
    for grp in groups:
        for d in grp:
            d.close()


def newest_levels(dev, grids, t_coarse):
    """streamlines.host_levels of downloaded fields after coarse step t_coarse"""
    def fields(li):
        return dev[li].download("rho"), dev[li].download("vel_temp" if t_sub_after(li, t_coarse) % 2 == 0 else "vel")
    return sl.host_levels(grids, fields)


def download_all(dev_level, temporal):
    names = wc.STATE_FIELDS + (wc.OLD_FIELDS if temporal else ()) + (("f_post_collision",) if dev_level.has_post_collision else ())
    return {n: dev_level.download(n) for n in names}


# ---- 1. one block onto one block ----
def test_single_block_identity_map_is_bit_identical(gpu):
    g = cases.make_level(1, [(1, 1, 1)], (1, 1, 1), 0.6, temporal=False)
    cases.init_perturbed(g, 3)
    g.obstacle[2:4, 5, 6, 0] = True
    levels = sl.host_levels([g], lambda li: (g.rho, g.vel))
    d = adapt(g, 0)
    src = ws.DeviceFlowSource(levels)
    try:
        counts = d.init_from_source(src, IDENTITY, 1.0, REST)
        res = ws.init_host(g, levels, IDENTITY, 1.0, REST)
        wc.assert_level_equals(d, res, False, "single block")
        assert counts.dtype == np.int64 and counts.tolist() == res["counts"].tolist() == [510, 0, 0, 0, 510]
        fluid = ~g.obstacle
        assert np.array_equal(d.download("rho")[fluid], g.rho[fluid]) and np.array_equal(d.download("vel")[fluid], g.vel[fluid])
    finally:
        src.close()
        d.close()


# ---- 2. every path of the kernel in one case ----
def test_nest_onto_tunnel_matches_the_restatement_bit_for_bit(gpu):
    levels = wc.planted_nest()
    grids, _ = wc.small_tunnel(levels=3, temporal=True)
    assert [g.n_blocks for g in grids] == [16, 96, 128] and all(g.obstacle.any() for g in grids)
    dev = [adapt(g, 0) for g in grids]
    src = ws.DeviceFlowSource(levels)
    outcomes, per_level = np.zeros(4, np.int64), np.zeros(2, np.int64)
    try:
        for li, (g, d) in enumerate(zip(grids, dev)):
            assert d.has_temporal_storage
            m = wc.nest_map(li)
            counts = d.init_from_source(src, m, wc.NEST_SCALE, wc.NEST_FALLBACK)
            res = ws.init_host(g, levels, m, wc.NEST_SCALE, wc.NEST_FALLBACK)
            wc.assert_level_equals(d, res, True, f"level index {li}")
            assert counts.tolist() == res["counts"].tolist(), (li, counts, res["counts"])
            assert counts[:4].sum() == (~g.obstacle).sum() and counts[4:].sum() == counts[0]
            assert np.isfinite(res["f"]).all()
            outcomes += counts[:4]
            per_level += counts[4:]
    finally:
        src.close()
        close_all(dev)
    print("outcomes", outcomes.tolist(), "found per source level", per_level.tolist())
    assert (outcomes > 0).all() and (per_level > 0).all()


# ---- 3. bookkeeping: the level is what an upload of the same arrays leaves ----
def _twin_run(grids, params, levels, maps, pre_steps, u=0.05, steps=4):
    """init_from_source on one hierarchy, ludwig_level_upload of init_host's arrays on its twin, `steps` coarse steps on both"""
    temporal = [g.f_old.size > 27 for g in grids]
    a, b = [adapt(g, 0) for g in grids], [adapt(g, 0) for g in grids]
    src = ws.DeviceFlowSource(levels)
    try:
        t = 1
        if pre_steps:
            for dev in (a, b):
                execute_timestep_batch(dev, 1, pre_steps, F32(u), params)
            t = pre_steps + 1
        for li, g in enumerate(grids):
            res = ws.init_host(g, levels, maps[li], wc.NEST_SCALE, wc.NEST_FALLBACK)
            a[li].init_from_source(src, maps[li], wc.NEST_SCALE, wc.NEST_FALLBACK)
            wc.upload_result(b[li], res, temporal[li])
        for dev in (a, b):
            execute_timestep_batch(dev, t, steps, F32(u), params)
        for li in range(len(grids)):
            fa, fb = download_all(a[li], temporal[li]), download_all(b[li], temporal[li])
            for name in fa:
                assert np.array_equal(fa[name].view(np.uint32), fb[name].view(np.uint32)), (li, name, pre_steps)
            assert np.isfinite(fa["rho"]).all()
        return [d.record_steps() for d in a], [d.record_steps() for d in b]
    finally:
        src.close()
        close_all(a, b)


@pytest.mark.parametrize("pre_steps", [0, 3])
def test_steps_after_the_call_equal_steps_after_an_upload_on_a_record_box(gpu, pre_steps):
    grids, params = cases.periodic_box((4, 4, 4))
    levels = sl.host_levels(grids, lambda li: (grids[li].rho, grids[li].vel))
    ra, rb = _twin_run(grids, params, levels, [np.array([0.75, 0.75, 0.75, 2.3, -1.1, 0.4], F32)], pre_steps, u=0.0)
    assert ra[0] > 0 and rb[0] > 0, (ra, rb)                 # the box steps by records, before and after


@pytest.mark.parametrize("pre_steps", [0, 3])
def test_steps_after_the_call_equal_steps_after_an_upload_on_a_tunnel(gpu, pre_steps):
    grids, params = wc.small_tunnel(levels=3, temporal=True)
    assert params.use_temporal_interp and grids[-1].bouzidi_enabled
    _twin_run(grids, params, wc.planted_nest(), [wc.nest_map(li) for li in range(3)], pre_steps)


# ---- 4. a source copied on the device from live levels ----
@pytest.mark.parametrize("t_coarse", [2, 3])
def test_source_from_levels_equals_a_host_built_source(gpu, t_coarse):
    grids, params = wc.small_tunnel(levels=2, temporal=True)
    live = [adapt(g, 0) for g in grids]
    a, b = [adapt(g, 0) for g in grids], [adapt(g, 0) for g in grids]
    srcs = []
    try:
        execute_timestep_batch(live, 1, t_coarse, F32(0.05), params)
        srcs.append(ws.DeviceFlowSource.from_levels(live, t_coarse))
        host_levels = newest_levels(live, grids, t_coarse)
        srcs.append(ws.DeviceFlowSource(host_levels))
        execute_timestep_batch(live, t_coarse + 1, 1, F32(0.05), params)       # the source does not alias the levels
        for li, g in enumerate(grids):
            m = np.array([2.0 ** -li] * 3 + [0.0] * 3, F32)
            ca = a[li].init_from_source(srcs[0], m, 1.0, REST)
            cb = b[li].init_from_source(srcs[1], m, 1.0, REST)
            assert ca.tolist() == cb.tolist() and ca[0] > 0
            fa, fb = download_all(a[li], True), download_all(b[li], True)
            for name in wc.STATE_FIELDS + wc.OLD_FIELDS:
                assert np.array_equal(fa[name].view(np.uint32), fb[name].view(np.uint32)), (li, name)
            wc.assert_level_equals(a[li], ws.init_host(g, host_levels, m, 1.0, REST), True, f"from_levels, level index {li}")
    finally:
        for s in srcs:
            s.close()
        close_all(live, a, b)


# ---- 5. refusals ----
def test_refusals_come_before_anything_is_written(gpu):
    lib = _lib.load()
    g = cases.make_level(1, [(1, 1, 1), (2, 1, 1)], (2, 1, 1), 0.6)
    cases.init_perturbed(g, 9)
    levels = sl.host_levels([g], lambda li: (g.rho, g.vel))
    d = adapt(g, 0)
    src = ws.DeviceFlowSource(levels)
    try:
        before = download_all(d, True)
        m, fb = IDENTITY.copy(), np.array(REST, F32)
        counts = np.full(5, -7, np.int64)

        def call(level=None, source=None, map6=m, scale=1.0, fallback=fb):
            return lib.ludwig_level_init_from_source(d.handle if level is None else level, src.handle if source is None else source,
                                                     None if map6 is None else map6.ctypes.data, float(scale),
                                                     None if fallback is None else fallback.ctypes.data, counts.ctypes.data)
        null = C.c_void_p(None)
        bad = [dict(level=null), dict(source=null), dict(map6=None), dict(fallback=None), dict(scale=np.nan), dict(scale=np.inf),
               dict(scale=0.0), dict(scale=-1.0)]
        for i in range(6):
            for v in (np.nan, np.inf):
                mm = m.copy(); mm[i] = v
                bad.append(dict(map6=mm))
        for i in range(3):
            for v in (0.0, -0.5):
                mm = m.copy(); mm[i] = v
                bad.append(dict(map6=mm))
        for i in range(4):
            ff = fb.copy(); ff[i] = np.nan
            bad.append(dict(fallback=ff))
        for kw in bad:
            assert call(**kw) == -1, kw                       # LUDWIG_ERR_INVALID
            assert lib.ludwig_last_error()
        after = download_all(d, True)
        for name in before:
            assert np.array_equal(before[name].view(np.uint32), after[name].view(np.uint32)), name
        # bad sources are refused where they are made
        h = C.c_void_p()
        dims, nb = np.array([2, 1, 1], np.int32), np.array([2], np.int32)
        bp = np.array([1, 3], np.int32)                      # entry 3 of 2 blocks
        arrs = [np.zeros(1024, np.uint8), np.ones(1024, F32), np.zeros(3072, F32)]
        tabs = [(C.c_void_p * 1)(a.ctypes.data) for a in [bp] + arrs]
        assert lib.ludwig_flow_source_create(0, 1, dims.ctypes.data, nb.ctypes.data, *tabs, C.byref(h)) == -1 and not h
        assert lib.ludwig_flow_source_create(0, 31, dims.ctypes.data, nb.ctypes.data, *tabs, C.byref(h)) == -1 and not h
        assert call() == 0 and counts.tolist() == [1024, 0, 0, 0, 1024]          # and the good call goes through
    finally:
        src.close()
        d.close()


def test_source_on_another_device_is_refused(gpu):
    if _lib.device_count() < 2:
        pytest.skip("one device visible: a source on another device cannot be made")
    g = cases.make_level(1, [(1, 1, 1)], (1, 1, 1), 0.6)
    levels = sl.host_levels([g], lambda li: (g.rho, g.vel))
    d, src = adapt(g, 0), ws.DeviceFlowSource(levels, device=1)
    try:
        before = download_all(d, True)
        with pytest.raises(_lib.LudwigError) as e:
            d.init_from_source(src, IDENTITY, 1.0, REST)
        assert e.value.code == -5                            # LUDWIG_ERR_STATE
        after = download_all(d, True)
        for name in before:
            assert np.array_equal(before[name], after[name]), name
    finally:
        src.close()
        d.close()


def test_a_level_of_ghost_copies_accepts_the_call_and_does_nothing(gpu):
    g = cases.make_level(1, [(1, 1, 1), (2, 1, 1)], (2, 1, 1), 0.6)
    cases.init_perturbed(g, 11)
    levels = sl.host_levels([g], lambda li: (g.rho, g.vel))
    g.n_owned = 0                                            # the ABI's n_owned < 0: the level only holds ghost copies here
    d = adapt(g, 0)
    src = ws.DeviceFlowSource(levels)
    try:
        before = download_all(d, True)
        assert d.init_from_source(src, IDENTITY, 0.5, REST).tolist() == [0, 0, 0, 0, 0]
        after = download_all(d, True)
        for name in before:
            assert np.array_equal(before[name].view(np.uint32), after[name].view(np.uint32)), name
    finally:
        src.close()
        d.close()


# ---- 6. run_case ----
RE266K = {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}, "simulation": {"steps": 16, "output_freq": 16}},
          "advanced": {"diagnostics": {"freq": 4}, "forces": {"series": {"enabled": True}}}}


class _Recording(case.HipStepper):
    """HipStepper that keeps what run_case asked of init_from and the fields straight after it"""
    taken = None

    def init_from(self, state, first_step, maps, vel_scale=1.0, fallback=REST):
        counts = super().init_from(state, first_step, maps, vel_scale, fallback)
        _Recording.taken = dict(state=state, first_step=first_step, maps=maps, scale=vel_scale, fallback=fallback, counts=counts,
                                fields=[{n: d.download(n) for n in ("rho", "vel", "vel_temp", "f", "f_temp")} for d in self.dev])
        return counts


def _run(tmp_path, name, over, stepper=case.HipStepper, final_fields=False):
    cfg = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), over)
    cfg.case_dir = str(tmp_path)                             # state paths are relative to the case folder
    setup = pp.setup_multilevel_domain(cfg, os.path.join(G, "ball1m.stl"))
    out, lines, kept = os.path.join(tmp_path, name), [], {}

    class Keeping(stepper):
        def close(self):
            if final_fields and self.dev and not kept:
                total = cfg.initial_condition_first_step - 1 + cfg.steps if cfg.initial_condition_state else cfg.steps
                kept["levels"] = newest_levels(self.dev, self.host, total)
            super().close()
    rows, _, params = case.run_case(cfg, Keeping, setup=setup, out_dir=out, log=lines.append)
    return cfg, setup, params, rows, out, lines, kept


def _check_warm_run(tmp_path, name, state_path, n_steps, src_name):
    over = copy.deepcopy(RE266K)
    over["basic"]["simulation"]["steps"] = n_steps
    over["advanced"]["initial_condition"] = {"state": os.path.relpath(state_path, tmp_path), "first_step": 17}
    _Recording.taken = None
    cfg, (grids, _, _, _), params, rows, out, lines, _ = _run(tmp_path, name, over, stepper=_Recording)
    got = _Recording.taken
    state = ws.load_state(state_path)
    assert got["first_step"] == 17 and got["fallback"][0] == 1.0 and got["fallback"][2:] == (0.0, 0.0)
    assert got["fallback"][1] == float(case.ramp_velocity(17, cfg.ramp_steps, cfg.u_lattice))
    assert got["scale"] == float(cfg.u_lattice) / state.u_lattice == 1.0
    count_lines = [l for l in lines if l.startswith("initial condition, level")]
    assert len(count_lines) == len(grids) == 3
    for li, g in enumerate(grids):
        m = ws.affine_map(state, g.dx, params.mesh_offset)
        assert np.array_equal(got["maps"][li], m)
        res = ws.init_host(g, state.host_levels(), m, got["scale"], got["fallback"])
        c = got["counts"][li]
        assert c.tolist() == res["counts"].tolist() and c[3] == 0 and c[0] + c[1] + c[2] == (~g.obstacle).sum() and c[0] > 0, (li, c)
        assert count_lines[li] == ws.counts_line(g.level_id, c)
        f = got["fields"][li]
        for dev_name, key in (("rho", "rho"), ("vel", "vel"), ("vel_temp", "vel"), ("f", "f"), ("f_temp", "f")):
            assert np.array_equal(f[dev_name].view(np.uint32), np.asfortranarray(res[key]).view(np.uint32)), (src_name, li, dev_name)
    # the step numbers of every file count from first_step
    assert rows and [r.step for r in rows][-1] == 16 + n_steps and all(r.step > 16 and np.isfinite(r.rho_min) for r in rows)
    series = np.loadtxt(os.path.join(out, "forces_series.csv"), delimiter=",", skiprows=1)
    assert series[:, 0].astype(int).tolist() == list(range(17, 17 + n_steps))
    conv = [l.split(",") for l in open(os.path.join(out, "convergence.csv")).read().splitlines()[1:]]
    assert [int(r[0]) for r in conv] == [r.step for r in rows]
    return rows


def test_run_case_writes_states_and_starts_from_them(gpu, tmp_path):
    """ball1m at surface_resolution 25. A: 16 steps from rest, a state every 8 steps and after the last. B: 8 steps from A's last state,
    first_step 17. C: the same from a state a coarser grid (surface_resolution 20) left after 8 steps. Nothing is asserted about how close
    B is to a continued run: the populations restart at equilibrium."""
    over = copy.deepcopy(RE266K)
    over["advanced"]["state_files"] = {"enabled": True, "interval": 8}
    cfg, (grids, _, _, _), params, rows, out, lines, kept = _run(tmp_path, "a", over, final_fields=True)
    assert sorted(n for n in os.listdir(out) if n.startswith("state_")) == ["state_000008.npz", "state_000016.npz"]
    state = ws.load_state(os.path.join(out, "state_000016.npz"))
    assert state.step == 16 and state.n_levels == 3 and state.u_lattice == float(cfg.u_lattice)
    assert np.array_equal(state.mesh_offset, np.asarray(params.mesh_offset, dtype=np.float64))
    for li, (g, (bp, obstacle, rho, vel)) in enumerate(zip(grids, kept["levels"])):
        lv = state.levels[li]
        assert lv["dx"] == g.dx and np.array_equal(lv["block_pointer"], g.block_pointer) and np.array_equal(lv["obstacle"], g.obstacle)
        assert np.array_equal(lv["rho"].view(np.uint32), rho.view(np.uint32)) and np.array_equal(lv["vel"].view(np.uint32), vel.view(np.uint32))
    _check_warm_run(tmp_path, "b", os.path.join(out, "state_000016.npz"), 8, "same grid")
    coarse = copy.deepcopy(RE266K)
    coarse["basic"]["surface_resolution"] = 20
    coarse["basic"]["simulation"]["steps"] = 8
    coarse["advanced"]["state_files"] = {"enabled": True}
    _, _, _, _, out_c, _, _ = _run(tmp_path, "coarse", coarse)
    assert sorted(n for n in os.listdir(out_c) if n.startswith("state_")) == ["state_000008.npz"]
    _check_warm_run(tmp_path, "c", os.path.join(out_c, "state_000008.npz"), 8, "coarser grid")


def test_keys_absent_every_file_keeps_its_bytes(gpu, tmp_path):
    """state files on: the run's other files are those of a run without the key (batches are cut with the batch's own inlet speed)"""
    import filecmp
    over = copy.deepcopy(RE266K)
    _, _, _, _, off, _, _ = _run(tmp_path, "off", over)
    over["advanced"]["state_files"] = {"enabled": True, "interval": 5}
    _, _, _, _, on, _, _ = _run(tmp_path, "on", over)
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + ["state_000005.npz", "state_000010.npz", "state_000015.npz", "state_000016.npz"])
    for name in os.listdir(off):
        if name != "convergence.csv":                       # wall time and MLUPS columns
            assert filecmp.cmp(os.path.join(off, name), os.path.join(on, name), shallow=False), name
