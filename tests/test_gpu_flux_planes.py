"""Flux planes reduced on the device (ludwig_flux_planes_*, the LUDWIG_OBSERVE_FLUXES entry of ludwig_execute_timestep_batch_observed,
HipStepper.flux_planes_*, run_case's fluxes.csv and flux_boxes.csv).

The kernels evaluate the float32 expressions of open_ludwig_amd/flux_planes.py in the same order with -ffp-contract=off and add in the
same fixed tree, so every comparison is np.array_equal on the uint64 view, never a tolerance."""
import copy
import ctypes as C
import filecmp
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, flux_planes as fp, force_series as fs, preprocess as pp
from open_ludwig_amd import probes as pm, surface_stats as ss, tracers as tr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _probes_common as pcommon  # noqa: E402
import _surface_common as scommon  # noqa: E402
import _tracer_cases as tc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")
U = F32(0.05)

# the tunnel: 48 x 32 x 32 coarse cells of dx 1; level 2 (dx 0.5) covers 8..32 along every axis; the sphere (centre 19.2, 16, 16,
# radius 6.8) lies inside it
TUNNEL_PLANES = (
    pp.FluxPlane("wake", 0, 28.0, None, 0.5),                                  # behind the sphere, the full cross-section: both levels
    pp.FluxPlane("through", 0, 19.2, None, 1.0),                               # through the sphere: invalid points
    pp.FluxPlane("ragged", 0, 40.0, ((4.0, 27.0), (4.0, 27.0)), 1.0),          # 23 x 23 = 529 = one full chunk + 17, wholly on level 1
    pp.FluxPlane("one", 0, 40.0, ((3.0, 3.5), (3.0, 3.5)), 1.0),               # one point
    pp.FluxPlane("ynormal", 1, 10.0, None, 1.0),
    pp.FluxPlane("znormal", 2, 22.0, None, 1.0, -1),
    pp.FluxPlane("fine", 1, 8.9, ((10.0, 30.0), (10.0, 30.0)), 0.5),           # wholly on the finest level, under the sphere's tip
)


def _plans(grids, specs=TUNNEL_PLANES):
    return [fp.plan_flux_plane(s, grids) for s in specs]


def _state(dev):
    return [{n: d.download(n) for n in STATES} for d in dev]


def _assert_same_state(got, want, what):
    for lvl, (a, b) in enumerate(zip(got, want)):
        for n in STATES:
            assert np.array_equal(a[n], b[n]), f"{what}: level {lvl + 1} {n}"


def _host(plans, dev, t_coarse):
    """(sums [n_planes, 8], counts [n_planes]) of the restatement from the downloaded fields after coarse step t_coarse"""
    class Fields:
        @staticmethod
        def field(li, name):
            return dev[li].download(name)
    return fp.host_sample(Fields, plans, t_coarse)


def _assert_same_records(got_sums, got_counts, want_sums, want_counts, what):
    assert np.array_equal(np.asarray(got_counts), np.asarray(want_counts)), (what, got_counts, want_counts)
    a, b = np.ascontiguousarray(got_sums, dtype=np.float64), np.ascontiguousarray(want_sums, dtype=np.float64)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, np.argwhere(a.view(np.uint64) != b.view(np.uint64))[:8])


def test_the_chosen_planes_hold_the_ragged_cases():
    """on the CPU: what the device test below relies on"""
    grids, _ = cases.tunnel_with_sphere(levels=2, wall_model=True)
    assert (grids[0].grid_dim_x * 8, grids[0].grid_dim_y * 8, grids[0].grid_dim_z * 8) == (48, 32, 32) and grids[1].dx == 0.5 * grids[0].dx
    plans = {p.spec.name: p for p in _plans(grids)}
    lengths = {name: [idx.size for _, idx in p.lists()] for name, p in plans.items()}
    levels = {name: [li for li, _ in p.lists()] for name, p in plans.items()}
    every = [n for ls in lengths.values() for n in ls]
    assert any(n % 2 == 1 for n in every) and any(n > 512 for n in every) and 1 in every
    assert levels["wake"] == [0, 1] and plans["wake"].n == 64 * 64
    assert (~plans["through"].valid).sum() > 0 and plans["through"].valid.sum() > 0
    assert plans["ragged"].dims == (23, 23) and lengths["ragged"] == [529] and levels["ragged"] == [0]
    assert plans["one"].n == 1 and lengths["one"] == [1]
    assert levels["fine"] == [1] and plans["fine"].valid.all() and plans["fine"].replaced.any()
    assert plans["znormal"].spec.direction == -1 and plans["ynormal"].axes == (0, 2)


@pytest.mark.gpu
def test_device_records_equal_the_restatement_on_every_ragged_case(gpu):
    grids, params = cases.tunnel_with_sphere(levels=2, wall_model=True)
    plans = _plans(grids)
    dev = [adapt(g, 0) for g in grids]
    X = fp.DeviceFluxPlanes(plans, dev, 4)
    try:
        execute_timestep_batch(dev, 1, 4, U, params)
        X.sample(4)
        steps, sums, counts = X.download()
        assert steps.tolist() == [4] and sums.shape == (1, len(plans), 8) and counts.shape == (1, len(plans))
        want_sums, want_counts = _host(plans, dev, 4)
        assert np.abs(want_sums).min(axis=1).max() > 0 and (want_counts > 0).all()
        _assert_same_records(sums[0], counts[0], want_sums, want_counts, "sample after 4 steps")
        assert counts[0].tolist() == [int(p.valid.sum()) for p in plans]
    finally:
        X.close()
        for d in dev:
            d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2])
def test_in_batch_records_equal_samples_between_batches_and_the_flow_is_untouched(gpu, levels):
    """levels = 1: one stream; levels = 2: every level reduces on its own stream, right after its last sub-step"""
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    plans = _plans(grids)
    runs = {}
    for how in ("batch", "between", "plain"):
        dev = [adapt(g, 0) for g in grids]
        X = fp.DeviceFluxPlanes(plans, dev, 4, 2, 3) if how != "plain" else None
        try:
            if how == "between":
                for t in range(1, 7):
                    execute_timestep_batch(dev, t, 1, U, params)
                    if X.is_sample_step(t):
                        X.sample(t)
            else:
                execute_timestep_batch(dev, 1, 6, U, params, fluxes=X)
            runs[how] = (X.download() if X is not None else None, _state(dev))
        finally:
            if X is not None:
                X.close()
            for d in dev:
                d.close()
    (steps, sums, counts), state = runs["batch"]
    assert steps.tolist() == [2, 5] and np.array_equal(steps, runs["between"][0][0])
    assert len({tuple(s) for s in sums.reshape(2, -1).view(np.uint64)}) == 2          # the two samples differ: each read its own step
    _assert_same_records(sums, counts, runs["between"][0][1], runs["between"][0][2], "in-batch against between batches")
    _assert_same_state(state, runs["plain"][1], "a batch with the set against one without")
    _assert_same_state(runs["between"][1], runs["plain"][1], "batches of one against one batch")


@pytest.mark.gpu
def test_beside_the_four_other_observers_nothing_changes(gpu):
    """the four older observers plus the flux entry in one list, out of kind order: their results are those of the same list without
    the flux entry, and the flux records those of the flux entry alone"""
    lib = _lib.load()
    grids, params = cases.tunnel_with_sphere(levels=2, wall_model=True)
    fin = len(grids) - 1
    mesh, center, radius = scommon.tunnel_sphere_mesh(grids)
    sparams = scommon.tunnel_params(center, radius)
    splan = ss.plan_surface(mesh, grids[-1], sparams)
    plans = _plans(grids)
    sched = {"probes": (1, 2), "surface": (2, 1), "forces": (2, 3), "tracers": (1, 1), "fluxes": (1, 2)}
    kinds = {"probes": _lib.OBSERVE_PROBES, "surface": _lib.OBSERVE_SURFACE, "forces": _lib.OBSERVE_FORCES,
             "tracers": _lib.OBSERVE_TRACERS, "fluxes": _lib.OBSERVE_FLUXES}

    def run(order):
        dev = [adapt(g, 0) for g in grids]
        sets = {}
        try:
            if "probes" in order:
                sets["probes"] = pm.DeviceProbes(pcommon.tunnel_points(grids), dev, 8, *sched["probes"])
            if "surface" in order:
                sets["surface"] = ss.DeviceSurfaceStats(splan, dev[fin], fin, grids[fin].tau, sparams, *sched["surface"])
            if "forces" in order:
                sets["forces"] = fs.from_mesh(mesh, splan, dev[fin], fin, grids[fin].tau, sparams, *sched["forces"], 8)
            if "tracers" in order:
                sets["tracers"] = tr.DeviceTracers(dev, tc.tunnel_seeds(), tc.TUNNEL_G, tc.TUNNEL_EVERY, *sched["tracers"])
            if "fluxes" in order:
                sets["fluxes"] = fp.DeviceFluxPlanes(plans, dev, 8, *sched["fluxes"])
            obs = (_lib.BatchObserver * len(order))(*[_lib.BatchObserver(kinds[n], sets[n].handle.value, *sched[n]) for n in order])
            arr = (C.c_void_p * len(dev))(*[d.handle for d in dev])
            fl = params.to_c()
            assert lib.ludwig_execute_timestep_batch_observed(arr, len(dev), 1, 6, float(U), C.byref(fl), obs, len(order)) == 0, \
                lib.ludwig_last_error()
            out = {"state": _state(dev)}
            for n in ("probes", "surface", "forces", "fluxes"):
                if n in sets:
                    out[n] = sets[n].download()
            if "tracers" in sets:
                sets["tracers"].snapshot(6)
                out["tracers"] = sets["tracers"].download()
            return out
        finally:
            for s in sets.values():
                s.close()
            for d in dev:
                d.close()
    a = run(("tracers", "fluxes", "forces", "probes", "surface"))
    b = run(("tracers", "forces", "probes", "surface"))
    c = run(("fluxes",))
    assert np.array_equal(a["probes"][0], b["probes"][0]) and np.array_equal(a["probes"][1].view(np.uint32), b["probes"][1].view(np.uint32))
    assert a["surface"][1] == b["surface"][1] == 5 and np.array_equal(a["surface"][0].view(np.uint64), b["surface"][0].view(np.uint64))
    assert a["forces"][0].tolist() == [2, 5] and all(np.array_equal(x, y) for x, y in zip(a["forces"], b["forces"]))
    assert np.array_equal(a["forces"][1].view(np.uint64), b["forces"][1].view(np.uint64))
    assert a["tracers"][1] == b["tracers"][1] == 6
    tc.assert_same_records(a["tracers"][0], b["tracers"][0])
    assert a["fluxes"][0].tolist() == [1, 3, 5] == c["fluxes"][0].tolist()
    _assert_same_records(a["fluxes"][1], a["fluxes"][2], c["fluxes"][1], c["fluxes"][2], "beside the others against alone")
    _assert_same_state(a["state"], b["state"], "with the flux entry against without")


@pytest.mark.gpu
def test_refusals_and_ring_behaviour(gpu):
    lib = _lib.load()
    grids, params = cases.tunnel_with_sphere(levels=2, wall_model=True)
    plans = _plans(grids)
    dev, other = [adapt(g, 0) for g in grids], [adapt(g, 0) for g in grids]
    fl = params.to_c()
    X = fp.DeviceFluxPlanes(plans, dev, 2)
    Y = fp.DeviceFluxPlanes(plans, other, 2)
    E = fp.DeviceFluxPlanes([], dev, 2)                                        # n_planes = 0

    def observed(levels, t0, n, entries):
        arr = (C.c_void_p * len(levels))(*[d.handle for d in levels])
        obs = (_lib.BatchObserver * len(entries))(*entries)
        return lib.ludwig_execute_timestep_batch_observed(arr, len(levels), t0, n, float(U), C.byref(fl), obs, len(entries))

    def entry(s, start=1, interval=1):
        return _lib.BatchObserver(_lib.OBSERVE_FLUXES, s.handle.value if s is not None else None, start, interval)
    try:
        assert observed(dev, 1, 1, []) == 0
        before = _state(dev)
        assert observed(dev, 2, 1, [entry(X, 1, 0)]) == -1 and b"interval" in lib.ludwig_last_error()
        assert observed(dev, 2, 1, [entry(Y)]) == -1 and b"other levels" in lib.ludwig_last_error()
        assert observed(dev[:1], 2, 1, [entry(X)]) == -1 and b"flux planes" in lib.ludwig_last_error()
        assert observed(dev, 2, 3, [entry(X)]) == -5 and b"overflow the ring" in lib.ludwig_last_error()      # 3 records, room for 2
        assert observed(dev, 2, 1, [entry(X), entry(X)]) == -1 and b"observer" in lib.ludwig_last_error()
        assert observed(dev, 2, 1, [_lib.BatchObserver(7, X.handle.value, 1, 1)]) == -1 and b"observer" in lib.ludwig_last_error()
        _assert_same_state(_state(dev), before, "after the refusals")
        assert X.download()[0].size == 0                                       # and nothing was sampled either
        # a null set is skipped, also as a second entry; a set without planes runs and downloads nothing but its steps
        assert observed(dev, 2, 1, [entry(None, 0, 0), entry(X)]) == 0, lib.ludwig_last_error()
        assert observed(dev, 3, 1, [entry(E)]) == 0, lib.ludwig_last_error()
        steps, sums, counts = E.download()
        assert steps.tolist() == [3] and sums.shape == (1, 0, 8) and counts.shape == (1, 0)
        # the ring: one more fills it, a third is refused between batches too; the download empties it
        X.sample(3)
        with pytest.raises(_lib.LudwigError) as e:
            X.sample(3)
        assert e.value.code == -5 and b"ring full" in lib.ludwig_last_error()
        assert observed(dev, 4, 1, [entry(X)]) == -5
        steps, sums, counts = X.download()
        assert steps.tolist() == [2, 3] and (counts > 0).all()
        assert X.download()[0].size == 0
        assert observed(dev, 4, 2, [entry(X)]) == 0, lib.ludwig_last_error()
        assert X.download()[0].tolist() == [4, 5]
    finally:
        for s in (X, Y, E):
            s.close()
        for d in dev + other:
            d.close()


@pytest.mark.gpu
def test_a_plane_above_512_x_512_points_takes_the_second_combine_stage(gpu):
    (g,), params = cases.periodic_box((3, 3, 3))
    h = 23.0 / 513.5
    spec = pp.FluxPlane("big", 0, 12.3, ((0.6, 23.6), (0.6, 0.6 + 512.5 * h)), h)
    assert fp.flux_grid(spec, [g])[2] == (513, 512)
    plan = fp.plan_flux_plane(spec, [g])
    assert plan.valid.all() and plan.n == 513 * 512 > 512 * 512                # one list of 513 chunks: 513 -> 2 -> 1 records
    d = adapt(g, 0)
    X = fp.DeviceFluxPlanes([plan], [d], 1)
    try:
        execute_timestep_batch([d], 1, 2, F32(0.0), params)
        X.sample(2)
        steps, sums, counts = X.download()
        want_sums, want_counts = _host([plan], [d], 2)
        assert want_counts.tolist() == [513 * 512] and np.abs(want_sums[0, 3:6]).max() > 0
        _assert_same_records(sums[0], counts[0], want_sums, want_counts, "513 x 512 points")
    finally:
        X.close()
        d.close()


CUBE = {"basic": {"num_levels": 3, "surface_resolution": 14, "simulation": {"steps": 10, "output_freq": 8, "ramp_steps": 4}},
        "advanced": {"diagnostics": {"freq": 4},
                     "flux_planes": {"enabled": True, "start_step": 2, "interval": 1,
                                     "planes": [{"name": "wake", "normal": "x", "position": 1.5, "direction": -1}],
                                     "boxes": [{"name": "cv", "bounds": [[-1.0, 1.2], [-0.9, 0.9], [-0.8, 0.8]]}]}}}


@pytest.mark.gpu
def test_run_case_writes_what_the_host_fallback_writes(gpu, tmp_path):
    """cube1m on three levels, samples after steps 2..10 into a ring of two, so that every batch is cut into segments; the host
    fallback is the same device stepper without flux_planes_setup: flux_planes.host_sample on its downloaded fields"""
    stl = os.path.join(G, "cube1m.stl")
    cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), copy.deepcopy(CUBE))
    setup = case.setup_multilevel_domain(cfg, stl)
    calls = []

    class SmallRing(case.HipStepper):
        def flux_planes_setup(self, plans, start_step=1, interval=1, capacity=64):
            super().flux_planes_setup(plans, start_step, interval, 2)

        def batch(self, t_start, n, u_curr, params):
            calls.append((t_start, n))
            super().batch(t_start, n, u_curr, params)

    class HostFallback:
        """a HipStepper that offers no flux_planes_setup"""

        def __init__(self, grids):
            self._st = case.HipStepper(grids)

        def __getattr__(self, name):
            if name == "flux_planes_setup":
                raise AttributeError(name)
            return getattr(self._st, name)
    outs = {}
    for name, factory in (("device", SmallRing), ("host", HostFallback)):
        outs[name] = os.path.join(tmp_path, name)
        case.run_case(cfg, factory, setup=setup, out_dir=outs[name], log=lambda s: None)
    assert [a + n - 1 for a, n in calls] == [8, 10]                            # no batch was cut for a sample: only async_depth cuts
    for f in ("fluxes.csv", "flux_boxes.csv"):
        assert filecmp.cmp(os.path.join(outs["device"], f), os.path.join(outs["host"], f), shallow=False), f
    rows = open(os.path.join(outs["device"], "fluxes.csv")).read().splitlines()
    assert rows[0] == fp.FLUXES_CSV_HEADER and len(rows) == 1 + 9 * 7
    assert [int(r.split(",")[0]) for r in rows[1::7]] == list(range(2, 11)) and all(int(r.split(",")[12]) > 0 for r in rows[1:])
    boxes = open(os.path.join(outs["device"], "flux_boxes.csv")).read().splitlines()
    assert boxes[1] == fp.BOXES_CSV_HEADER and len(boxes) == 2 + 9
