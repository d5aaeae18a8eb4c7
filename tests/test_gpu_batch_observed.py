"""The batch's one way in (ludwig_execute_timestep_batch_observed): a list of tagged observer entries.

Every observer launches the kernels it launched behind its own entry point, on the same streams in the same order, so every check here
is np.array_equal: all four observers in one batch give what each gives alone through ludwig_execute_timestep_batch_probes, _sampled,
_loads and _tracers, and the flow is the flow of a run that observes one set."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from open_ludwig_amd import _lib, adapt, cases, force_series as fs, probes as pm, surface_stats as ss, tracers as tr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _probes_common as pcommon  # noqa: E402
import _surface_common as scommon  # noqa: E402
import _tracer_cases as tc  # noqa: E402

F32 = np.float32
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")
U = F32(0.05)
STEPS = 6
SCHEDULES = {"probes": (1, 2), "surface": (2, 1), "forces": (2, 3), "tracers": (1, 1)}      # start_step, interval


def _state(dev):
    return [{n: d.download(n) for n in STATES} for d in dev]


def _assert_same_state(got, want, what):
    for lvl, (a, b) in enumerate(zip(got, want)):
        for n in STATES:
            assert np.array_equal(a[n], b[n]), f"{what}: level {lvl + 1} {n}"


class _Stepper:
    """fresh device levels of the tunnel with the named sets, each on its schedule of SCHEDULES"""

    def __init__(self, grids, params, plans, which):
        fin = len(grids) - 1
        self.dev = [adapt(g, 0) for g in grids]
        self.arr = (C.c_void_p * len(grids))(*[d.handle for d in self.dev])
        self.args = (self.arr, len(grids), 1, STEPS, float(U))
        self.fl = params.to_c()
        self.sets = {}
        if "probes" in which:
            self.sets["probes"] = pm.DeviceProbes(plans["probes"], self.dev, 8, *SCHEDULES["probes"])
        if "surface" in which:
            self.sets["surface"] = ss.DeviceSurfaceStats(plans["surface"], self.dev[fin], fin, grids[fin].tau, plans["sparams"], *SCHEDULES["surface"])
        if "forces" in which:
            self.sets["forces"] = fs.from_mesh(plans["mesh"], plans["surface"], self.dev[fin], fin, grids[fin].tau, plans["sparams"],
                                               *SCHEDULES["forces"], 8)
        if "tracers" in which:
            self.sets["tracers"] = tr.DeviceTracers(self.dev, plans["seeds"], tc.TUNNEL_G, tc.TUNNEL_EVERY, *SCHEDULES["tracers"])

    def entry(self, name, kind):
        return _lib.BatchObserver(kind, self.sets[name].handle.value, *SCHEDULES[name])

    def results(self):
        out = {"state": _state(self.dev)}
        if "probes" in self.sets:
            out["probes"] = self.sets["probes"].download()
        if "surface" in self.sets:
            out["surface"] = self.sets["surface"].download()
        if "forces" in self.sets:
            out["forces"] = self.sets["forces"].download()
        if "tracers" in self.sets:
            self.sets["tracers"].snapshot(STEPS)
            out["tracers"] = self.sets["tracers"].download()
        return out

    def close(self):
        for s in self.sets.values():
            s.close()
        for d in self.dev:
            d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2])
def test_four_observers_in_one_batch_equal_each_alone_through_its_old_entry_point(gpu, levels):
    """levels = 1: one stream, no events, no join; levels = 2: level streams and the tracers' join. The entries are passed out of kind
    order, with a null entry of interval 0 among them."""
    lib = _lib.load()
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    mesh, center, radius = scommon.tunnel_sphere_mesh(grids)
    sparams = scommon.tunnel_params(center, radius)
    plans = {"probes": pcommon.tunnel_points(grids), "surface": ss.plan_surface(mesh, grids[-1], sparams), "mesh": mesh, "sparams": sparams,
             "seeds": tc.tunnel_seeds()}
    assert plans["probes"].n > 0 and plans["surface"].found.sum() > 0

    def run(which, call):
        st = _Stepper(grids, params, plans, which)
        try:
            assert call(st) == 0, lib.ludwig_last_error()
            return st.results()
        finally:
            st.close()

    def observed(st):
        obs = (_lib.BatchObserver * 5)(st.entry("tracers", _lib.OBSERVE_TRACERS), st.entry("forces", _lib.OBSERVE_FORCES),
                                       _lib.BatchObserver(_lib.OBSERVE_SURFACE, None, 0, 0), st.entry("probes", _lib.OBSERVE_PROBES),
                                       st.entry("surface", _lib.OBSERVE_SURFACE))
        return lib.ludwig_execute_timestep_batch_observed(*st.args, C.byref(st.fl), obs, 5)
    a = run(("probes", "surface", "forces", "tracers"), observed)
    b1 = run(("probes",), lambda st: lib.ludwig_execute_timestep_batch_probes(*st.args, C.byref(st.fl), st.sets["probes"].handle,
                                                                              *SCHEDULES["probes"]))
    b2 = run(("surface",), lambda st: lib.ludwig_execute_timestep_batch_sampled(
        *st.args, C.byref(st.fl), C.byref(_lib.BatchSamplers(None, 0, 1, st.sets["surface"].handle.value, *SCHEDULES["surface"]))))
    b3 = run(("forces",), lambda st: lib.ludwig_execute_timestep_batch_loads(*st.args, C.byref(st.fl), None, st.sets["forces"].handle,
                                                                             *SCHEDULES["forces"]))
    b4 = run(("tracers",), lambda st: lib.ludwig_execute_timestep_batch_tracers(*st.args, C.byref(st.fl), None, None, 0, 1,
                                                                                st.sets["tracers"].handle, *SCHEDULES["tracers"]))
    steps, values = a["probes"]
    assert steps.tolist() == [1, 3, 5] and np.array_equal(steps, b1["probes"][0])
    assert np.array_equal(values.view(np.uint32), b1["probes"][1].view(np.uint32))
    sums, n = a["surface"]
    assert n == b2["surface"][1] == 5 and np.array_equal(sums.view(np.uint64), b2["surface"][0].view(np.uint64)) and np.abs(sums).max() > 0
    steps, sums, cov = a["forces"]
    assert steps.tolist() == [2, 5] and np.array_equal(steps, b3["forces"][0])
    assert np.array_equal(sums.view(np.uint64), b3["forces"][1].view(np.uint64)) and np.array_equal(cov, b3["forces"][2])
    rec, n = a["tracers"]
    assert n == b4["tracers"][1] == STEPS
    tc.assert_same_records(rec, b4["tracers"][0])
    assert (rec[:, 7] == 0).any()
    _assert_same_state(a["state"], b1["state"], "four observers against the probes alone")


@pytest.mark.gpu
def test_what_the_observer_list_itself_is_refused_for_and_what_it_may_hold(gpu):
    (g,), params = cases.periodic_box((3, 3, 3))
    lib = _lib.load()
    d, copy = adapt(g, 0), adapt(g, 0)
    fl = params.to_c()
    T = tr.DeviceTracers([d], tc.UNIFORM_SEEDS, 2, 1, 1, 1)

    def observed(level, t0, entries, n):
        obs = (_lib.BatchObserver * len(entries))(*entries) if entries is not None else None
        return lib.ludwig_execute_timestep_batch_observed((C.c_void_p * 1)(level.handle), 1, t0, 1, 0.0, C.byref(fl), obs, n)
    tracers = _lib.BatchObserver(_lib.OBSERVE_TRACERS, T.handle.value, 1, 1)
    try:
        for level in (d, copy):
            assert lib.ludwig_execute_timestep_batch((C.c_void_p * 1)(level.handle), 1, 1, 1, 0.0, C.byref(fl)) == 0
        before = _state([d])
        for entries, n in (([tracers], -1), (None, 1), ([_lib.BatchObserver(7, T.handle.value, 1, 1)], 1), ([tracers, tracers], 2)):
            assert observed(d, 2, entries, n) == -1, (entries, n)
            assert b"observer" in lib.ludwig_last_error(), lib.ludwig_last_error()
            _assert_same_state(_state([d]), before, f"refused list of {n}")
        T.snapshot(1)
        assert T.download()[1] == 0                                          # nothing was advanced either
        # no observers at all: the plain batch
        assert observed(d, 2, None, 0) == 0
        assert lib.ludwig_execute_timestep_batch((C.c_void_p * 1)(copy.handle), 1, 2, 1, 0.0, C.byref(fl)) == 0
        _assert_same_state(_state([d]), _state([copy]), "no observers against the plain batch")
        # a second entry of a kind whose set is null is no second entry
        assert observed(d, 3, [_lib.BatchObserver(_lib.OBSERVE_TRACERS, None, 0, 0), tracers], 2) == 0, lib.ludwig_last_error()
        T.snapshot(3)
        assert T.download()[1] == 1
    finally:
        T.close()
        d.close()
        copy.close()
