"""The record step (kernels.hpp "Record step"): plain levels step from 11-float collision records instead of f / vel / rho.

Everything here is bit for bit: against the CPU oracle on periodic boxes whose run structure differs - (1,1,1) a block that is its
own neighbour in every direction, (2,1,1) a short run, (5,2,3) runs of 4 plus a lone block (both outer-face paths and the link
bits), (4,3,2) - after 1, 2, 5 and 6 steps, i.e. ending in either parity and with the last step reading populations (1) or records
(the others); and against the f path of the same binary (LUDWIG_RECORD_STEP=0) on the rough states of tests/_edge_states.py, NaN-aware
as everywhere (tests/_edge_states.py nan_aware_diff). Around the step: a download in the middle of a run, an upload after record
steps, the rho store switched on mid-run, levels the rule excludes, and a batch with an in-batch observer.
"""
import copy

import numpy as np
import pytest

import _edge_states as es
from open_ludwig_amd import adapt, cases, execute_timestep_batch, probes as pm
from oracle import oracle

pytestmark = pytest.mark.gpu
F32 = np.float32

BOXES = [(1, 1, 1), (2, 1, 1), (5, 2, 3), (4, 3, 2)]
STEPS = (1, 2, 5, 6)
INITS = ("taylor_green", "perturbed")


def make(nb, init):
    grids, params = cases.periodic_box(nb)
    if init == "perturbed":
        cases.init_perturbed(grids[0], 5)
    return grids, params


_reference = {}


def reference(nb, init):
    """the oracle's f, vel, rho after each step count of STEPS: computed once per (box, start), never changed afterwards"""
    key = (nb, init)
    if key not in _reference:
        grids, params = make(nb, init)
        out, t = {}, 0
        for n in STEPS:
            oracle.execute_timestep_batch(grids, t + 1, n - t, F32(0.0), params)
            t = n
            fn, vn = oracle.newest_buffers(0, n)
            out[n] = {"f": getattr(grids[0], fn).copy(), "vel": getattr(grids[0], vn).copy(), "rho": grids[0].rho.copy()}
            for a in out[n].values():
                a.setflags(write=False)
        _reference[key] = out
    return _reference[key]


def compare(dev, want, n, what):
    fn, vn = oracle.newest_buffers(0, n)
    for name, ref in ((fn, want["f"]), (vn, want["vel"]), ("rho", want["rho"])):
        es.assert_nan_aware_equal(dev.download(name), ref, f"{what} after {n} steps: {name}")


@pytest.mark.parametrize("init", INITS)
@pytest.mark.parametrize("nb", BOXES, ids=lambda b: "x".join(map(str, b)))
def test_record_step_equals_the_oracle(gpu, nb, init):
    want = reference(nb, init)
    for n in STEPS:
        grids, params = make(nb, init)
        dev = adapt(grids[0], 0)
        try:
            execute_timestep_batch([dev], 1, n, F32(0.0), params)
            assert dev.record_steps() == n, "a periodic box of plain cells steps by records"
            compare(dev, want[n], n, f"{nb} {init}")
        finally:
            dev.close()


def test_download_in_the_middle_then_continue(gpu):
    nb, init = (5, 2, 3), "perturbed"
    want = reference(nb, init)
    grids, params = make(nb, init)
    dev = adapt(grids[0], 0)
    try:
        execute_timestep_batch([dev], 1, 2, F32(0.0), params)
        compare(dev, want[2], 2, "first leg")              # brings populations back; the next step starts from them
        execute_timestep_batch([dev], 3, 3, F32(0.0), params)
        compare(dev, want[5], 5, "second leg")
        dev.download("rho")                                # rho alone: one parity comes back
        execute_timestep_batch([dev], 6, 1, F32(0.0), params)
        compare(dev, want[6], 6, "third leg")
        assert dev.record_steps() == 6
    finally:
        dev.close()


def test_upload_after_record_steps_is_used_by_the_next_step(gpu):
    nb = (4, 3, 2)
    grids, params = make(nb, "taylor_green")
    other, _ = make(nb, "perturbed")
    dev = adapt(grids[0], 0)
    try:
        execute_timestep_batch([dev], 1, 2, F32(0.0), params)
        oracle.execute_timestep_batch(grids, 1, 2, F32(0.0), params)
        for name in ("f", "f_temp"):                       # new populations; vel and rho stay what the two steps made of them
            getattr(grids[0], name)[...] = getattr(other[0], name)
            dev.upload(name, getattr(grids[0], name))
        execute_timestep_batch([dev], 3, 3, F32(0.0), params)
        oracle.execute_timestep_batch(grids, 3, 3, F32(0.0), params)
        fn, vn = oracle.newest_buffers(0, 5)
        compare(dev, {"f": getattr(grids[0], fn), "vel": getattr(grids[0], vn), "rho": grids[0].rho}, 5, "after the upload")
        assert dev.record_steps() == 5
    finally:
        dev.close()


def test_rho_store_switched_on_mid_run(gpu):
    nb, init = (2, 1, 1), "perturbed"
    want = reference(nb, init)
    grids, params = make(nb, init)
    dev = adapt(grids[0], 0)
    try:
        execute_timestep_batch([dev], 1, 2, F32(0.0), params)
        dev.set_rho_store(True)
        execute_timestep_batch([dev], 3, 3, F32(0.0), params)
        assert dev.record_steps() == 5                     # rho is record component 0: nothing extra to store
        compare(dev, want[5], 5, "rho stored every step")
    finally:
        dev.close()


@pytest.mark.parametrize("nb", [(1, 1, 1), (5, 2, 3)], ids=lambda b: "x".join(map(str, b)))
def test_switched_off_gives_the_same_bits(gpu, monkeypatch, nb):
    monkeypatch.setenv("LUDWIG_RECORD_STEP", "0")
    want = reference(nb, "perturbed")
    grids, params = make(nb, "perturbed")
    dev = adapt(grids[0], 0)
    try:
        execute_timestep_batch([dev], 1, 5, F32(0.0), params)
        assert dev.record_steps() == 0
        compare(dev, want[5], 5, "f path")
    finally:
        dev.close()


@pytest.mark.parametrize("order", ["0", "1"])
def test_either_launch_order_gives_the_same_bits(gpu, monkeypatch, order):
    """(8,8,1): 16 runs of 4 blocks x 8 planes = two full 8 x 8 tiles of workgroups, so LUDWIG_RECORD_ORDER=1 really transposes"""
    monkeypatch.setenv("LUDWIG_RECORD_ORDER", order)
    nb = (8, 8, 1)
    want = reference(nb, "perturbed")
    grids, params = make(nb, "perturbed")
    dev = adapt(grids[0], 0)
    try:
        execute_timestep_batch([dev], 1, 2, F32(0.0), params)
        assert dev.record_steps() == 2
        compare(dev, want[2], 2, f"record order {order}")
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ["obstacle", "sponge"])
def test_a_level_with_one_special_cell_takes_the_f_path(gpu, kind):
    grids, params = make((2, 2, 1), "perturbed")
    g = grids[0]
    if kind == "obstacle":
        g.obstacle[3, 4, 5, 1] = True
    else:
        g.sponge[3, 4, 5, 1] = F32(0.25)
    dev = adapt(g, 0)
    try:
        execute_timestep_batch([dev], 1, 3, F32(0.0), params)
        oracle.execute_timestep_batch(grids, 1, 3, F32(0.0), params)
        assert dev.record_steps() == 0
        fn, vn = oracle.newest_buffers(0, 3)
        compare(dev, {"f": getattr(g, fn), "vel": getattr(g, vn), "rho": g.rho}, 3, kind)
    finally:
        dev.close()


ROUGH = [es.density_clamp, es.subnormal_state, lambda: es.omega_clamp(0.5), lambda: es.omega_clamp(0.4999), es.wale_branches,
         es.nan_velocity_only, lambda: es.nonfinite_population("nan"), lambda: es.nonfinite_population("nan", es.REST),
         lambda: es.nonfinite_population("+inf"), lambda: es.nonfinite_population("-inf"), lambda: es.overflowed_rho(1.2),
         lambda: es.overflowed_rho(0.8)]
ROUGH_IDS = ["clamp", "subnormal", "omega_0.5", "omega_0.4999", "wale", "nan_vel", "nan_k4", "nan_rest", "+inf", "-inf", "rho_overflow_1.2",
             "rho_overflow_0.8"]


@pytest.mark.parametrize("build", ROUGH, ids=ROUGH_IDS)
def test_rough_states_equal_the_f_path(gpu, monkeypatch, build):
    """three steps each, so that what a rough cell left in its record is read back by its neighbours twice"""
    e = build()
    got = {}
    for path in ("records", "f"):
        if path == "f":
            monkeypatch.setenv("LUDWIG_RECORD_STEP", "0")
        dev = adapt(copy.deepcopy(e.grids[0]), 0)
        try:
            execute_timestep_batch([dev], 1, 3, F32(e.u), e.params)
            assert dev.record_steps() == (3 if path == "records" else 0)
            got[path] = {name: dev.download(name) for name in ("f", "f_temp", "vel", "vel_temp", "rho")}
        finally:
            dev.close()
    for name in ("f", "vel", "rho"):                        # the newest state (odd step count); f_temp / vel_temp hold step 2's
        es.assert_nan_aware_equal(got["records"][name], got["f"][name], f"{e.name} {name}")
    for name in ("f_temp", "vel_temp"):
        es.assert_nan_aware_equal(got["records"][name], got["f"][name], f"{e.name} {name} (the step before)")


def test_batch_with_probes_equals_the_f_path(gpu, monkeypatch):
    nb = (5, 2, 3)
    grids, params = make(nb, "perturbed")
    plan = pm.plan_probes([[3.3, 4.2, 5.1], [33.5, 9.25, 17.75], [20.0, 8.0, 8.0]], grids)
    got = {}
    for path in ("records", "f"):
        if path == "f":
            monkeypatch.setenv("LUDWIG_RECORD_STEP", "0")
        dev = adapt(grids[0], 0)
        P = pm.DeviceProbes(plan, [dev], 8, 1, 1)
        try:
            execute_timestep_batch([dev], 1, 2, F32(0.0), params)                  # by records (when on)
            execute_timestep_batch([dev], 3, 3, F32(0.0), params, probes=P)        # in-batch observer: the f path, from the records' state
            assert dev.record_steps() == (2 if path == "records" else 0)
            steps, series = P.download()
            assert steps.tolist() == [3, 4, 5]
            execute_timestep_batch([dev], 6, 1, F32(0.0), params)                  # and back
            assert dev.record_steps() == (3 if path == "records" else 0)
            got[path] = (series, dev.download("f_temp"), dev.download("vel_temp"), dev.download("rho"))
        finally:
            P.close()
            dev.close()
    for a, b, name in zip(got["records"], got["f"], ("probe series", "f", "vel", "rho")):
        es.assert_nan_aware_equal(a, b, name)
    want = reference(nb, "perturbed")[6]
    for a, name in zip(got["records"][1:], ("f", "vel", "rho")):
        es.assert_nan_aware_equal(a, want[name], f"{name} against the oracle")
