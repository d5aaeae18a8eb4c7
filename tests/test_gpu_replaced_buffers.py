"""Device buffers that are replaced while a level lives: work lists (set_order, and the record step's list made from them), the
iso-surface triangle buffers (grown, then reused), and observer sets made, destroyed and made again on the same level. A 32^3 periodic
box, 64 blocks, one level. Everything is bit for bit against the same thing done once on a fresh level; there is no memory-usage
assertion, free memory on a shared card is not ours to read."""
import numpy as np
import pytest

import _edge_states as es
import _surface_common as sc
from open_ludwig_amd import _lib, adapt, cases, execute_timestep_batch, flux_planes as fp, force_series as fs, order as order_mod
from open_ludwig_amd import preprocess as pp, probes as pm, slices as sl, streamlines as st, surface_stats as ss, tracers as tr
from open_ludwig_amd import wall_diagnostics as wd

pytestmark = pytest.mark.gpu
F32 = np.float32
NB = (4, 4, 4)
STATE = ("f", "f_temp", "vel", "vel_temp", "rho")


def box():
    grids, params = cases.periodic_box(NB)
    cases.init_perturbed(grids[0], 5)
    return grids, params


def orders(g):
    coords = np.asarray(g.active_block_coords)
    return order_mod.build("block_planes", coords), order_mod.build("run_per_xcd", coords)


@pytest.mark.parametrize("record", [True, False], ids=["records", "f_path"])
def test_a_second_order_steps_like_a_level_given_it_from_the_start(gpu, monkeypatch, record):
    """the record step is on by default, so the second set_order also has the record work list rebuilt"""
    if not record:
        monkeypatch.setenv("LUDWIG_RECORD_STEP", "0")
    grids, params = box()
    first, second = orders(grids[0])
    assert not np.array_equal(first, second)
    got = {}
    for how in ("replaced", "fresh"):
        dev = adapt(grids[0], 0)
        try:
            if how == "replaced":
                dev.set_order(first)
                execute_timestep_batch([dev], 1, 1, F32(0.0), params)
                dev.set_order(second)
                execute_timestep_batch([dev], 2, 3, F32(0.0), params)
            else:
                dev.set_order(second)
                execute_timestep_batch([dev], 1, 4, F32(0.0), params)
            assert dev.record_steps() == (4 if record else 0)
            got[how] = {name: dev.download(name) for name in STATE}
        finally:
            dev.close()
    for name in STATE:
        es.assert_nan_aware_equal(got["replaced"][name], got["fresh"][name], name)


def test_triangle_buffers_grow_and_are_reused(gpu):
    grids, params = box()
    dev = adapt(grids[0], 0)
    try:
        execute_timestep_batch([dev], 1, 2, F32(0.0), params)
        speed = np.linalg.norm(dev.download("vel_temp").astype(np.float64), axis=-1)
        few, more = float(np.quantile(speed, 0.995)), float(np.quantile(speed, 0.5))
        a = dev.isosurface("velocity_magnitude", few, "vel_temp")
        b = dev.isosurface("velocity_magnitude", more, "vel_temp")
        c = dev.isosurface("velocity_magnitude", few, "vel_temp")
        assert 0 < a[0] < b[0] and c[0] == a[0], (a[0], b[0], c[0])
        for x, y, name in zip(a[1:], c[1:], ("positions", "attributes", "keys")):
            es.assert_nan_aware_equal(x, y, name)
    finally:
        dev.close()


# ---- observer sets: one maker and one sampler per kind ----
def surface_plan(n_blocks, n=600, seed=3):
    """a hand-made plan: more triangles than one chunk of 512 (the force series reduces in two stages), some without a cell"""
    rng = np.random.default_rng(seed)
    found = rng.random(n) > 0.1
    blocks = np.where(found, rng.integers(0, n_blocks, n), -1).astype(np.int32)
    cells = np.where(found, rng.integers(0, 512, n), 0).astype(np.int32)
    normals = rng.standard_normal((n, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    plan = ss.SurfacePlan(found, blocks, cells, rng.uniform(0.1, 0.9, n).astype(F32), normals.astype(F32))
    return plan, rng.uniform(0.5, 1.5, n).astype(F32), rng.uniform(-4.0, 4.0, (3, n)).astype(F32)


POINTS = [[3.3, 4.2, 5.1], [30.5, 9.25, 17.75], [20.0, 8.0, 8.0], [15.9, 16.1, 24.0]]
SEEDS = np.array([[5.2, 7.3, 11.6], [3.25, 20.125, 2.9], [16.0, 16.0, 16.0]], dtype=F32)
T = 2                                                       # the state the samples read: after coarse step 2


def makers(grids, dev):
    g = grids[0]
    plan, area, arm = surface_plan(g.n_blocks)
    sparams = sc.tunnel_params((16.0, 16.0, 16.0), 5.0)
    pplan = pm.plan_probes(POINTS, grids)
    fplans = [fp.plan_flux_plane(pp.FluxPlane("x", 0, 12.0, None, 1.0), grids),
              fp.plan_flux_plane(pp.FluxPlane("z", 2, 20.0, ((4.0, 27.0), (4.0, 27.0)), 1.0), grids)]
    splans = [sl.plan_slice(pp.SlicePlane("z", 2, 16.05, ((0.2, 30.8), (0.3, 30.7)), 0.37, pp.SLICE_FIELDS), grids)]
    W = np.array([[1.0, 0.5], [0.25, -1.0]])

    def sampled(S, *calls):
        for name, args in calls:
            getattr(S, name)(*args)
        out = S.download(0, 1) if isinstance(S, _lib.ModeSet) else S.download()
        return [np.asarray(x) for x in (out if isinstance(out, (tuple, list)) else (out,))]

    return {
        "probes": (lambda: pm.DeviceProbes(pplan, [dev], 8, 1, 1), lambda S: sampled(S, ("sample", (0, T)))),
        "surface_stats": (lambda: ss.DeviceSurfaceStats(plan, dev, 0, g.tau, sparams), lambda S: sampled(S, ("accumulate", (T,)))),
        "force_series": (lambda: fs.DeviceForceSeries(plan, area, arm, dev, 0, g.tau, sparams), lambda S: sampled(S, ("sample", (T, T)))),
        "flux_planes": (lambda: fp.DeviceFluxPlanes(fplans, [dev], 4), lambda S: sampled(S, ("sample", (T,)))),
        "modes": (lambda: _lib.ModeSet([dev], W), lambda S: sampled(S, ("accumulate", (0, T, 0)))),
        "wall_surface": (lambda: wd.DeviceWallSurface(plan, dev, sparams), lambda S: sampled(S, ("compute", (T,)))),
        "slices": (lambda: sl.DeviceSlices(splans, [dev], grids), lambda S: sampled(S, ("sample", (T,)))),
        "streamlines": (lambda: st.DeviceStreamlines([dev], SEEDS, np.ones(len(SEEDS), F32), 0.5, 1.0e-6, 40),
                        lambda S: sampled(S, ("trace", (T,)))),
        "tracers": (lambda: tr.DeviceTracers([dev], SEEDS, 2, 1, 1, 1), lambda S: sampled(S, ("advance", (T,)), ("advance", (T,)), ("snapshot", (T,)))),
    }


KINDS = ("probes", "surface_stats", "force_series", "flux_planes", "modes", "wall_surface", "slices", "streamlines", "tracers")


@pytest.fixture(scope="module")
def stepped(gpu):
    """one level two steps on, shared by every kind: a set reads the level and writes only its own buffers"""
    grids, params = box()
    dev = adapt(grids[0], 0)
    execute_timestep_batch([dev], 1, T, F32(0.0), params)
    yield grids, dev
    dev.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_set_made_again_samples_like_a_set_made_once(stepped, kind):
    grids, dev = stepped
    make, sample = makers(grids, dev)[kind]
    once = make()
    try:
        want = sample(once)
    finally:
        once.close()
    make().close()
    again = make()
    try:
        got = sample(again)
    finally:
        again.close()
    assert len(got) == len(want) > 0
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.size > 0 or i > 0
        es.assert_nan_aware_equal(a, b, f"{kind} output {i}")
