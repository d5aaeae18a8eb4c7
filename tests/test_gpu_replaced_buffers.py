"""Device buffers that are replaced while a level lives: work lists (set_order, and the record step's list made from them), the
iso-surface triangle buffers (grown, then reused), and observer sets made, destroyed and made again on the same level. A 32^3 periodic
box, 64 blocks, one level. Everything is bit for bit against the same thing done once on a fresh level; there is no memory-usage
assertion, free memory on a shared card is not ours to read."""
import numpy as np
import pytest

import _edge_states as es
from _observer_sets import KINDS, POINTS, SEEDS, T, makers, surface_plan  # noqa: F401
from open_ludwig_amd import adapt, cases, execute_timestep_batch, order as order_mod

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


# ---- observer sets: one maker and one sampler per kind (tests/_observer_sets.py) ----
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
