"""HIP against the CPU oracle on the edge-state catalogue (tests/_edge_states.py), NaN-aware and bit for bit over every output array.

The catalogue's host test (tests/test_edge_states_host.py) shows that each entry reaches its branch; here the device has to land on
the same bits there. The entries step through execute_timestep_batch (the A/B swap and, on 2 levels, the interface pass), on the
fast x-run instantiation (periodic boxes), GENERAL (tunnels; merged and separate launches), POST (Bouzidi), WALL, 64-bit
addressing, and with rho elided (download replays it) or stored every step.

One divergence is kept on purpose ("Non-finite states"): at a cell whose pulled set holds +-Inf, or whose
density sum overflows, the reference multiplies such values by lattice constants 0 and gets NaN, which the kernel's dropped
products do not reproduce. The test pins exactly that: differences only at those cells, and only where the oracle wrote NaN.
"""
import numpy as np
import pytest

import _edge_states as es
from open_ludwig_amd import adapt, execute_timestep_batch
from oracle import oracle

pytestmark = pytest.mark.gpu
F32 = np.float32

EXACT = [es.density_clamp, es.subnormal_state, lambda: es.nonfinite_population("nan"), lambda: es.nonfinite_population("nan", es.REST),
         es.nan_velocity_only, es.wale_branches, lambda: es.omega_clamp(0.5), lambda: es.omega_clamp(0.4999),
         es.wall_distance_edges, es.wall_umag_edges, es.wall_y_plus_edges, es.wall_model_tau_half, lambda: es.sponge_edges(True), lambda: es.sponge_edges(False),
         lambda: es.bouzidi_edges(0.001), lambda: es.bouzidi_edges(-1.0),
         *[(lambda kd=kd, t=t: es.interface_edges(kd, t)) for kd in ("parent_half", "ratio_low", "ratio_high", "nan_parent")
           for t in (True, False)]]
EXACT_IDS = ["clamp", "subnormal", "nan_k4", "nan_rest", "nan_vel", "wale", "omega_0.5", "omega_0.4999", "wall_dist", "wall_umag", "wall_y_plus", "wall_tau_half",
             "sponge_blend", "sponge_noblend", "bouzidi_list", "bouzidi_map",
             *[f"iface_{kd}_t{int(t)}" for kd in ("parent_half", "ratio_low", "ratio_high", "nan_parent") for t in (True, False)]]


def step_both(e, rho_store=False):
    dev = [adapt(g, 0) for g in e.grids]
    if rho_store:
        for d in dev:
            d.set_rho_store(True)
    f_in0 = [np.array(g.f_temp) for g in e.grids]
    execute_timestep_batch(dev, 1, e.steps, F32(e.u), e.params)
    es.run_oracle(e)
    return dev, f_in0


def compare_all(e, dev, allowed=None):
    """every output array of every level; `allowed` [8,8,8,nb] bool on level 1: cells where the oracle's NaN may be missing"""
    for i, (g, d) in enumerate(zip(e.grids, dev)):
        for name in es.output_names(i, g, e.steps):
            a, b = d.download(name), getattr(g, name)
            mask = None
            if name == "f_post_collision" and not getattr(g, "force_post_collision", False):
                from test_gpu_parity import post_collision_rows
                mask = post_collision_rows(g)
            diff = es.nan_aware_diff(a, b)
            if mask is not None:
                diff &= mask if mask.ndim == diff.ndim else mask[..., None]
            if allowed is not None and i == 0:
                cell_mask = allowed if diff.ndim == 4 else allowed[..., None]
                kept = diff & ~cell_mask
                assert not kept.any(), f"{e.name} level 1 {name}: {int(kept.sum())} elements differ outside the non-finite cells"
                assert np.isnan(b[diff]).all(), f"{e.name} {name}: a difference where the oracle did not write NaN"
            else:
                es.assert_nan_aware_equal(a, b, f"{e.name} level {i + 1} {name}", mask)
    for d in dev:
        d.close()


@pytest.mark.parametrize("build", EXACT, ids=EXACT_IDS)
def test_edge_entry_bit_exact(gpu, build):
    e = build()
    dev, _ = step_both(e)
    compare_all(e, dev)


@pytest.mark.parametrize("build", [es.density_clamp, es.subnormal_state, lambda: es.nonfinite_population("nan")],
                         ids=["clamp", "subnormal", "nan_k4"])
def test_edge_entry_with_rho_stored(gpu, build):
    e = build()
    dev, _ = step_both(e, rho_store=True)
    compare_all(e, dev)


@pytest.mark.parametrize("env", [("LUDWIG_MERGE_CLASSES", "0"), ("LUDWIG_MERGE_CLASSES", "1"), ("LUDWIG_WIDE_ADDR", "1")])
@pytest.mark.parametrize("build", [es.wall_distance_edges, es.wall_umag_edges, es.wall_y_plus_edges, lambda: es.sponge_edges(True),
                                   lambda: es.bouzidi_edges(0.001), lambda: es.interface_edges("nan_parent", True)],
                         ids=["wall_dist", "wall_umag", "wall_y_plus", "sponge", "bouzidi", "iface_nan"])
def test_edge_entry_on_other_kernel_paths(gpu, monkeypatch, env, build):
    monkeypatch.setenv(*env)
    e = build()
    dev, _ = step_both(e)
    compare_all(e, dev)


@pytest.mark.parametrize("kind", ["+inf", "-inf"])
def test_infinite_population_differs_only_where_the_reference_writes_nan(gpu, kind):
    e = es.nonfinite_population(kind)
    dev, f_in = step_both(e)
    allowed = es.nonfinite_pull_cells(e.grids[0], f_in[0])
    assert [tuple(int(i) for i in a) for a in np.argwhere(allowed)] == [e.cells["puller"]]
    compare_all(e, dev, allowed)


@pytest.mark.parametrize("tau", [1.2, 0.8])
def test_overflowed_density_differs_only_where_the_reference_writes_nan(gpu, tau):
    e = es.overflowed_rho(tau)
    dev, f_in = step_both(e)
    allowed = es.nonfinite_pull_cells(e.grids[0], f_in[0])
    assert [tuple(int(i) for i in a) for a in np.argwhere(allowed)] == [e.cells["cell"]]
    c = e.cells["cell"]
    f_dev, f_ref = dev[0].download("f"), e.grids[0].f
    compare_all(e, dev, allowed)
    # exactly the documented difference: with 1 - omega > 0 the kernel's rest population is -Inf * (-1/3) * 3 = +Inf (no 0 * -Inf term),
    # and feq + (1 - omega) * Inf = +Inf where the reference has NaN; with 1 - omega < 0 it is Inf - Inf = NaN like the reference
    diff = es.nan_aware_diff(f_dev, f_ref)
    want = [c + (es.REST,)] if tau > 1.0 else []
    assert [tuple(int(i) for i in a) for a in np.argwhere(diff)] == want
    if want:
        assert f_dev[want[0]] == np.inf and np.isnan(f_ref[want[0]])


def test_nan_set_after_one_step_on_the_device(gpu):
    """NaN in population k of cell x: exactly cell x + c_k is not finite on the device too."""
    for k in (4, es.REST, 26):
        e = es.nonfinite_population("nan", k)
        e.steps = 1
        dev, _ = step_both(e)
        f, v = dev[0].download("f"), dev[0].download("vel")
        bad = ~np.isfinite(f).all(axis=4) | ~np.isfinite(v).all(axis=4)
        assert [tuple(int(i) for i in a) for a in np.argwhere(bad)] == [e.cells["puller"]]
        for d in dev:
            d.close()


def test_device_expectations_from_the_reference(gpu):
    """The host test's reference-derived expectations, on the device directly."""
    e = es.density_clamp()
    e.steps = 1
    dev, _ = step_both(e)
    r, v = dev[0].download("rho"), dev[0].download("vel")
    for name in ("below", "exact", "negative"):
        assert r[e.cells[name]] == F32(0.01)
    for name in ("below", "exact"):
        assert (v[e.cells[name]].view(np.uint32) == 0).all()
    dev[0].close()
    e = es.subnormal_state()
    e.steps = 1
    dev, _ = step_both(e)
    assert es.is_subnormal(dev[0].download("vel")).sum() > 0
    dev[0].close()
    e = es.nan_velocity_only()
    dev, _ = step_both(e)
    assert np.isfinite(dev[0].download("f")).all()
    dev[0].close()
    for q_min in (0.001, -1.0):
        e = es.bouzidi_edges(q_min)
        e.steps = 1
        e.grids[0].force_post_collision = True
        dev, _ = step_both(e)
        fp, f = dev[0].download("f_post_collision"), dev[0].download("f")
        x, y, z, b, k = e.cells["half"]
        assert f[x, y, z, b, 26 - k] == fp[x, y, z, b, k]
        x, y, z, b, k = e.cells["one"]
        assert f[x, y, z, b, 26 - k] == F32(0.5) * fp[x, y, z, b, k] + F32(0.5) * fp[x, y, z, b, 26 - k]
        dev[0].close()


def test_readers_of_a_diverged_state(gpu):
    """One non-finite state, the readers of it: a NaN in a fluid cell next to the sphere, stepped twice so that it has spread to its
    neighbours, the obstacle cells among them. The statistics sums equal numpy float64 sums of the downloaded fields, the gradient
    fields equal tests/_gradient_ref.py, the probe series equals probes.trilinear of the downloaded fields - all NaN-aware, with NaN
    present in each. Obstacle cells next to the NaN still report velocity +0 and gradient fields +0."""
    import _gradient_ref as gref
    from open_ludwig_amd import cases, probes as pm, statistics
    grids, params = cases.tunnel_with_sphere((6, 4, 4), levels=1, wall_model=True, tau=0.5003)
    g = grids[0]
    obs = g.obstacle
    near = np.zeros_like(obs)
    near[1:-1, 1:-1, 1:-1] = ~obs[1:-1, 1:-1, 1:-1] & (obs[2:, 1:-1, 1:-1] | obs[:-2, 1:-1, 1:-1])
    x, y, z, b = (int(i) for i in np.argwhere(near)[0])
    es._both(g, "f", (x, y, z, b, es.REST), np.nan)            # the cell itself pulls it (c = 0)
    gx, gy, gz = ((int(m[b]) - 1) * 8 + c for m, c in ((g.map_x, x), (g.map_y, y), (g.map_z, z)))
    plan = pm.plan_probes([[gx + 0.75, gy + 0.6, gz + 0.55], [4.3, 5.2, 6.1]], grids)
    ref = [adapt(gg, 0) for gg in grids]
    dev = [adapt(gg, 0) for gg in grids]
    P = pm.DeviceProbes(plan, dev, 4, 1, 1)
    try:
        ref[0].stats_reset()
        acc = [None, None, None]
        want = []
        for t in (1, 2):
            execute_timestep_batch(ref, t, 1, F32(0.05), params)
            ref[0].stats_accumulate(statistics.t_sub_after(0, t))
            vel_name = "vel" if t % 2 == 1 else "vel_temp"
            rho, vel = ref[0].download("rho"), ref[0].download(vel_name)
            r, u = rho.astype(np.float64), vel.astype(np.float64)
            uu = np.stack([u[..., i] * u[..., j] for i, j in statistics.PAIRS], axis=-1)
            for k, v in enumerate((r, u, uu)):
                acc[k] = v.copy() if acc[k] is None else acc[k] + v
            want.append(pm.sample_fields(plan, lambda li: (rho, vel)))
        assert np.isnan(vel).any() and np.isnan(rho).any()
        for k, name in enumerate(("rho", "vel", "vel2")):
            got, n = ref[0].stats_download(name)
            assert n == 2
            es.assert_nan_aware_equal(got, acc[k], f"statistics {name}")
            assert np.isnan(got).any()
        w, q = ref[0].gradient_fields("vel_temp", F32(1.0))
        rw, rq = gref.gradient_fields(ref[0].download("vel_temp"), g.neighbor_table, g.obstacle, F32(1.0))
        es.assert_nan_aware_equal(w, rw, "vorticity")
        es.assert_nan_aware_equal(q, rq, "Q")
        assert np.isnan(w).any()
        # obstacle cells whose fluid neighbours hold NaN: velocity and gradient fields are +0 (all bits clear)
        nan_cell = np.isnan(vel).any(axis=4)
        touched = np.zeros_like(obs)
        touched[1:-1, 1:-1, 1:-1] = obs[1:-1, 1:-1, 1:-1] & (nan_cell[2:, 1:-1, 1:-1] | nan_cell[:-2, 1:-1, 1:-1] |
                                                             nan_cell[1:-1, 2:, 1:-1] | nan_cell[1:-1, :-2, 1:-1] |
                                                             nan_cell[1:-1, 1:-1, 2:] | nan_cell[1:-1, 1:-1, :-2])
        assert touched.any()
        assert (vel[touched].view(np.uint32) == 0).all()
        assert (w[touched].view(np.uint32) == 0).all() and (q[touched].view(np.uint32) == 0).all()
        execute_timestep_batch(dev, 1, 2, F32(0.05), params, probes=P)
        steps, got = P.download()
        assert steps.tolist() == [1, 2]
        es.assert_nan_aware_equal(got, np.stack(want), "probe series")
        assert np.isnan(got[1, 0]).any() and np.isfinite(got[:, 1]).all()
    finally:
        P.close()
        for d in ref + dev:
            d.close()
