"""Velocity-gradient fields computed on the device (ludwig_level_gradient_fields_*, DeviceLevel / HipStepper.gradient_fields, the
Vorticity / QCriterion arrays of run_case's flow file).

The device evaluates the float32 expressions of tests/_gradient_ref.py in the same order with -ffp-contract=off, so the checks
against the restatement are np.array_equal, not tolerances."""
import copy
import os

import numpy as np
import pytest

import _gradient_ref as ref
from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, output, preprocess as pp
from test_gpu_statistics import read_vtu_with_field_data

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")


def _check_level(d, g, vel_name, scale):
    w, q = d.gradient_fields(vel_name, scale)
    rw, rq = ref.gradient_fields(d.download(vel_name), g.neighbor_table, g.obstacle, scale)
    assert w.shape == rw.shape and q.shape == rq.shape and w.dtype == F32 and q.dtype == F32
    assert np.array_equal(w, rw), f"level {g.level_id} {vel_name}: vorticity"
    assert np.array_equal(q, rq), f"level {g.level_id} {vel_name}: Q"
    return w, q


@pytest.mark.gpu
def test_taylor_green_matches_restatement_and_analytic_vorticity(gpu):
    """periodic 32^3, a Taylor-Green field uploaded, no step"""
    grids, _ = cases.periodic_box((4, 4, 4), init=False)
    g = grids[0]
    gx, gy, gz = (c - 1 for c in cases.global_cell_coords(g))
    n, dx = 32, 0.37
    k = 2 * np.pi / n                                              # per cell
    a, b = 0.03, -0.02
    c = -(a + b)
    X, Y, Z = k * gx, k * gy, k * gz
    u = np.stack([a * np.cos(X) * np.sin(Y) * np.sin(Z), b * np.sin(X) * np.cos(Y) * np.sin(Z),
                  c * np.sin(X) * np.sin(Y) * np.cos(Z)], axis=-1).astype(F32)
    d = adapt(g, 0)
    try:
        d.upload("vel", np.asfortranarray(u))
        scale = F32(1.0 / dx)
        w, q = _check_level(d, g, "vel", scale)
        kk = k / dx                                                # per unit length
        exact = np.stack([(c - b) * kk * np.sin(X) * np.cos(Y) * np.cos(Z), (a - c) * kk * np.cos(X) * np.sin(Y) * np.cos(Z),
                          (b - a) * kk * np.cos(X) * np.cos(Y) * np.sin(Z)], axis=-1)
        # the central difference of a sinusoid is sin(k)/k times its derivative: truncation <= (1 - sin(k)/k) |omega|
        bound = (1 - np.sin(k) / k) * np.abs(exact).max() + 1e-6 * np.abs(exact).max()
        err = np.abs(w - exact).max()
        assert 0 < err <= bound, (err, bound)
        assert np.abs(w - np.sin(k) / k * exact).max() <= 1e-5 * np.abs(exact).max()
        assert np.abs(q).max() > 0
    finally:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_tunnel_levels_match_restatement_for_both_buffers(gpu, levels):
    """Bouzidi, wall model, sponge, level edges: every level, both velocity buffers, after a few coarse steps"""
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    dev = [adapt(g, 0) for g in grids]
    try:
        execute_timestep_batch(dev, 1, 3, F32(0.05), params)
        for d, g in zip(dev, grids):
            scale = F32(1.0 / g.dx)
            for vel_name in ("vel", "vel_temp"):
                w, q = _check_level(d, g, vel_name, scale)
                assert np.abs(w).max() > 1e-4 and np.abs(q).max() > 0
            assert g.obstacle.any() and not q[g.obstacle].any()
    finally:
        for d in dev:
            d.close()


@pytest.mark.gpu
def test_computing_does_not_perturb_the_flow(gpu):
    grids, params = cases.tunnel_with_sphere(levels=3, wall_model=True)
    runs = []
    for compute in (False, True):
        dev = [adapt(g, 0) for g in grids]
        for t in range(1, 7):
            execute_timestep_batch(dev, t, 1, F32(0.05), params)
            if compute:
                for d, g in zip(dev, grids):
                    d.gradient_fields("vel_temp" if t % 2 == 0 else "vel", F32(1.0 / g.dx))
        runs.append([{n: d.download(n) for n in STATES} for d in dev])
        for d in dev:
            d.close()
    for lvl, (a, b) in enumerate(zip(*runs)):
        for n in STATES:
            assert np.array_equal(a[n], b[n]), f"level {lvl + 1} {n}"


@pytest.mark.gpu
def test_error_and_state_paths(gpu):
    grids, _ = cases.tunnel_with_sphere(levels=1)
    g = grids[0]
    lib = _lib.load()
    d = adapt(g, 0)
    try:
        w = np.zeros((8, 8, 8, g.n_blocks, 3), F32, order="F")
        assert lib.ludwig_level_gradient_fields_download(d.handle, _lib.GRAD_VORTICITY, w.ctypes.data, w.nbytes) == -5   # before compute
        for field, scale in ((_lib.RHO, 1.0), (_lib.VEL_OLD, 1.0), (_lib.VEL, 0.0), (_lib.VEL, float("nan")), (_lib.VEL, float("inf"))):
            assert lib.ludwig_level_gradient_fields_compute(d.handle, field, scale) == -1, (field, scale)
        assert lib.ludwig_level_gradient_fields_download(d.handle, _lib.GRAD_VORTICITY, w.ctypes.data, w.nbytes) == -5
        with pytest.raises(ValueError):
            d.gradient_fields("rho", 1.0)
        assert lib.ludwig_level_gradient_fields_compute(d.handle, _lib.VEL, -2.0) == 0          # any finite non-zero scale
        assert lib.ludwig_level_gradient_fields_download(d.handle, _lib.GRAD_VORTICITY, w.ctypes.data, w.nbytes) == 0
        assert lib.ludwig_level_gradient_fields_download(d.handle, _lib.GRAD_Q, w.ctypes.data, w.nbytes) == -1                # wrong bytes
        assert lib.ludwig_level_gradient_fields_download(d.handle, 2, w.ctypes.data, w.nbytes) == -1
        assert lib.ludwig_level_gradient_fields_download(d.handle, _lib.GRAD_VORTICITY, None, w.nbytes) == -1
    finally:
        d.close()
    # a level that owns no block: both calls accepted, nothing computed, zeros downloaded
    ghost = copy.copy(g)
    ghost.n_owned = 0
    d = adapt(ghost, 0)
    try:
        assert d.info().n_owned == 0
        wv, qv = d.gradient_fields("vel", 1.0)
        assert wv.shape == (8, 8, 8, g.n_blocks, 3) and not wv.any() and not qv.any()
    finally:
        d.close()


@pytest.mark.gpu
def test_run_case_writes_vorticity_and_q_and_leaves_everything_else_alone(gpu, tmp_path):
    """ball1m, 3 levels, 24 steps in batches of 8, output every 5 steps: files at 5, 15 (odd: `vel`) and 20 (even: `vel_temp`),
    each from the state at its batch's end"""
    base = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}}})
    base.diag_freq, base.output_freq = 8, 5
    assert base.async_depth == 8
    on = copy.copy(base)
    on.output_fields = base.output_fields + ("Vorticity", "QCriterion")
    stl = os.path.join(G, "ball1m.stl")
    seen = {}

    class Recording(case.HipStepper):
        def gradient_fields(self, level, vel_name, scale):
            w, q = super().gradient_fields(level, vel_name, scale)
            seen.setdefault(self.step_of_batch, {})[level] = (vel_name, scale, w, q)
            return w, q

        def batch(self, t_start, n, u_curr, params):
            super().batch(t_start, n, u_curr, params)
            self.step_of_batch = t_start + n - 1

    d_off, d_on = tmp_path / "off", tmp_path / "on"
    case.run_case(base, case.HipStepper, steps=24, setup=pp.setup_multilevel_domain(base, stl), out_dir=str(d_off))
    setup = pp.setup_multilevel_domain(on, stl)
    grids = setup[0]
    case.run_case(on, Recording, steps=24, setup=setup, out_dir=str(d_on))
    assert sorted(os.listdir(d_on)) == sorted(os.listdir(d_off))
    assert sorted(seen) == [8, 16, 24]
    sel = output.select_export_blocks([g.active_block_coords for g in grids])
    for out_step, batch_end in ((5, 8), (15, 16), (20, 24)):
        name = "flow_%06d.vtu" % out_step
        t_off, t_on = open(d_off / name).read(), open(d_on / name).read()
        cut = t_off.index("</CellData>")                # the same file with two arrays after the others
        assert t_on.startswith(t_off[:cut]) and t_on.endswith(t_off[cut:])
        a, b = read_vtu_with_field_data(str(d_off / name)), read_vtu_with_field_data(str(d_on / name))
        assert list(b["cells"]) == list(a["cells"]) + ["Vorticity", "QCriterion"]
        for k in a["cells"]:
            assert np.array_equal(a["cells"][k], b["cells"][k]), (name, k)
        rec = seen[batch_end]
        assert sorted(rec) == sorted({l for l, _ in sel})
        want_w, want_q = [], []
        for lvl, blk in sel:
            vel_name, scale, w, q = rec[lvl]
            assert vel_name == ("vel_temp" if out_step % 2 == 0 else "vel") and scale == F32(1.0 / grids[lvl].dx)
            want_w.append(w[:, :, :, blk].reshape(512, 3, order="F"))
            want_q.append(q[:, :, :, blk].reshape(512, order="F"))
        assert b["cells"]["Vorticity"].dtype == F32
        assert np.array_equal(b["cells"]["Vorticity"], np.concatenate(want_w)), name
        assert np.array_equal(b["cells"]["QCriterion"], np.concatenate(want_q)), name
        assert np.abs(b["cells"]["Vorticity"]).max() > 0
    for name in os.listdir(d_off):
        if name.startswith("flow_"):
            continue
        x, y = open(d_off / name, "rb").read(), open(d_on / name, "rb").read()
        if name == "convergence.csv":                # Walltime and MLUPS differ from run to run
            strip = lambda t: [",".join(c for i, c in enumerate(l.split(",")) if i not in (1, 5)) for l in t.decode().splitlines()]
            assert strip(x) == strip(y)
        else:
            assert x == y, name
