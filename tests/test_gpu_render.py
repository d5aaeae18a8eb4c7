"""Volume images rendered on the device (ludwig_render_*, render.DeviceRender, HipStepper.render, run_case's render_*.png).

The device evaluates the float32 expressions of open_ludwig_amd/render.py (render_host) in the same order with -ffp-contract=off, so
every check against the restatement is np.array_equal on RGBA (NaN meeting NaN), end codes and sample counts, not a tolerance."""
import copy
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import _render_cases as rc
import _streamline_cases as sc
from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, preprocess as pp, render as rd

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")


class Downloads:
    """what render.stepper_scalars asks of a stepper, from the device's own downloads"""

    def __init__(self, dev):
        self.dev = dev

    def field(self, li, name):
        return self.dev[li].download(name)

    def gradient_fields(self, li, vel_name, scale):
        return self.dev[li].gradient_fields(vel_name, scale)       # ludwig_level_gradient_fields_compute and _download


def _host(dev, grids, field, t_coarse, view, scales, info=None):
    return rd.render_host(rd.host_levels(grids, rd.stepper_scalars(Downloads(dev), grids, field, t_coarse, scales)), info=info, **view)


@pytest.mark.gpu
def test_uploaded_fields_on_27_blocks_orthographic_and_perspective(gpu):
    """uploaded fields, no step: vel holds uniform flow, vel_temp solid-body rotation; the odd coarse step reads vel, the even one
    vel_temp, so the two |u| images differ"""
    g = sc.box27()
    d = adapt(g, 0)
    r = rd.DeviceRender([d], 16 * 12)
    try:
        rho, rot = sc.rotation_fields()
        _, uni = sc.uniform_fields()
        d.upload("rho", rho)
        d.upload("vel", uni)
        d.upload("vel_temp", rot)
        scales = np.ones(1, F32)
        for view in rc.box_views():
            got = {}
            for field, t_coarse in (("velocity_magnitude", 1), ("velocity_magnitude", 2), ("density", 2)):
                r.image(t_coarse, field, scales, **view)
                got[field, t_coarse] = r.download()
                rc.assert_same(got[field, t_coarse], _host([d], [g], field, t_coarse, view, scales))
                codes = got[field, t_coarse][1]
                assert (codes == rd.EXIT).any() and (codes == rd.MISS).any()
            assert np.array_equal(got["velocity_magnitude", 1][1], got["velocity_magnitude", 2][1])
            assert not np.array_equal(got["velocity_magnitude", 1][0], got["velocity_magnitude", 2][0])
        # the compositing check of the host test, on the device
        d.upload("rho", np.ones((8, 8, 8, 27), F32, order="F"))
        r.image(0, "density", scales, **rc.axis_view())
        rgba, codes, n = r.download()
        T, alpha = F32(1.0), F32(rc.KAPPA) * F32(0.5)
        for _ in range(48):
            T = F32(T - F32(T * alpha))
        assert (codes == rd.EXIT).all() and (n == 49).all() and (rgba[..., 0] == T).all()
    finally:
        r.close()
        d.close()


@pytest.mark.gpu
def test_planted_views_reach_every_end_code(gpu):
    g, rho, vel, _ = rc.planted_levels()
    d = adapt(g, 0)
    r = rd.DeviceRender([d], 24 * 16)
    try:
        d.upload("rho", rho)
        d.upload("vel_temp", vel)
        scales = np.ones(1, F32)
        seen = set()
        for field in ("density", "velocity_magnitude"):                     # |u| holds a NaN and an infinite cell
            for view in rc.planted_views():
                r.image(0, field, scales, **view)
                got = r.download()
                rc.assert_same(got, _host([d], [g], field, 0, view, scales))
                seen |= set(got[1].ravel().tolist())
        assert seen == {rd.EXIT, rd.MISS, rd.BODY, rd.OPAQUE, rd.SAMPLES}
    finally:
        r.close()
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_tunnel_levels_match_restatement_after_3_and_4_steps(gpu, levels):
    """the locator on a real hierarchy under an oblique perspective camera: rays that cross every level, hit the sphere and miss the box;
    right after a batch whose rho store may have been elided; all four fields, Q and |omega| from the gradient fields the level computes
    with the caller's scale. A render leaves every state field as it was."""
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    dev = [adapt(g, 0) for g in grids]
    r = rd.DeviceRender(dev, rc.TUNNEL_SIZE[0] * rc.TUNNEL_SIZE[1])
    scales = rd.level_scales(grids)
    try:
        t_done = 0
        for t_coarse in (3, 4):
            execute_timestep_batch(dev, t_done + 1, t_coarse - t_done, F32(0.05), params)
            t_done = t_coarse
            before = [{n: d.download(n) for n in STATES} for d in dev]         # ahead of every image, the first gradient fields included
            images = {}
            for field in ("density", "velocity_magnitude", "q_criterion", "vorticity_magnitude"):
                r.image(t_coarse, field, scales, **rc.tunnel_view(field))
                images[field] = r.download()
            for field, got in images.items():
                info = {}
                rc.assert_same(got, _host(dev, grids, field, t_coarse, rc.tunnel_view(field), scales, info))
                rc.check_tunnel_rays(got[1], got[2], info, levels)
                assert len(np.unique(got[0][got[1] == rd.EXIT][:, 0:3], axis=0)) > 8, field        # the medium shows
            # the step before reads level 1's other velocity buffer
            r.image(t_coarse - 1, "velocity_magnitude", scales, **rc.tunnel_view("velocity_magnitude"))
            other = r.download()
            rc.assert_same(other, _host(dev, grids, "velocity_magnitude", t_coarse - 1, rc.tunnel_view("velocity_magnitude"), scales))
            assert not np.array_equal(other[0], images["velocity_magnitude"][0])
            for lvl, (d, b) in enumerate(zip(dev, before)):
                for n in STATES:
                    assert np.array_equal(d.download(n), b[n]), f"level {lvl + 1} {n}"
    finally:
        r.close()
        for d in dev:
            d.close()


@pytest.mark.gpu
def test_error_paths_and_max_pixels(gpu):
    g = sc.box27()
    lib = _lib.load()
    d = adapt(g, 0)
    arr = (C.c_void_p * 1)(d.handle)
    out = C.c_void_p()
    view = rc.box_views()[0]
    cam, table, scales = view["camera"], np.ascontiguousarray(view["table"]).reshape(-1), np.ones(1, F32)
    good = dict(t=1, which=0, sc=scales.ctypes.data, cam=cam.ctypes.data, persp=0, w=16, h=12, step=0.5, lo=0.0, hi=1.0, t_min=1 / 256,
                max_samples=64, table=table.ctypes.data)

    def image(handle, **kw):
        a = dict(good, **kw)
        par = np.array([a["step"], a["lo"], a["hi"], a["t_min"], 0, 0, 0, 0.7, 0.7, 0.7], dtype=F32)
        return lib.ludwig_render_image(handle, a["t"], a["which"], a["sc"], a["cam"], a["persp"], a["w"], a["h"], par.ctypes.data,
                                       a["max_samples"], a["table"])
    try:
        for n_levels, max_pixels in ((0, 100), (31, 100), (1, 0), (1, -5), (1, 2 ** 31)):
            assert lib.ludwig_render_create(arr, n_levels, max_pixels, C.byref(out)) == -1 and out.value is None
            assert lib.ludwig_last_error()
        r = rd.DeviceRender([d], 16 * 12)
        rgba, codes, n = np.zeros((12, 16, 4), F32), np.zeros((12, 16), np.int32), np.zeros((12, 16), np.int32)
        down = lambda nbytes=rgba.nbytes, a=rgba.ctypes.data: lib.ludwig_render_download(r.handle, a, codes.ctypes.data, n.ctypes.data, nbytes)
        assert down() == -5 and b"before" in lib.ludwig_last_error()               # LUDWIG_ERR_STATE before the first image
        nan, inf = float("nan"), float("inf")
        for kw in ({"w": 17}, {"w": 0}, {"h": 0}, {"w": -16, "h": -12}, {"w": 2 ** 16, "h": 2 ** 16}, {"step": 0.0}, {"step": -1.0},
                   {"step": nan}, {"step": inf}, {"t_min": 0.0}, {"t_min": nan}, {"t_min": inf}, {"max_samples": 0}, {"hi": 0.0},
                   {"hi": nan}, {"lo": nan}, {"which": 4}, {"which": -1}, {"t": -1}, {"persp": 2}, {"sc": None}, {"cam": None},
                   {"table": None}, {"sc": np.zeros(1, F32).ctypes.data}, {"sc": np.full(1, -1.0, F32).ctypes.data},
                   {"sc": np.full(1, nan, F32).ctypes.data}, {"sc": np.full(1, inf, F32).ctypes.data}):
            assert image(r.handle, **kw) == -1, kw                                  # LUDWIG_ERR_INVALID
            assert lib.ludwig_last_error()
        assert down() == -5                                                         # nothing was launched, nothing is there to fetch
        assert image(r.handle) == 0
        assert down(rgba.nbytes - 4) == -1 and down(a=None) == -1 and down() == 0
        assert (n[codes != rd.MISS] > 0).all() and (codes != rd.MISS).any()
        assert image(r.handle, w=4, h=4) == 0 and down() == -1 and down(4 * 4 * 16) == 0      # the last image's size counts
        r.close()
        with pytest.raises(RuntimeError, match="closed"):
            r.image(1, "density", scales, **view)
        with pytest.raises(RuntimeError, match="closed"):
            r.download()
        r = rd.DeviceRender([d], 16 * 12)
        with pytest.raises(ValueError):
            r.image(1, "pressure", scales, **view)
        with pytest.raises(ValueError):
            r.image(1, "density", np.ones(2, F32), **view)
        r.close()
    finally:
        d.close()
    # LUDWIG_ERR_STATE: a level made without block_pointer, a level that holds ghost blocks
    bare = copy.copy(g)
    bare.block_pointer = np.zeros(0, np.int32)
    ghost = copy.copy(g)
    ghost.n_owned = g.n_blocks - 3
    for host, word in ((bare, b"block_pointer"), (ghost, b"ghost")):
        d = adapt(host, 0)
        try:
            with pytest.raises(_lib.LudwigError) as e:
                rd.DeviceRender([d], 100)
            assert e.value.code == -5 and word in lib.ludwig_last_error()
        finally:
            d.close()


CUBE = {"basic": {"num_levels": 3, "surface_resolution": 14, "simulation": {"steps": 10, "output_freq": 8, "ramp_steps": 4}},
        "advanced": {"diagnostics": {"freq": 4}}}
RENDER = {"enabled": True, "start_step": 2, "interval": 3, "width": 24, "height": 16, "views": [
    {"name": "wake", "field": "velocity_magnitude", "range": [0.0, 0.02], "colormap": "heat", "opacity": 0.05,
     "camera": {"type": "perspective", "position": [-6.0, -5.0, 4.0], "look_at": [0.0, 0.0, 0.0], "up": [0, 0, 1], "fov": 40}},
    {"name": "q", "field": "q_criterion", "range": [-0.01, 0.01], "colormap": "coolwarm", "opacity": 0.5, "background": [1, 1, 1],
     "camera": {"type": "orthographic", "position": [0.2, -8.0, 0.1], "look_at": [0.2, 0.0, 0.1], "up": [0, 0, 1], "extent": 9.0}}]}


@pytest.mark.gpu
def test_run_case_writes_images_at_the_sampled_steps_and_leaves_the_rest_unchanged(gpu, tmp_path):
    """cube1m on its levels, 10 coarse steps, two views after steps 2, 5 and 8: the PNGs decode to the quantised render_host images of
    the downloaded fields, and every other output file keeps its bytes"""
    stl = os.path.join(G, "cube1m.stl")
    runs = {}
    for on in (False, True):
        over = copy.deepcopy(CUBE)
        if on:
            over["advanced"]["render"] = RENDER
        cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), over)
        setup = pp.setup_multilevel_domain(cfg, stl)
        want = {}

        class Recording(case.HipStepper):
            def render(self, plan, t_coarse):
                got = super().render(plan, t_coarse)
                host = rd.host_image(self, self.host, plan, t_coarse)
                rc.assert_same(got, host)
                want[plan.name, t_coarse] = host
                return got
        out = os.path.join(tmp_path, "on" if on else "off")
        lines = []
        case.run_case(cfg, Recording, setup=setup, out_dir=out, log=lines.append)
        runs[on] = (out, want, lines)
    off, (on, want, lines) = runs[False][0], runs[True]
    steps = [2, 5, 8]
    new = [f"render_{n}_{s:06d}.png" for n in ("wake", "q") for s in steps]
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + new)
    for name in os.listdir(off):
        if name != "convergence.csv":                                       # wall time and MLUPS columns
            assert filecmp.cmp(os.path.join(off, name), os.path.join(on, name), shallow=False), name
    assert not runs[False][1] and sorted(want) == sorted((n, s) for n in ("wake", "q") for s in steps)
    for (name, s_step), (rgba, codes, n) in want.items():
        img = rd.read_png(os.path.join(on, f"render_{name}_{s_step:06d}.png"))
        assert img.shape == (16, 24, 3) and np.array_equal(img, rd.quantise(rgba))
        assert (codes == rd.BODY).any() and (codes == rd.EXIT).any()
        logged = [l for l in lines if l.startswith(f"render {name!r}: step {s_step}:")]
        assert len(logged) == 1 and f"body {int((codes == rd.BODY).sum())}" in logged[0] and f"{int(n.sum())} samples" in logged[0]
