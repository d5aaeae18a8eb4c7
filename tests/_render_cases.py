"""Shared cases and checks of the volume-image tests (host and device)."""
import numpy as np

import _iso_cases as ic
import _streamline_cases as sc
from open_ludwig_amd import render as rd

F32 = np.float32


def assert_same(got, want):
    """RGBA (NaN meeting NaN), end codes and sample counts, bit for bit"""
    (gr, gc, gn), (wr, wc, wn) = got, want
    assert gr.dtype == wr.dtype == F32 and gc.dtype == wc.dtype == np.int32 and gn.dtype == wn.dtype == np.int32
    assert gr.shape == wr.shape and gc.shape == wc.shape and gn.shape == wn.shape
    assert np.array_equal(gc, wc), f"codes differ at pixels {np.argwhere(gc != wc)[:8].tolist()}"
    assert np.array_equal(gn, wn), f"sample counts differ at pixels {np.argwhere(gn != wn)[:8].tolist()}"
    assert np.array_equal(gr, wr, equal_nan=True), f"rgba differ at {np.argwhere(~((gr == wr) | (np.isnan(gr) & np.isnan(wr))))[:4].tolist()}"


def view(camera, width, height, lo, hi, table, step=0.5, max_samples=4096, background=(0.1, 0.2, 0.3), body_color=(0.7, 0.6, 0.5)):
    """the keyword arguments render_host and DeviceRender.image share"""
    cam, persp = rd.Camera.build(camera, width, height).arrays()
    return dict(camera=cam, perspective=persp, width=width, height=height, step=step, lo=lo, hi=hi, max_samples=max_samples, table=table,
                background=background, body_color=body_color)


# ---- 1. 27 blocks, uploaded fields ----
BOX_ORTHO = {"type": "orthographic", "position": [-3.0, 11.3, 12.4], "look_at": [12.0, 12.1, 11.7], "up": [0.0, 0.0, 1.0], "extent": 30.0}
BOX_PERSP = {"type": "perspective", "position": [-14.0, -9.0, 31.0], "look_at": [12.0, 12.0, 12.0], "up": [0.0, 0.0, 1.0], "fov": 55.0}


def box_views():
    """a 16 x 12 orthographic and a 16 x 12 perspective view of the 24^3 box, oblique, some rays beside the box"""
    table = rd.bake_table("heat", 0.08)
    return [view(BOX_ORTHO, 16, 12, 0.0, 0.06, table), view(BOX_PERSP, 16, 12, 0.0, 0.06, table)]


# the compositing check: rays along +x from x = -3 at step 0.5 through a uniform scalar with a constant kappa; a black medium before a
# white background, so that the red channel is the transmittance itself
KAPPA = 0.0625
AXIS_CAMERA = {"type": "orthographic", "position": [-3.0, 12.0, 12.0], "look_at": [5.0, 12.0, 12.0], "up": [0.0, 0.0, 1.0], "extent": 9.0}


def axis_view():
    table = np.zeros((256, 4), F32)
    table[:, 3] = KAPPA
    return view(AXIS_CAMERA, 4, 3, 0.0, 2.0, table, background=(1.0, 1.0, 1.0))


# ---- 2. planted states on three blocks in an L: the box is [0, 16.5] x [0, 16.5] x [0, 8.5], the block at x, y in 8..16 is absent ----
PLANTED_CAMERA = {"type": "orthographic", "position": [-5.0, 8.0, 4.0], "look_at": [8.0, 8.0, 4.0], "up": [0.0, 0.0, 1.0], "extent": 12.0}
PLANTED_SIZE = (24, 16)


def planted_views():
    """24 x 16 along +x, wider than the box: thin medium; a large kappa (OPAQUE); max_samples = 8 (SAMPLES)"""
    w, h = PLANTED_SIZE
    thin, thick = rd.bake_table("coolwarm", 0.02), rd.bake_table("gray", 40.0)
    return [view(PLANTED_CAMERA, w, h, 0.98, 1.02, thin), view(PLANTED_CAMERA, w, h, 0.98, 1.02, thick),
            view(PLANTED_CAMERA, w, h, 0.98, 1.02, thin, max_samples=8)]


def planted_levels(field="density"):
    g, rho, vel, _, _ = sc.planted()
    s = rd.scalar_host(field, rho, vel, None, None)
    return g, rho, vel, rd.host_levels([g], [s])


# ---- 3. the tunnel: sphere centre (19.2, 16, 16), radius 6.8 coarse cells, level 2 from 8 to 32, level 3 from 12 to 28 ----
TUNNEL_CAMERA = {"type": "perspective", "position": [-22.0, -17.0, 43.0], "look_at": [19.2, 16.0, 16.0], "up": [0.0, 0.0, 1.0], "fov": 42.0}
TUNNEL_SIZE = (32, 24)
TUNNEL_RANGES = {"density": (0.99, 1.01), "velocity_magnitude": (0.0, 0.08), "q_criterion": (-1.0e-5, 1.0e-5),
                 "vorticity_magnitude": (0.0, 0.02)}


def tunnel_view(field):
    lo, hi = TUNNEL_RANGES[field]
    return view(TUNNEL_CAMERA, *TUNNEL_SIZE, lo, hi, rd.bake_table("coolwarm", 0.01))


def check_tunnel_rays(codes, samples, info, levels):
    """the oblique camera's rays cross every level, hit the sphere and miss the box"""
    assert (codes == rd.BODY).any() and (codes == rd.MISS).any() and (codes == rd.EXIT).any()
    assert (samples[codes == rd.MISS] == 0).all() and (samples[codes != rd.MISS] > 0).all()
    every = (1 << levels) - 1
    assert (info["levels"] == every).any(), "no ray has samples on every level"
    assert ((codes == rd.BODY) & (info["levels"] == every)).any(), "no ray reaches the sphere through every level"


def analytic_fields(grids):
    """smooth rho and u per level as functions of the position, [8,8,8,nb] and [8,8,8,nb,3] float32"""
    out = []
    for li, g in enumerate(grids):
        x = (ic.cell_centres([tuple(c) for c in np.asarray(g.active_block_coords).reshape(-1, 3)]) + 0.5) / 2.0 ** li
        rho = np.asfortranarray((1.0 + 0.001 * x[..., 0] - 0.002 * x[..., 2] + 0.0005 * np.sin(0.7 * x[..., 1])).astype(F32))
        vel = np.asfortranarray(np.stack([0.04 + 0.001 * x[..., 1], -0.002 * x[..., 0], 0.0003 * x[..., 2] * x[..., 1]], axis=-1).astype(F32))
        out.append((rho, vel))
    return out
