"""Volume images of the live flow, ray-marched on the device (no reference counterpart: the reference writes whole flow files only).

advanced.render in a case YAML lists views {name, field, range, colormap, opacity, camera, ...}; run_case renders every view every
`interval` coarse steps from `start_step` from the newest state of ALL levels and writes render_<name>_%06d.png (8-bit RGB). The device
side is ludwig_render_* (k_render): one lane per ray, one wavefront per 8 x 8 pixel tile, the streamlines' locator through every level's
dense block_pointer. This module holds the definition as a numpy restatement (sample_scalar_host, render_host: the checker), the camera,
the colour tables and the PNG files.

Definition. Everything is float32; every product, sum, quotient and sqrt is rounded on its own; only + - x / sqrt floor, ldexp (a scaling by a
power of two, exact), comparisons and int <-> float conversions appear, so the restatement matches the device bit for bit.
  * Positions are the streamlines' P: cell units of level index 0, domain frame; cell i of level index li has its centre at
    (i + 0.5) 2^-li.
  * Camera (built in float64, cast once): eye, corner (the centre of pixel (0, 0), the top-left one), du, dv (the steps per pixel column
    and row), dir (a unit vector), perspective. Pixel (i, j), column i, row j: T = (corner + (float)i du) + (float)j dv per component.
    Orthographic: O = T, D = dir. Perspective: O = eye, d = T - O, m = sqrt((dx dx + dy dy) + dz dz), D = d / m; m not > 0 or not
    finite: code MISS.
  * Box: lo = 0, hi_a = (float)(8 grid_dim_a of level index 0) + 0.5f. t0 = 0, t1 = +inf; per axis x, y, z: D_a == 0: MISS unless
    lo_a <= O_a <= hi_a; else a = (lo_a - O_a) / D_a, b = (hi_a - O_a) / D_a, t0 = fmax(t0, fmin(a, b)), t1 = fmin(t1, fmax(a, b)) (fmin
    and fmax return the other operand for a NaN). not (t0 < t1): MISS.
  * s(P) is streamlines.sample(P) applied to one per-cell scalar of the chosen level: the finest level whose active blocks hold the base
    cell (none: OUTSIDE), an obstacle base cell: OBSTACLE, weights g - floor(g), a corner outside the grid, in an absent block or in an
    obstacle cell takes the base cell's value, probes.trilinear. The scalars are isosurface.FIELDS from the same sources
    (isosurface.scalar_host): rho; |u| per cell, then interpolated; Q and |omega| of the level's gradient fields with its `scale`.
  * March: t = t0, T = 1, (R, G, B) = 0, n = 0. Loop:
        not (t < t1): code EXIT, leave;  n == max_samples: code SAMPLES, leave
        P = O + t D;  (kind, s, li) = sample(P);  n += 1;  li = 0 when OUTSIDE;  delta = step 2^-li (exact)
        OBSTACLE: shade the body, code BODY, leave
        found and s == s (a NaN value adds nothing):
            x = fmin(fmax((s - lo) inv, 0), 1), inv = 1 / (hi - lo);  (r, g, b, kappa) = table[(int)(x 255 + 0.5)]
            alpha = fmin(kappa delta, 1);  w = T alpha;  R = R + w r (G, B alike);  T = T - w;  T < t_min: code OPAQUE, leave
        t = t + delta
    After leaving, unless BODY: R = R + T bg_r (G, B alike). A = 1 - T.
  * Body: o(e) = 1 if the base cell's face neighbour at e on its own level is an obstacle cell of an active block, else 0 (outside the
    grid or an absent block: 0). n_a = o(-e_a) - o(+e_a), nn = n.n. nn == 0: shade = 1; else c = -((n_x D_x + n_y D_y) + n_z D_z) /
    sqrt((float)nn), shade = 0.3 + 0.7 fmax(c, 0): a headlight on a voxel normal. R = R + T (body_r shade) (G, B alike), then T = 0.
  * Table: 256 entries (r, g, b, kappa), kappa an extinction per coarse cell length, baked from control points [x, r, g, b, opacity] by
    linear interpolation in float64 at x = k / 255 (bake_table).
  * State: every level's newest state after coarse step t_coarse (statistics.t_sub_after), as for the streamlines.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
import zlib
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import statistics as stats_mod
from ._lib import Handle
from .blocks import BLOCK_SIZE
from .isosurface import check_field, scalar_host
from .probes import trilinear

F32 = np.float32
EXIT, MISS, BODY, OPAQUE, SAMPLES = 0, 1, 2, 3, 4
CODE_NAMES = ("exit", "miss", "body", "opaque", "max_samples")
FOUND, OUTSIDE, OBSTACLE = 0, 1, 2
T_MIN = 1.0 / 256.0                               # a ray ends as OPAQUE once its transmittance falls below this
CAMERA_TYPES = ("orthographic", "perspective")


# ---- camera ----
class Camera:
    """eye, corner, du, dv, dir in float64, in the frame its points were given in; arrays() is what the kernel takes"""

    def __init__(self, eye, corner, du, dv, direction, perspective: bool, width: int, height: int):
        self.eye, self.corner, self.du, self.dv, self.dir = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, corner, du, dv, direction))
        self.perspective, self.width, self.height = bool(perspective), int(width), int(height)

    @classmethod
    def build(cls, spec: dict, width: int, height: int, offset=(0.0, 0.0, 0.0), scale: float = 1.0, where: str = "camera") -> "Camera":
        """spec {type: orthographic | perspective, position, look_at, up, fov | extent}: fov the vertical field of view in degrees,
        extent the image's height in the points' units. Points are moved by `offset` and divided by `scale` (and extent with them), all in
        float64. Row 0 is the top row, column 0 the left one, seen along the view direction with `up` upwards. ValueError names `where`."""
        if not isinstance(spec, dict):
            raise ValueError(f"{where} must be a mapping")
        kind = str(spec.get("type", "perspective"))
        if kind not in CAMERA_TYPES:
            raise ValueError(f"{where}.type {kind!r} is unknown (one of {', '.join(CAMERA_TYPES)})")
        allowed = ("type", "position", "look_at", "up", "extent" if kind == "orthographic" else "fov")
        for key in spec:
            if key not in allowed:
                raise ValueError(f"{where}.{key} is no key of a camera of type {kind} (one of {', '.join(allowed)})")
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError(f"{where}: an image of {width} x {height} pixels")
        vec = {}
        for key, default in (("position", None), ("look_at", None), ("up", (0.0, 0.0, 1.0))):
            v = spec.get(key, default)
            if v is None:
                raise ValueError(f"{where}.{key} is missing")
            try:
                v = np.asarray(v, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"{where}.{key} must be [x, y, z]") from None
            if v.shape != (3,) or not np.isfinite(v).all():
                raise ValueError(f"{where}.{key} must be three finite numbers")
            vec[key] = v
        off, scale = np.asarray(offset, dtype=np.float64).reshape(3), float(scale)
        eye, at = (vec["position"] + off) / scale, (vec["look_at"] + off) / scale
        f = at - eye
        if not np.linalg.norm(f) > 0.0:
            raise ValueError(f"{where}.look_at must differ from {where}.position")
        f = f / np.linalg.norm(f)
        r = np.cross(f, vec["up"])
        if not np.linalg.norm(r) > 1.0e-12 * np.linalg.norm(vec["up"]) or not np.linalg.norm(vec["up"]) > 0.0:
            raise ValueError(f"{where}.up must not be parallel to the view direction")
        r = r / np.linalg.norm(r)
        u = np.cross(r, f)
        key = "extent" if kind == "orthographic" else "fov"
        try:
            size = float(spec.get(key, 40.0 if key == "fov" else "nan"))
        except (TypeError, ValueError):
            raise ValueError(f"{where}.{key} must be a number") from None
        if kind == "orthographic":
            if not (math.isfinite(size) and size > 0.0):
                raise ValueError(f"{where}.extent must be positive and finite, got {size}")
            px = size / scale / height
            centre = eye
        else:
            if not (0.0 < size < 180.0):
                raise ValueError(f"{where}.fov must lie in (0, 180) degrees, got {size}")
            px = 2.0 * math.tan(math.radians(size) / 2.0) / height
            centre = eye + f
        corner = centre + ((0.5 - width / 2.0) * px) * r - ((0.5 - height / 2.0) * px) * u
        return cls(eye, corner, px * r, -px * u, f, kind == "perspective", width, height)

    def ray(self, i, j) -> Tuple[np.ndarray, np.ndarray]:
        """origin and unit direction (float64) of the ray through column i, row j (fractions allowed)"""
        t = self.corner + float(i) * self.du + float(j) * self.dv
        if not self.perspective:
            return t, self.dir.copy()
        d = t - self.eye
        return self.eye.copy(), d / np.linalg.norm(d)

    def arrays(self) -> Tuple[np.ndarray, int]:
        """(16 float32: eye, corner, du, dv, dir, 0; perspective as 0 or 1): the one cast"""
        return np.concatenate([self.eye, self.corner, self.du, self.dv, self.dir, [0.0]]).astype(F32), int(self.perspective)


# ---- colour tables ----
PRESETS = {
    # [x, r, g, b, opacity]; every channel of gray and heat and the opacity of both rise with x; coolwarm's red never falls and its blue never rises,
    # its opacity is lowest in the middle
    "gray": [[0.0, 0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0, 1.0]],
    "heat": [[0.0, 0.0, 0.0, 0.0, 0.0], [0.4, 0.8, 0.0, 0.0, 0.2], [0.8, 1.0, 0.8, 0.0, 0.6], [1.0, 1.0, 1.0, 1.0, 1.0]],
    "coolwarm": [[0.0, 0.1, 0.3, 0.9, 1.0], [0.5, 0.9, 0.9, 0.9, 0.0], [1.0, 0.9, 0.3, 0.1, 1.0]],
}


def control_points(colormap, where: str = "colormap") -> np.ndarray:
    """a preset's name or a list of [x, r, g, b, opacity] -> [n, 5] float64, x strictly rising from 0 to 1. ValueError names `where`."""
    if isinstance(colormap, str):
        if colormap not in PRESETS:
            raise ValueError(f"{where} {colormap!r} is unknown (one of {', '.join(PRESETS)}, or a list of [x, r, g, b, opacity])")
        return np.asarray(PRESETS[colormap], dtype=np.float64)
    try:
        p = np.asarray(colormap, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{where} must be a preset's name or a list of [x, r, g, b, opacity]") from None
    if p.ndim != 2 or p.shape[1] != 5 or p.shape[0] < 2 or not np.isfinite(p).all():
        raise ValueError(f"{where} must hold at least two finite control points [x, r, g, b, opacity]")
    if p[0, 0] != 0.0 or p[-1, 0] != 1.0 or not (np.diff(p[:, 0]) > 0.0).all():
        raise ValueError(f"{where}: x must rise strictly from 0 to 1")
    if (p[:, 1:] < 0.0).any():
        raise ValueError(f"{where}: colours and opacities must be >= 0")
    return p


def bake_table(colormap, opacity: float = 1.0) -> np.ndarray:
    """[256, 4] float32 (r, g, b, kappa): the control points interpolated linearly in float64 at x = k / 255, kappa = opacity times the
    points' opacity, cast once"""
    p = control_points(colormap)
    x = np.arange(256, dtype=np.float64) / 255.0
    out = np.stack([np.interp(x, p[:, 0], p[:, 1 + k]) for k in range(4)], axis=1)
    out[:, 3] *= float(opacity)
    return out.astype(F32)


# ---- the numpy restatement of k_render ----
def host_levels(grids: Sequence, scalars: Sequence[np.ndarray]) -> List[tuple]:
    """what sample_scalar_host reads of every level, level index 0 first: (block_pointer [gx, gy, gz] 1-based, obstacle [8,8,8,nb]
    bool, scalar [8,8,8,nb] float32)"""
    return [(np.asarray(g.block_pointer), np.asarray(g.obstacle).astype(bool), np.asarray(s, dtype=F32)) for g, s in zip(grids, scalars)]


def stepper_scalars(stepper, grids, field: str, t_coarse: int, scales=None) -> List[np.ndarray]:
    """the scalar `field` of every level's newest state after coarse step t_coarse from a stepper's downloads: field(level, name), and
    gradient_fields(level, vel name, scale) for Q / vorticity; scales default to 1 / dx of the level"""
    check_field(field)
    out = []
    for li, g in enumerate(grids):
        vel_name = "vel_temp" if stats_mod.t_sub_after(li, t_coarse) % 2 == 0 else "vel"
        rho = vel = vort = q = None
        if field == "density":
            rho = stepper.field(li, "rho")
        elif field == "velocity_magnitude":
            vel = stepper.field(li, vel_name)
        else:
            vort, q = stepper.gradient_fields(li, vel_name, F32(1.0 / g.dx) if scales is None else F32(scales[li]))
        out.append(scalar_host(field, rho, vel, vort, q))
    return out


def level_scales(grids) -> np.ndarray:
    """1 / dx per level in float32: the gradient fields' scale of the flow file"""
    return np.array([F32(1.0 / g.dx) for g in grids], dtype=F32)


def _block(bp: np.ndarray, i: np.ndarray) -> np.ndarray:
    """0-based block of the cells i [n, 3] (int64) of a level, -1: outside the grid or no block there"""
    B = BLOCK_SIZE
    b = np.full(i.shape[0], -1, np.int64)
    if bp.size == 0:
        return b
    dims = np.array(bp.shape, dtype=np.int64).reshape(3)
    inside = ((i >= 0) & (i < B * dims)).all(axis=1)
    b[inside] = bp[i[inside, 0] // B, i[inside, 1] // B, i[inside, 2] // B].astype(np.int64) - 1
    return b


def _cell_values(a: np.ndarray, i: np.ndarray, b: np.ndarray) -> np.ndarray:
    B = BLOCK_SIZE
    return a[i[:, 0] % B, i[:, 1] % B, i[:, 2] % B, b]


def sample_scalar_host(P: np.ndarray, levels: Sequence[tuple]):
    """sample(P) of the definition for P [n, 3] float32 -> (kind [n] int32: 0 found, 1 outside, 2 obstacle; value [n] float32, NaN where
    kind != 0; level index [n] int32, -1: none; base cell [n, 3] int64 and its block [n] int64, 0 and -1 where outside)"""
    P = np.asarray(P, dtype=F32).reshape(-1, 3)
    n = P.shape[0]
    kind = np.full(n, OUTSIDE, np.int32)
    value = np.full(n, np.nan, F32)
    level = np.full(n, -1, np.int32)
    base = np.zeros((n, 3), np.int64)
    block = np.full(n, -1, np.int64)
    todo = np.ones(n, bool)
    B = BLOCK_SIZE
    for li in range(len(levels) - 1, -1, -1):
        idx = np.flatnonzero(todo)
        if idx.size == 0:
            break
        bp, obstacle, s = levels[li]
        dims = np.array(bp.shape, dtype=np.int64).reshape(3) if bp.size else np.zeros(3, np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            g = P[idx] * F32(2.0 ** li) - F32(0.5)
            f = np.floor(g)
            ok = (g >= F32(0.0)).all(axis=1) & (f <= (B * dims - 1).astype(F32)).all(axis=1)
        i0 = np.zeros((idx.size, 3), np.int64)
        i0[ok] = f[ok].astype(np.int64)
        b0 = np.where(ok, _block(bp, i0), -1)
        hit = b0 >= 0
        if not hit.any():
            continue
        todo[idx[hit]] = False
        idx, g, f, i0, b0 = idx[hit], g[hit], f[hit], i0[hit], b0[hit]
        level[idx], base[idx], block[idx] = li, i0, b0
        solid = _cell_values(obstacle, i0, b0)
        kind[idx] = np.where(solid, OBSTACLE, FOUND)
        idx, g, f, i0, b0 = idx[~solid], g[~solid], f[~solid], i0[~solid], b0[~solid]
        if idx.size == 0:
            continue
        v = np.empty((idx.size, 8), F32)
        for c in range(8):
            i = i0 + np.array([c & 1, (c >> 1) & 1, c >> 2], dtype=np.int64)
            b = _block(bp, i)
            valid = b >= 0
            valid[valid] = ~_cell_values(obstacle, i[valid], b[valid])
            v[:, c] = _cell_values(s, np.where(valid[:, None], i, i0), np.where(valid, b, b0))
        with np.errstate(invalid="ignore", over="ignore"):
            value[idx] = trilinear(v, (g - f).astype(F32))
    return kind, value, level, base, block


def _body_shade(levels, li, i0, D) -> np.ndarray:
    """the headlight shade [n] float32 of obstacle base cells i0 [n, 3] on levels li [n], seen along D [n, 3]"""
    shade = np.ones(i0.shape[0], F32)
    for l in np.unique(li):
        sel = np.flatnonzero(li == l)
        bp, obstacle, _ = levels[int(l)]
        nrm = np.zeros((sel.size, 3), np.int64)
        for a in range(3):
            for sgn in (-1, 1):
                i = i0[sel].copy()
                i[:, a] += sgn
                b = _block(bp, i)
                o = np.zeros(sel.size, np.int64)
                o[b >= 0] = _cell_values(obstacle, i[b >= 0], b[b >= 0])
                nrm[:, a] -= sgn * o
        nn = (nrm * nrm).sum(axis=1)
        lit = nn != 0
        nf, d = nrm[lit].astype(F32), D[sel[lit]]
        with np.errstate(invalid="ignore", over="ignore"):
            c = -((nf[:, 0] * d[:, 0] + nf[:, 1] * d[:, 1]) + nf[:, 2] * d[:, 2]) / np.sqrt(nn[lit].astype(F32))
            shade[sel[lit]] = F32(0.3) + F32(0.7) * np.fmax(c, F32(0.0))
    return shade


def render_host(levels: Sequence[tuple], camera, perspective, width: int, height: int, step, lo, hi, max_samples: int, table,
                background=(0.0, 0.0, 0.0), body_color=(0.7, 0.7, 0.7), t_min=T_MIN, info: Optional[dict] = None):
    """every ray of the definition, vectorised over the rays, one sample per iteration -> (rgba [height, width, 4] float32, codes
    [height, width] int32, samples [height, width] int32). levels: host_levels; camera: Camera.arrays()[0]. info, if a dict, receives
    what the tests ask of their inputs: 'levels' [height, width] int32, bit li set where a sample of the ray was found on level index li,
    and 'outside' [height, width] int32, the ray's samples that found no level."""
    cam = np.asarray(camera, dtype=F32).reshape(-1)
    eye, corner, du, dv, direction = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12:15]
    W, H, max_samples = int(width), int(height), int(max_samples)
    step, lo, hi, t_min = F32(step), F32(lo), F32(hi), F32(t_min)
    table = np.asarray(table, dtype=F32).reshape(256, 4)
    bg, body = np.asarray(background, dtype=F32).reshape(3), np.asarray(body_color, dtype=F32).reshape(3)
    N = W * H
    i = np.tile(np.arange(W, dtype=np.int64), H).astype(F32)
    j = np.repeat(np.arange(H, dtype=np.int64), W).astype(F32)
    one, zero = F32(1.0), F32(0.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = one / (hi - lo)
        T0 = (corner[None, :] + i[:, None] * du[None, :]) + j[:, None] * dv[None, :]
        if perspective:
            O = np.tile(eye, (N, 1))
            d = T0 - O
            m = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            D = d / m[:, None]
            miss = ~((m > zero) & np.isfinite(m))
        else:
            O, D, miss = T0, np.tile(direction, (N, 1)), np.zeros(N, bool)
        bp0 = levels[0][0]
        dims0 = np.array(bp0.shape, dtype=np.int64).reshape(3) if bp0.size else np.zeros(3, np.int64)
        box_hi = (BLOCK_SIZE * dims0).astype(F32) + F32(0.5)
        t0, t1 = np.zeros(N, F32), np.full(N, np.inf, F32)
        for a in range(3):
            flat = D[:, a] == zero
            miss |= flat & ~((zero <= O[:, a]) & (O[:, a] <= box_hi[a]))
            p, q = (zero - O[:, a]) / D[:, a], (box_hi[a] - O[:, a]) / D[:, a]
            t0 = np.where(flat, t0, np.fmax(t0, np.fmin(p, q)))
            t1 = np.where(flat, t1, np.fmin(t1, np.fmax(p, q)))
        miss |= ~(t0 < t1)
        n = np.zeros(N, np.int32)
        code = np.full(N, MISS, np.int32)
        T = np.ones(N, F32)
        rgb = np.zeros((N, 3), F32)
        seen, outside = np.zeros(N, np.int32), np.zeros(N, np.int32)
        t = t0.astype(F32)
        alive = ~miss
        while True:
            idx = np.flatnonzero(alive)
            if idx.size == 0:
                break
            done = ~(t[idx] < t1[idx])
            code[idx[done]] = EXIT
            full = ~done & (n[idx] == max_samples)
            code[idx[full]] = SAMPLES
            alive[idx[done | full]] = False
            idx = idx[~(done | full)]
            if idx.size == 0:
                break
            P = O[idx] + t[idx, None] * D[idx]
            kind, s, li, i0, _ = sample_scalar_host(P, levels)
            n[idx] += 1
            found = kind == FOUND
            seen[idx[found]] |= (1 << li[found]).astype(np.int32)
            outside[idx[kind == OUTSIDE]] += 1
            delta = np.ldexp(np.full(idx.size, step, F32), -np.maximum(li, 0).astype(np.int32)).astype(F32)
            solid = kind == OBSTACLE
            if solid.any():
                k = idx[solid]
                shade = _body_shade(levels, li[solid], i0[solid], D[k])
                rgb[k] = rgb[k] + T[k, None] * (body[None, :] * shade[:, None])
                T[k] = zero
                code[k] = BODY
                alive[k] = False
            lit = found & (s == s)
            k = idx[lit]
            x = np.fmin(np.fmax((s[lit] - lo) * inv, zero), one)
            e = table[(x * F32(255.0) + F32(0.5)).astype(np.int32)]
            w = T[k] * np.fmin(e[:, 3] * delta[lit], one)
            rgb[k] = rgb[k] + w[:, None] * e[:, 0:3]
            T[k] = T[k] - w
            dark = T[k] < t_min
            code[k[dark]] = OPAQUE
            alive[k[dark]] = False
            t[idx] = t[idx] + delta
        open_ = code != BODY
        rgb[open_] = rgb[open_] + T[open_, None] * bg[None, :]
        rgba = np.concatenate([rgb, (one - T)[:, None]], axis=1).astype(F32)
    if info is not None:
        info["levels"], info["outside"] = seen.reshape(H, W), outside.reshape(H, W)
    return rgba.reshape(H, W, 4), code.reshape(H, W), n.reshape(H, W)


# ---- the device set (ludwig_render_*) ----
class DeviceRender(Handle):
    """a render set over ALL device levels of a hierarchy (DeviceLevel, level index 0 first) with room for max_pixels pixels"""
    _destroy, _closed = "ludwig_render_destroy", "render set closed"

    def __init__(self, levels: Sequence, max_pixels: int):
        from . import _lib
        self._lib = _lib.load()
        self.n_levels, self.max_pixels = len(levels), int(max_pixels)
        self.shape = None
        arr = (C.c_void_p * len(levels))(*[lv.handle for lv in levels])
        h = C.c_void_p()
        _lib.check(self._lib.ludwig_render_create(arr, len(levels), self.max_pixels, C.byref(h)))
        self._h = h

    def image(self, t_coarse: int, field: str, scales, camera, perspective, width: int, height: int, step, lo, hi, max_samples: int, table,
              background=(0.0, 0.0, 0.0), body_color=(0.7, 0.7, 0.7), t_min=T_MIN) -> None:
        """queue one image of `field` (isosurface.FIELDS) of the newest state after coarse step t_coarse; the arguments are render_host's,
        scales [n_levels] the gradient fields' scale per level"""
        from . import _lib
        sc = np.ascontiguousarray(scales, dtype=F32).reshape(-1)
        if sc.size != self.n_levels:
            raise ValueError(f"render: {sc.size} scales for {self.n_levels} levels")
        cam = np.ascontiguousarray(camera, dtype=F32).reshape(-1)
        tab = np.ascontiguousarray(table, dtype=F32).reshape(-1)
        if cam.size != 16 or tab.size != 1024:
            raise ValueError(f"render: a camera of {cam.size} floats (16) or a table of {tab.size} (1024)")
        par = np.concatenate([[step, lo, hi, t_min], np.asarray(background, dtype=np.float64).reshape(3),
                              np.asarray(body_color, dtype=np.float64).reshape(3)]).astype(F32)
        _lib.check(self._lib.ludwig_render_image(self.handle, int(t_coarse), check_field(field), sc.ctypes.data, cam.ctypes.data,
                                                 int(bool(perspective)), int(width), int(height), par.ctypes.data, int(max_samples),
                                                 tab.ctypes.data))
        self.shape = (int(height), int(width))

    def download(self):
        """the last image: (rgba [height, width, 4] float32, codes [height, width] int32, samples [height, width] int32)"""
        from . import _lib
        h, w = self.shape if self.shape is not None else (0, 0)
        rgba, codes, samples = np.zeros((h, w, 4), F32), np.zeros((h, w), np.int32), np.zeros((h, w), np.int32)
        _lib.check(self._lib.ludwig_render_download(self.handle, rgba.ctypes.data, codes.ctypes.data, samples.ctypes.data, rgba.nbytes))
        return rgba, codes, samples


# ---- views of a run ----
class ViewPlan:
    """one view of a case as the kernel takes it: the camera in cell units of level index 0 and the baked table"""

    def __init__(self, view, width: int, height: int, offset, dx1: float):
        """view: preprocess.RenderView; its camera points are in the STL frame: (p + mesh_offset) / dx_1, as streamlines.seed_positions"""
        self.name, self.field = view.name, view.field
        self.width, self.height = int(width), int(height)
        self.camera, self.perspective = Camera.build(dict(view.camera), width, height, offset, dx1).arrays()
        self.table = bake_table([list(p) for p in view.colormap], view.opacity)
        self.lo, self.hi, self.step, self.max_samples = view.lo, view.hi, view.step, view.max_samples
        self.background, self.body_color = tuple(view.background), tuple(view.body_color)

    def arguments(self) -> dict:
        """the keyword arguments DeviceRender.image and render_host share"""
        return dict(camera=self.camera, perspective=self.perspective, width=self.width, height=self.height, step=self.step, lo=self.lo,
                    hi=self.hi, max_samples=self.max_samples, table=self.table, background=self.background, body_color=self.body_color)


def host_image(stepper, grids, plan: ViewPlan, t_coarse: int):
    """render_host of a view from a stepper's downloaded fields (the checker; a stepper without `render`)"""
    return render_host(host_levels(grids, stepper_scalars(stepper, grids, plan.field, t_coarse)), **plan.arguments())


def check_schedule(start_step: int, interval: int) -> Tuple[int, int]:
    return stats_mod.check_schedule("render", start_step, interval)


def summary(codes: np.ndarray, samples: np.ndarray) -> str:
    """one log line of an image: rays per end code and the total of samples"""
    ends = ", ".join(f"{nm} {int((codes == k).sum())}" for k, nm in enumerate(CODE_NAMES))
    return f"{codes.size} rays ended by: {ends}; {int(samples.astype(np.int64).sum())} samples"


# ---- files ----
def render_file_name(name: str, step: int) -> str:
    return "render_%s_%06d.png" % (name, step)


def quantise(rgba: np.ndarray) -> np.ndarray:
    """[h, w, >= 3] colours in 0..1 -> [h, w, 3] uint8: clip(rint(255 c), 0, 255), a NaN as 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.rint(np.asarray(rgba, dtype=F32)[..., 0:3] * F32(255.0))
    return np.clip(np.nan_to_num(c, nan=0.0), 0.0, 255.0).astype(np.uint8)


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path: str, image: np.ndarray) -> None:
    """image [h, w, 3] uint8 -> an 8-bit RGB PNG, every row with filter 0, one IDAT chunk"""
    a = np.ascontiguousarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: an image must be [h, w, 3] uint8, got {a.dtype} {a.shape}")
    h, w = a.shape[0], a.shape[1]
    rows = np.zeros((h, 1 + 3 * w), np.uint8)
    rows[:, 1:] = a.reshape(h, 3 * w)
    with open(path, "wb") as io:
        io.write(PNG_SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                 _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))


def read_png(path: str) -> np.ndarray:
    """what write_png wrote -> [h, w, 3] uint8 (8-bit RGB, no interlace, filter 0 on every row; anything else raises)"""
    with open(path, "rb") as io:
        raw = io.read()
    if raw[:8] != PNG_SIGNATURE:
        raise ValueError(f"{path}: no PNG signature")
    pos, head, data = 8, None, b""
    while pos < len(raw):
        (n,), tag = struct.unpack(">I", raw[pos:pos + 4]), raw[pos + 4:pos + 8]
        body = raw[pos + 8:pos + 8 + n]
        if struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError(f"{path}: chunk {tag!r} fails its CRC")
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            data += body
        pos += 12 + n
    if head is None or head[2:] != (8, 2, 0, 0, 0):
        raise ValueError(f"{path}: not an 8-bit RGB image without interlace")
    w, h = head[0], head[1]
    rows = np.frombuffer(zlib.decompress(data), dtype=np.uint8).reshape(h, 1 + 3 * w)
    if rows[:, 0].any():
        raise ValueError(f"{path}: a row filter other than 0")
    return rows[:, 1:].reshape(h, w, 3).copy()
