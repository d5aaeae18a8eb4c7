"""Shared cases and checks of the streamline tests (host and device)."""
import numpy as np

import _iso_cases as ic
from open_ludwig_amd import cases, streamlines as sl

F32 = np.float32


def assert_same(got, want):
    """counts, codes and the used records, bit for bit, NaN meeting NaN"""
    (gc, ge, gr), (wc, we, wr) = got, want
    assert gc.dtype == wc.dtype == np.int32 and ge.dtype == we.dtype == np.int32 and gr.dtype == wr.dtype == F32
    assert np.array_equal(gc, wc), f"counts differ at lines {np.flatnonzero(gc != wc)[:8].tolist()}"
    assert np.array_equal(ge, we), f"codes differ at lines {np.flatnonzero(ge != we)[:8].tolist()}"
    a, b = sl.used(gc, gr), sl.used(wc, wr)
    assert np.array_equal(a, b, equal_nan=True), f"records differ at {np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))[:4].tolist()}"


def one_level(g, rho, vel):
    return sl.host_levels([g], lambda li: (rho, vel))


# ---- 1. uploaded fields on 27 blocks ----
U0 = F32(0.05)
UNIFORM_SEEDS = np.array([[3.25, 7.3, 11.6], [12.75, 20.125, 2.9], [20.5, 0.75, 23.4]], dtype=F32)


def box27():
    coords, _ = ic.block_grid(3, 3, 3)
    return cases.make_level(1, coords, (3, 3, 3), 0.6)


def uniform_fields():
    rho = np.ones((8, 8, 8, 27), F32, order="F")
    vel = np.zeros((8, 8, 8, 27, 3), F32, order="F")
    vel[..., 0] = U0
    return rho, vel


def both_directions(seeds):
    """(seeds, sign) with every seed forward, then every seed backward"""
    s = np.asarray(seeds, dtype=F32).reshape(-1, 3)
    return np.concatenate([s, s]), np.concatenate([np.ones(len(s), F32), -np.ones(len(s), F32)])


def check_uniform(counts, codes, rec, seeds, sign, step=0.5):
    """exact vertices P_0 + k step s in x, the other components unchanged, the line ending with code 1 where the 24-cell grid ends:
    a vertex needs floor(x - 0.5) in 0..23, and so does the midpoint before the next one"""
    for i, (p, s) in enumerate(zip(seeds, sign)):
        k, x = 0, float(p[0])
        inside = lambda v: 0.0 <= v - 0.5 and np.floor(v - 0.5) <= 23
        while inside(x + 0.5 * step * s) and inside(x + step * s):
            x += step * float(s)
            k += 1
        assert codes[i] == sl.END_OUTSIDE and counts[i] == k + 1 > 4, (i, codes[i], counts[i], k)
        want = np.tile(p, (k + 1, 1))
        want[:, 0] = p[0] + F32(step) * s * np.arange(k + 1, dtype=F32)
        assert np.array_equal(rec[i, : k + 1, 0:3], want)
        assert np.array_equal(rec[i, : k + 1, 7], np.zeros(k + 1, F32))


OMEGA = 0.004
CENTRE = ic.SPHERE_CENTRE + 0.5                    # a cell centre i lies at position i + 0.5
ROTATION = [(0.5, 8.0, 101), (1.0, 8.0, 50), (0.25, 4.0, 101)]         # step, radius, n = round(2 pi r / step)


def rotation_fields():
    """solid-body rotation about the z axis through the off-lattice centre: an exactly linear field"""
    coords, _ = ic.block_grid(3, 3, 3)
    x = ic.cell_centres(coords)
    rho = np.asfortranarray((1.0 + 0.001 * x[..., 0] - 0.002 * x[..., 2]).astype(F32))
    vel = np.zeros((8, 8, 8, 27, 3), F32, order="F")
    vel[..., 0] = (-OMEGA * (x[..., 1] - ic.SPHERE_CENTRE[1])).astype(F32)
    vel[..., 1] = (OMEGA * (x[..., 0] - ic.SPHERE_CENTRE[0])).astype(F32)
    return rho, vel


def rotation_seeds(radius):
    ang = np.array([0.3, 2.0, 4.4])
    p = np.stack([CENTRE[0] + radius * np.cos(ang), CENTRE[1] + radius * np.sin(ang), np.array([5.3, 11.9, 17.45])], axis=1)
    return p.astype(F32)


def check_rotation(counts, codes, rec, step, radius, n):
    """the midpoint rule with a unit direction on an exactly linear field: the radius grows by 1 + eps^4 per step, eps = step / (2 r),
    and z stays; plain Euler would drift by 2 eps^2 per step"""
    assert (counts == n + 1).all() and (codes == sl.END_STEPS).all()
    p = rec[:, : n + 1, 0:3].astype(np.float64)
    r = np.hypot(p[..., 0] - CENTRE[0], p[..., 1] - CENTRE[1])
    drift = r[:, n] - r[:, 0]
    bound = n * (step / (2 * radius)) ** 4 * radius
    print(f"rotation step {step} r {radius} n {n}: drift {drift.tolist()} against n eps^4 r = {bound:.3e}; "
          f"z drift {np.abs(p[:, n, 2] - p[:, 0, 2]).max():.1e}")
    assert (drift >= 0.9 * bound - 1e-4).all() and (drift <= 1.05 * bound + 1e-4).all(), (drift, bound)
    assert (np.abs(p[:, n, 2] - p[:, 0, 2]) <= 1e-4).all()


# ---- 2. planted states on three blocks in an L ----
MIN_SPEED = F32(0.001)


def planted():
    """three blocks in an L (the fourth, (2, 2, 1), absent) with obstacle cells on block faces, one NaN and one infinite velocity, a
    patch of zero velocity and a cell whose speed equals MIN_SPEED exactly -> (level, rho, vel, seeds, sign)"""
    coords = [(1, 1, 1), (2, 1, 1), (1, 2, 1)]
    g = cases.make_level(1, coords, (2, 2, 1), 0.6)
    assert [tuple(c) for c in g.active_block_coords] == [(1, 1, 1), (1, 2, 1), (2, 1, 1)]
    x = ic.cell_centres(sorted(coords))
    rho = np.asfortranarray((1.0 + 0.01 * np.cos(0.2 * x[..., 0] * x[..., 1])).astype(F32))
    vel = np.asfortranarray(np.stack([0.03 + 0.01 * np.sin(0.3 * x[..., 1]), 0.008 * np.cos(0.4 * x[..., 2] + 0.1 * x[..., 0]),
                                      0.001 * np.sin(0.5 * x[..., 0])], axis=-1).astype(F32))
    g.obstacle[7, 3:5, 2:4, 0] = True                                       # on the +x face of block 0
    g.obstacle[0, 4, 5, 2] = True                                           # on the -x face of block 2 = (2, 1, 1)
    g.obstacle[2:4, 7, 6, 0] = True                                         # on the +y face of block 0
    vel[3, 3, 5, 2, 1] = np.nan
    vel[5, 1, 6, 2, 0] = np.inf
    vel[2:6, 1:4, 0:3, 1, :] = 0.0                                          # block 1 = (1, 2, 1)
    vel[2, 5, 3, 0, :] = (MIN_SPEED, 0.0, 0.0)
    seeds = [[2.5, 5.5, 3.5],                                               # the centre of the MIN_SPEED cell: the line continues
             [np.nan, 3.0, 3.0], [40.0, 3.0, 3.0], [7.5, 3.5, 2.5],         # NaN, outside, inside an obstacle cell
             [1.2, 12.6, 4.2],                                              # block (1, 2, 1), heading for the absent fourth block
             [0.7, 9.9, 1.4]]                                               # towards the patch of zero velocity
    seeds += [[1.1, 0.8 + 0.9 * j, 0.9 + 0.8 * j] for j in range(8)]       # a rake through the faces, the NaN and the infinity
    seeds += [[4.3, 3.6 + 0.3 * j, 2.2 + 0.4 * j] for j in range(4)]       # at the obstacle cells on the +x face of block 0
    seeds += [[9.2, 1.4, 6.6]]                                              # next to the infinite velocity
    s, sign = both_directions(np.array(seeds, dtype=F32))
    return g, rho, vel, s, sign


PLANTED_MAX_STEPS = 24


# ---- 3. the tunnel ----
TUNNEL_STEP, TUNNEL_MIN_SPEED, TUNNEL_MAX_STEPS = 0.5, 1.0e-6, 160


def tunnel_rake():
    """a rake upstream of the sphere (centre (19.2, 16, 16), radius 6.8 coarse cells) across the refined region (level 2 from
    8 to 32, level 3 from 12 to 28) and a ring of seeds close to the sphere, both directions"""
    y = np.linspace(5.2, 26.9, 12)
    z = 16.3 + 0.21 * np.arange(12)
    p = np.stack([np.full(12, 5.3), y, z], axis=1)
    a = 2.0 * np.pi * (np.arange(16) + 0.3) / 16                            # a ring 0.25 coarse cells off the sphere's surface
    near = np.stack([19.2 + 7.05 * np.cos(a), 16.0 + 7.05 * np.sin(a), np.full(16, 16.2)], axis=1)
    return both_directions(np.concatenate([p, near]).astype(F32))
