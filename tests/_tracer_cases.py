"""Shared cases and checks of the tracer tests (host and device); the fields and shapes are the streamline tests' own."""
import numpy as np

import _streamline_cases as sc
from open_ludwig_amd import tracers as tr

F32 = np.float32


def velocity_level(g, vel):
    """one level as advance_host reads it: the velocity only"""
    return tr.velocity_levels([g], lambda li: vel)


def assert_same_records(got, want):
    """snapshot records bit for bit, NaN meeting NaN"""
    assert got.dtype == want.dtype == F32 and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True), f"records differ at {np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4].tolist()}"


# ---- 1. uniform flow on 27 blocks: one seed that leaves the 24-cell grid, one that stays ----
UNIFORM_SEEDS = np.array([[23.2, 7.3, 11.6], [3.25, 20.125, 2.9]], dtype=F32)
UNIFORM_ADVANCES = 32
UNIFORM_LAST_ALIVE = 26          # moves of the first seed: the 27th midpoint, x = 24.5 + 0.025, has left floor(x - 0.5) <= 23


def check_uniform(history):
    """history[k] = (P, state) after advance k (advance 0 releases; advance k >= 1 is move k)"""
    for k, (P, state) in enumerate(history):
        assert state[1] == tr.ALIVE
        assert state[0] == (tr.ALIVE if k <= UNIFORM_LAST_ALIVE else tr.OUTSIDE), (k, state[0])
        moves = np.array([min(k, UNIFORM_LAST_ALIVE), k], dtype=np.float64)
        want = UNIFORM_SEEDS.astype(np.float64)
        want[:, 0] += moves * float(sc.U0)
        assert np.abs(P.astype(np.float64) - want).max() <= 1e-4, (k, P, want)
    assert abs(float(history[-1][0][0, 0]) - 24.49998) < 2e-5
    assert np.array_equal(history[-1][0][0], history[UNIFORM_LAST_ALIVE][0][0])          # P unchanged once dead


# ---- 2. solid-body rotation: one full turn ----
ROTATION_RADII = (8.0, 4.0)
ROTATION_ADVANCES = {1: 1571, 4: 393}            # round(2 pi / (Omega dt)) for Omega = 0.004
ROTATION_DRIFT = 1e-3                            # cells; the midpoint rule measured at most 3.7e-5 (dt = 1) and 2.3e-5 (dt = 4)
EULER_DRIFT = {1: (0.05, 0.10), 4: (0.21, 0.41)}    # what plain Euler drifts by, radius 4 and 8


def rotation_seeds():
    return np.concatenate([sc.rotation_seeds(r) for r in ROTATION_RADII])


def radii(P):
    p = np.asarray(P, dtype=np.float64)
    return np.hypot(p[:, 0] - sc.CENTRE[0], p[:, 1] - sc.CENTRE[1])


def euler_host(levels, P, n, dt):
    """the same turn with the midpoint removed: what the drift bound must tell apart"""
    P = P.copy()
    for _ in range(n):
        code, u, _ = tr.sample_u(P, levels)
        assert (code == 0).all()
        P = P + F32(dt) * u
    return P


# ---- 3. planted states (the streamlines' L of three blocks), G = 1 ----
PLANTED_ADVANCES, PLANTED_DT = 24, 8.0           # about 0.25 cells per advance
# slots by what ends them: the NaN seed and the outside seed (1), the seed inside an obstacle cell (2), the seed next to the infinite
# velocity (3), and two seeds of this file: one 0.8 cells from the absent fourth block (1), one whose midpoint reaches the NaN velocity's
# stencil before its start does (3)
PLANTED_ENDS = {1: 1, 2: 1, 3: 2, 18: 3, 19: 1, 20: 3}


def planted():
    g, _, vel, seeds, _ = sc.planted()
    seeds = np.concatenate([seeds[: len(seeds) // 2], np.array([[7.2, 12.6, 4.2], [10.1, 3.4, 5.4]], dtype=F32)])
    return g, vel, seeds


# ---- 4. the release ring ----
RING_SEEDS = np.array([[23.2, 7.3, 11.6], [3.25, 20.125, 2.9], [23.9, 1.5, 2.5], [np.nan, 3.0, 3.0], [12.75, 20.125, 2.9]], dtype=F32)
RING_G, RING_EVERY, RING_ADVANCES = 3, 2, 9
RING_DT = 8.0                                    # 0.4 cells per advance: the seeds near x = 24 leave the grid within the ring's life


def slot_ids_loop(K, n_seeds, G, release_every, start_step, interval):
    """the bookkeeping as a plain loop over the advances"""
    rel = np.full(n_seeds * G, -1, np.int64)
    for k in range(K):
        if k % release_every == 0:
            r = k // release_every
            rel[(r % G) * n_seeds: (r % G + 1) * n_seeds] = r
    s = np.tile(np.arange(n_seeds), G)
    pid = np.where(rel >= 0, rel * n_seeds + s, -1)
    birth = np.where(rel >= 0, start_step + rel * release_every * interval, -1)
    return rel, pid, birth


# ---- 5. the tunnel: a dense rake straddling the level edges ----
# Level 2 covers x from 8 coarse cells, level 3 from 12; the locator takes a level once the BASE cell floor(P 2^li - 0.5) lies in it, half
# a fine cell further in: from x = 8.25 and x = 12.125. The flow moves about 0.04 cells per coarse step in +x, so a second rake sits up
# to 0.2 cells upstream of those two edges: its particles cross them within the six steps, some with only their midpoint across.
TUNNEL_STEPS = 6
TUNNEL_G, TUNNEL_EVERY = 2, 2
TUNNEL_SCHEDULES = ((1, 1), (2, 2))              # start_step, interval


def tunnel_seeds():
    """64 points with x within +-0.1 of 8 and of 12 at varied y, z, 64 more within 0.2 upstream of the locator's edges, plus the
    streamline tests' rake (forward half)"""
    i = np.arange(32)
    dx = -0.1 + 0.2 * (i + 0.5) / 32
    y = 9.3 + 13.0 * ((i * 7) % 32) / 32
    z = 10.1 + 11.5 * ((i * 11) % 32) / 32
    edge = np.concatenate([np.stack([8.0 + dx, y, z], axis=1), np.stack([12.0 + dx, y[::-1], z], axis=1)])
    up = -0.2 * (i + 0.5) / 32
    y2, z2 = 13.1 + 5.8 * ((i * 5) % 32) / 32, 13.2 + 5.6 * ((i * 13) % 32) / 32     # inside level 3's y, z extent as well
    locator = np.concatenate([np.stack([8.25 + up, y, z], axis=1), np.stack([12.125 + up, y2, z2], axis=1)])
    rake, _ = sc.tunnel_rake()
    return np.concatenate([edge, locator, rake[: len(rake) // 2]]).astype(F32)
