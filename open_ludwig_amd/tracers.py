"""Tracer particles advected on the device inside every batch (no reference counterpart: the reference writes whole flow files only).

advanced.tracers in a case YAML lists seed groups {name, points | line}; from `start_step` on, every `interval` coarse steps the set makes
one advance INSIDE the C batch (ludwig_execute_timestep_batch_tracers, k_tracers_advance) - no batch is cut for it - and every
`release_every` advances every seed releases a new particle into a ring of `generations`. Every `output_interval` coarse steps run_case
takes a snapshot (k_tracers_snapshot) and writes tracers_<name>_%06d.vtp (VTK XML PolyData: one `Verts` cell per live particle, `Lines`
cells = streaklines) and tracers_<name>.pvd. A particle keeps its ParticleId across files, which is what ParaView's temporal-particles-to-
pathlines filter needs: pathlines come from the snapshot sequence, no history is kept on the device. This module holds the definition as
a numpy restatement (advance_host, snapshot_host: the checker), the host bookkeeping, the seed plan and the files.

Definition. Everything is float32, every product and sum rounded on its own.
  * A position P is the streamlines' P (streamlines.seed_positions): cell units of level index 0, domain frame. Lattice velocity is the
    same in coarse cells per coarse step on every level (dx and dt halve together), so P += dt u needs no per-level scale.
  * sample_u(P) is streamlines.sample_host(P) - finest level holding P, float range test before any conversion, block_pointer, obstacle
    base cell, a corner that is no fluid cell takes the base cell's values, the probes' trilinear order - returning u and the level index
    only. rho is not part of a tracer and is never read.
  * A set has n_seeds seeds and G generations; slot g n_seeds + s holds P[3] and an int32 state: -1 empty, 0 alive, 1 outside, 2 obstacle
    (streamlines.END_OUTSIDE / END_OBSTACLE), 3 non-finite.
  * Advance k (k = 0, 1, ..., counted by the set on the host) behind coarse step t reads every level's newest velocity after t, with
    dt = float(interval):
      1. if k % release_every == 0, r = k / release_every and generation r % G is the released one;
      2. every alive slot not of the released generation: u = sample_u(P) (on failure the state takes the code and P stays);
         Pm = P + (0.5f dt) u per component; um = sample_u(Pm) (on failure the same); Pn = P + dt um; a non-finite component: state 3 and
         P stays; else P = Pn. A dead slot is never touched again until it is released;
      3. the released generation's slots get P = seed_s and state 0: overwritten whatever they held, not advanced, not sampled (a bad
         seed dies at its first advance).
  * Host bookkeeping (slot_ids; nothing of it is on the device): after K advances generation g holds release r = the largest
    r <= (K - 1) / release_every with r % G == g; ParticleId = r n_seeds + s, Birth = start_step + r release_every interval,
    Age = t - Birth.
  * Snapshot (changes no state): rec[slot][8] = x, y, z, ux, uy, uz, level index, code. An alive slot is sampled at P: code 0 with values,
    or zeros, level -1 and the failing code; any other slot: zeros, level -1, code = its state. The position is always written.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import statistics as stats_mod
from ._lib import Handle
from .streamlines import END_OBSTACLE, END_OUTSIDE, expand_group, host_levels, sample_host, seed_positions, to_domain

F32 = np.float32
EMPTY, ALIVE, OUTSIDE, OBSTACLE, NONFINITE = -1, 0, END_OUTSIDE, END_OBSTACLE, 3
REC = 8                                            # floats per snapshot record: x, y, z, ux, uy, uz, level index, code
CODE_NAMES = ("alive", "outside", "obstacle", "non-finite")


# ---- the numpy restatement of k_tracers_advance / k_tracers_snapshot ----
def velocity_levels(grids: Sequence, vel_of) -> List[tuple]:
    """streamlines.host_levels with only the velocity read: vel_of(level index) -> that level's velocity buffer [8,8,8,nb,3]. The rho
    entry is a zero-stride placeholder nothing of this module looks at."""
    def fields(li):
        vel = np.asarray(vel_of(li), dtype=F32)
        return np.broadcast_to(F32(0.0), vel.shape[:4]), vel
    return host_levels(grids, fields)


def stepper_levels(stepper, grids, t_coarse: int) -> List[tuple]:
    """velocity_levels of a stepper's newest state after coarse step t_coarse, from downloaded fields (stepper.field(level, name))"""
    from .statistics import t_sub_after
    return velocity_levels(grids, lambda li: stepper.field(li, "vel_temp" if t_sub_after(li, t_coarse) % 2 == 0 else "vel"))


def sample_u(P: np.ndarray, levels: Sequence[tuple]):
    """(code [n] int32, u [n, 3] float32, level index [n] int32) of the definition's sample_u"""
    code, vals, level, _ = sample_host(P, levels)
    return code, vals[:, 1:4], level


def new_state(n_seeds: int, generations: int) -> Tuple[np.ndarray, np.ndarray]:
    """(P [n_slots, 3] float32 zeros, state [n_slots] int32 all empty)"""
    n = int(n_seeds) * int(generations)
    return np.zeros((n, 3), F32), np.full(n, EMPTY, np.int32)


def advance_host(levels: Sequence[tuple], P: np.ndarray, state: np.ndarray, seeds, k: int, generations: int, release_every: int, dt,
                 info: Optional[dict] = None) -> None:
    """advance k of the definition, in place on P [n_slots, 3] float32 and state [n_slots] int32. info, if a dict, is added to:
    'level_changed' (alive particles whose start level differs from their start level at the previous advance; info['last_level']
    carries it) and 'midpoint_other_level' (midpoints on another level than their start)."""
    seeds = np.asarray(seeds, dtype=F32).reshape(-1, 3)
    n_seeds, dt = seeds.shape[0], F32(dt)
    released = (k // release_every) % generations if k % release_every == 0 else -1
    gen = np.arange(state.size) // max(n_seeds, 1)
    idx = np.flatnonzero((state == ALIVE) & (gen != released))
    with np.errstate(invalid="ignore", over="ignore"):
        code, u, li = sample_u(P[idx], levels)
        if info is not None:
            last = info.setdefault("last_level", np.full(state.size, -1, np.int32))
            seen = (code == 0) & (last[idx] >= 0)
            info["level_changed"] = info.get("level_changed", 0) + int((seen & (last[idx] != li)).sum())
            last[idx] = np.where(code == 0, li, -1)
        state[idx[code != 0]] = code[code != 0]
        idx, u, li = idx[code == 0], u[code == 0], li[code == 0]
        Pm = P[idx] + (F32(0.5) * dt) * u
        code, um, lm = sample_u(Pm, levels)
        if info is not None:
            info["midpoint_other_level"] = info.get("midpoint_other_level", 0) + int(((code == 0) & (lm != li)).sum())
        state[idx[code != 0]] = code[code != 0]
        idx, um = idx[code == 0], um[code == 0]
        Pn = P[idx] + dt * um
        ok = np.isfinite(Pn).all(axis=1)
        state[idx[~ok]] = NONFINITE
        P[idx[ok]] = Pn[ok]
    if released >= 0:
        sl = slice(released * n_seeds, (released + 1) * n_seeds)
        P[sl] = seeds
        state[sl] = ALIVE
        if info is not None and "last_level" in info:
            info["last_level"][sl] = -1


def snapshot_host(levels: Sequence[tuple], P: np.ndarray, state: np.ndarray) -> np.ndarray:
    """the snapshot records [n_slots, 8] float32 of the definition"""
    rec = np.zeros((state.size, REC), F32)
    rec[:, 0:3] = P
    rec[:, 6] = -1
    rec[:, 7] = state
    idx = np.flatnonzero(state == ALIVE)
    code, u, li = sample_u(P[idx], levels)
    ok = code == 0
    rec[idx[ok], 3:6] = u[ok]
    rec[idx[ok], 6] = li[ok]
    rec[idx, 7] = code
    return rec


# ---- host bookkeeping ----
def check_schedule(start_step: int, interval: int, release_every: int = 1, generations: int = 1) -> None:
    stats_mod.check_schedule("tracers", start_step, interval)
    if int(release_every) < 1 or int(generations) < 1:
        raise ValueError(f"tracers: release_every {release_every} and generations {generations} must be >= 1")


def advances_through(t_coarse: int, start_step: int, interval: int) -> int:
    """how many advances a run has made once coarse step t_coarse is done"""
    return 0 if t_coarse < start_step else (int(t_coarse) - int(start_step)) // int(interval) + 1


def slot_ids(K: int, n_seeds: int, generations: int, release_every: int, start_step: int = 1, interval: int = 1):
    """after K advances, per slot: (release [n_slots] int64, -1 where the generation was never released; ParticleId int64 = release
    n_seeds + seed, -1 likewise; Birth int64 = start_step + release release_every interval, the coarse step behind which it was released)"""
    n_seeds, G = int(n_seeds), int(generations)
    g = np.repeat(np.arange(G, dtype=np.int64), n_seeds)
    s = np.tile(np.arange(n_seeds, dtype=np.int64), G)
    if K <= 0:
        r = np.full(g.size, -1, np.int64)
    else:
        last = (int(K) - 1) // int(release_every)                   # the newest release
        r = last - ((last - g) % G)                                 # the largest r <= last with r % G == g (negative: never)
        r = np.where(r >= 0, r, -1)
    pid = np.where(r >= 0, r * n_seeds + s, -1)
    birth = np.where(r >= 0, int(start_step) + r * int(release_every) * int(interval), -1)
    return r, pid, birth


class HostTracers:
    """state plus schedule on the host, for steppers without the device set: advance(levels) is advance_host with the set's own count"""

    def __init__(self, seeds, generations: int, release_every: int, dt):
        self.seeds = np.array(seeds, dtype=F32).reshape(-1, 3)
        self.n_seeds, self.generations, self.release_every, self.dt = self.seeds.shape[0], int(generations), int(release_every), F32(dt)
        check_schedule(1, 1, release_every, generations)
        self.P, self.state = new_state(self.n_seeds, self.generations)
        self.n_advances = 0
        self.info: dict = {}

    def advance(self, levels: Sequence[tuple]) -> None:
        advance_host(levels, self.P, self.state, self.seeds, self.n_advances, self.generations, self.release_every, self.dt, self.info)
        self.n_advances += 1

    def snapshot(self, levels: Sequence[tuple]) -> np.ndarray:
        return snapshot_host(levels, self.P, self.state)


# ---- the device set (ludwig_tracers_*) ----
class DeviceTracers(Handle):
    """a tracer set over ALL device levels of a hierarchy (DeviceLevel, level index 0 first); seeds [n, 3] float32 positions in cell
    units of level index 0. start_step / interval: the coarse steps a batch advances it behind (execute_timestep_batch(tracers=...));
    dt = float(interval)."""
    _destroy, _closed = "ludwig_tracers_destroy", "tracer set closed"

    def __init__(self, levels: Sequence, seeds, generations: int = 1, release_every: int = 1, start_step: int = 1, interval: int = 1,
                 dt=None):
        from . import _lib
        self._lib = _lib.load()
        sd = np.ascontiguousarray(seeds, dtype=np.float32).reshape(-1, 3)
        self.n_seeds, self.generations, self.release_every = int(sd.shape[0]), int(generations), int(release_every)
        self.start_step, self.interval = int(start_step), int(interval)
        self.dt = F32(self.interval if dt is None else dt)
        arr = (C.c_void_p * len(levels))(*[lv.handle for lv in levels])
        h = C.c_void_p()
        _lib.check(self._lib.ludwig_tracers_create(arr, len(levels), self.n_seeds, sd.ctypes.data if self.n_seeds else None, self.generations,
                                                   self.release_every, float(self.dt), C.byref(h)))
        self._h = h

    @property
    def n_slots(self) -> int:
        return self.n_seeds * self.generations

    def is_advance_step(self, t_coarse: int) -> bool:
        return stats_mod.is_sample_step(t_coarse, self.start_step, self.interval)

    def advance(self, t_coarse: int) -> None:
        """queue one advance behind coarse step t_coarse, outside a batch"""
        from . import _lib
        _lib.check(self._lib.ludwig_tracers_advance(self.handle, int(t_coarse)))

    def snapshot(self, t_coarse: int) -> None:
        """queue a snapshot on the newest velocity after coarse step t_coarse"""
        from . import _lib
        _lib.check(self._lib.ludwig_tracers_snapshot(self.handle, int(t_coarse)))

    def download(self) -> Tuple[np.ndarray, int]:
        """the last snapshot: (records [n_slots, 8] float32, advances so far)"""
        from . import _lib
        rec = np.zeros((self.n_slots, REC), np.float32)
        k = C.c_int64(-1)
        _lib.check(self._lib.ludwig_tracers_download(self.handle, rec.ctypes.data if self.n_slots else None, rec.nbytes, C.byref(k)))
        return rec, int(k.value)


# ---- seeds ----
class TracerPlan:
    """every seed of a run: the groups' seeds in order (expand_group / seed_positions, as the streamlines')"""

    def __init__(self, groups: Sequence, offset, dx1: float):
        """groups: (name, points [n, 3] in the STL frame) pairs"""
        self.names = [str(nm) for nm, _ in groups]
        self.dx1 = float(dx1)
        P = [seed_positions(pts, offset, dx1) for _, pts in groups]
        self.seeds = np.concatenate(P + [np.zeros((0, 3), F32)]).astype(F32)
        self.group = np.concatenate([np.full(p.shape[0], gi, np.int32) for gi, p in enumerate(P)] + [np.zeros(0, np.int32)])
        self.seed_index = np.concatenate([np.arange(p.shape[0], dtype=np.int32) for p in P] + [np.zeros(0, np.int32)])

    @property
    def n_seeds(self) -> int:
        return int(self.group.size)


def check_capacity(n_seeds: int, generations: int, max_particles: int, steps: int, start_step: int, interval: int, release_every: int) -> None:
    """the configuration errors a run names before its first step"""
    if int(n_seeds) * int(generations) > int(max_particles):
        raise ValueError(f"advanced.tracers: {n_seeds} seeds of {generations} generations are more than advanced.tracers.max_particles = "
                         f"{max_particles}")
    K = advances_through(int(steps), start_step, interval)
    if K > 0 and ((K - 1) // int(release_every) + 1) * int(n_seeds) - 1 > np.iinfo(np.int32).max:
        raise ValueError(f"advanced.tracers: ParticleId does not fit int32 over {steps} steps ({(K - 1) // int(release_every) + 1} releases of "
                         f"{n_seeds} seeds): raise release_every or interval")


def jump_warning(interval: int, u_lattice: float, n_levels: int) -> Optional[str]:
    """one log line if a particle jumps more than a finest cell per advance"""
    jump = float(interval) * float(u_lattice) * 2.0 ** (int(n_levels) - 1)
    if jump > 1.0:
        return (f"tracers: warning: interval {interval} x u_lattice {u_lattice:g} x 2^{int(n_levels) - 1} = {jump:.3g} > 1: a particle jumps "
                f"more than a finest cell per advance")
    return None


# ---- files ----
def tracer_file_name(name: str, step: int) -> str:
    return "tracers_%s_%06d.vtp" % (name, step)


def streaklines(alive: np.ndarray, release: np.ndarray, n_seeds: int, generations: int) -> List[np.ndarray]:
    """per seed, the slots of its live particles in release order, newest first, broken at a dead or empty generation; runs of fewer
    than two particles give no line. alive [n_slots] bool, release [n_slots] (slot_ids). Returns slot index arrays, seed after seed."""
    out = []
    alive = np.asarray(alive, dtype=bool).reshape(int(generations), int(n_seeds))
    rel = np.asarray(release).reshape(int(generations), int(n_seeds))
    for s in range(int(n_seeds)):
        order = np.argsort(-rel[:, s], kind="stable")              # newest release first; never-released generations (-1) last
        run: List[int] = []
        for g in order:
            if alive[g, s] and rel[g, s] >= 0:
                run.append(int(g) * int(n_seeds) + s)
                continue
            if len(run) >= 2:
                out.append(np.array(run, dtype=np.int64))
            run = []
        if len(run) >= 2:
            out.append(np.array(run, dtype=np.int64))
    return out


class Particles:
    """one group's snapshot as the file holds it: the particles with code 0 in slot order and the streaklines through them"""

    def __init__(self, points, vel, level, particle_id, seed, age, connectivity, offsets):
        self.points, self.vel, self.level, self.particle_id, self.seed, self.age = points, vel, level, particle_id, seed, age
        self.connectivity, self.offsets = connectivity, offsets


def group_particles(plan: TracerPlan, gi: int, rec: np.ndarray, K: int, step: int, generations: int, release_every: int, start_step: int,
                    interval: int) -> Particles:
    """group gi of a snapshot after K advances, taken behind coarse step `step`"""
    n_seeds = plan.n_seeds
    rel, pid, birth = slot_ids(K, n_seeds, generations, release_every, start_step, interval)
    in_group = np.tile(plan.group == gi, int(generations))
    live = (rec[:, 7] == ALIVE) & (rel >= 0)
    keep = np.flatnonzero(live & in_group)
    place = np.full(rec.shape[0], -1, np.int64)
    place[keep] = np.arange(keep.size)
    lines = [place[l] for l in streaklines(live & in_group, rel, n_seeds, generations)]
    conn = np.concatenate(lines + [np.zeros(0, np.int64)]).astype(np.int64)
    off = np.cumsum([len(l) for l in lines], dtype=np.int64) if lines else np.zeros(0, np.int64)
    seed = np.tile(plan.seed_index, int(generations))
    return Particles(to_domain(rec[keep, 0:3], plan.dx1), rec[keep, 3:6].astype(F32), rec[keep, 6].astype(np.int32) + 1,
                     pid[keep].astype(np.int32), seed[keep].astype(np.int32), (int(step) - birth[keep]).astype(np.int32), conn, off)


class TracerWriter:
    """tracers_<name>_%06d.vtp per snapshot and tracers_<name>.pvd (time = step * time_scale), rewritten after every file"""

    def __init__(self, out_dir: str, plan: TracerPlan, time_scale: float, generations: int, release_every: int, start_step: int, interval: int):
        self.out_dir, self.plan, self.time_scale = out_dir, plan, float(time_scale)
        self.schedule = (int(generations), int(release_every), int(start_step), int(interval))
        self.entries: Dict[str, List[Tuple[float, str]]] = {n: [] for n in plan.names}

    def write(self, step: int, rec: np.ndarray, K: int) -> List[Particles]:
        from .output import write_vtp_tracers
        from .slices import write_pvd
        out = []
        for gi, name in enumerate(self.plan.names):
            p = group_particles(self.plan, gi, rec, K, step, *self.schedule)
            f = tracer_file_name(name, step)
            write_vtp_tracers(os.path.join(self.out_dir, f), p.points, p.vel, p.level, p.particle_id, p.seed, p.age, p.connectivity, p.offsets)
            self.entries[name].append((float(step) * self.time_scale, f))
            write_pvd(os.path.join(self.out_dir, "tracers_%s.pvd" % name), self.entries[name])
            out.append(p)
        return out


def summary(plan: TracerPlan, gi: int, rec: np.ndarray, generations: int) -> str:
    """one log line of a group's snapshot: alive, dead by code, empty"""
    code = rec[np.tile(plan.group == gi, int(generations)), 7].astype(np.int32)
    dead = ", ".join(f"{nm} {int((code == k).sum())}" for k, nm in enumerate(CODE_NAMES) if k > 0)
    return f"{code.size} slots: alive {int((code == ALIVE).sum())}; dead: {dead}; empty {int((code == EMPTY).sum())}"


from .isosurface import read_vtp                   # noqa: E402,F401  (the reader of every kind of PolyData file)
