"""Warm start: a run's levels filled from another run's flow, resampled on the device (no reference counterpart: the reference starts
every run from rest, init_eq! src/main.jl:109-134).

What is carried from one grid to another is the MACROSCOPIC state, rho and u. The populations restart at their equilibrium, so the
non-equilibrium part (the viscous stress) is rebuilt by the first steps; a cell that a finer source level covers takes the finer
level's interpolated value; and a warm-started run is NOT bit-identical to a continued one, not even on an identical grid.

advanced.state_files in a case YAML makes run_case write state_%06d.npz (FlowState: rho and the newest velocity of every level);
advanced.initial_condition names such a file, and every level is filled from it after set-up. The device side is ludwig_flow_source_* and
ludwig_level_init_from_source (k_init_from_source); this module holds the definition as a numpy restatement (init_host: the checker),
the state file and the map between the two runs' frames.

Definition. Everything is float32, every product and sum rounded on its own.
  * A destination cell (x, y, z) of a block at 1-based block coordinates m has the global cell coordinates gc_a = 8 (m_a - 1) + x_a and
    samples the source at P_a = a_a ((float)gc_a + 0.5f) + b_a: a position in cell units of the source's level index 0, domain frame.
  * (code, q, li) = streamlines.sample_host(P) on the source (the finest source level whose active blocks hold the base cell; code 1
    outside, 2 in a source obstacle cell).
  * code 0 and rho, ux, uy, uz all finite, with s = vel_scale: rho' = 1 + (rho - 1) (s s), u' = u s. (Scaling u by s at a fixed lattice
    speed of sound scales the pressure fluctuation by s^2.) Otherwise rho', u' = fallback.
  * An obstacle cell of the destination gets rho' = 1, u' = 0.
  * rho = rho', vel = vel_temp = u', f = f_temp = equilibrium_host(rho', u'); with temporal storage the saved state gets the same.
  * counts over the destination's non-obstacle cells: found, outside, source obstacle, non-finite, then found per source level.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from ._lib import Handle
from .blocks import BLOCK_SIZE, build_lattice_arrays
from .streamlines import sample_host

F32 = np.float32
FOUND, OUTSIDE, SOURCE_OBSTACLE, NON_FINITE = 0, 1, 2, 3
N_OUTCOMES = 4
COUNT_NAMES = ("found", "outside", "source obstacle", "non-finite")


# ---- the state a run leaves behind ----
class FlowState:
    """rho and the newest velocity of every level of a run after a coarse step, with what places them in space.
    levels: per level (level index 0 first) a dict of block_pointer [gx, gy, gz] int32 (1-based, 0 = absent), obstacle [8,8,8,nb] bool,
    rho [8,8,8,nb] float32, vel [8,8,8,nb,3] float32, dx float. mesh_offset: the run's (domain frame = STL frame after stl_scale, plus
    mesh_offset: the probes' convention). u_lattice, step (the coarse step the state follows), case (the case's name)."""

    def __init__(self, levels: Sequence[dict], mesh_offset, u_lattice: float, step: int, case: str = ""):
        self.levels = [dict(block_pointer=np.asfortranarray(lv["block_pointer"], dtype=np.int32),
                            obstacle=np.asfortranarray(np.asarray(lv["obstacle"]).astype(bool)),
                            rho=np.asfortranarray(lv["rho"], dtype=F32), vel=np.asfortranarray(lv["vel"], dtype=F32),
                            dx=float(lv["dx"])) for lv in levels]
        self.mesh_offset = np.asarray(mesh_offset, dtype=np.float64).reshape(3)
        self.u_lattice = float(u_lattice)
        self.step = int(step)
        self.case = str(case)

    @property
    def n_levels(self) -> int:
        return len(self.levels)

    def host_levels(self) -> List[tuple]:
        """what streamlines.sample_host reads"""
        return [(lv["block_pointer"], lv["obstacle"], lv["rho"], lv["vel"]) for lv in self.levels]


def state_file_name(step: int) -> str:
    return "state_%06d.npz" % step


def state_from_stepper(stepper, grids, t_coarse: int, mesh_offset, u_lattice: float, case: str = "") -> FlowState:
    """the FlowState of a stepper's newest state after coarse step t_coarse, from downloaded fields"""
    from .statistics import t_sub_after
    levels = []
    for li, g in enumerate(grids):
        vel_name = "vel_temp" if t_sub_after(li, t_coarse) % 2 == 0 else "vel"
        levels.append(dict(block_pointer=g.block_pointer, obstacle=g.obstacle, rho=stepper.field(li, "rho"),
                           vel=stepper.field(li, vel_name), dx=g.dx))
    return FlowState(levels, mesh_offset, u_lattice, t_coarse, case)


def save_state(path: str, state: FlowState) -> None:
    """one .npz file, numpy arrays only (read back with allow_pickle=False)"""
    arrays = dict(n_levels=np.array(state.n_levels, np.int32), mesh_offset=state.mesh_offset, u_lattice=np.array(state.u_lattice, np.float64),
                  step=np.array(state.step, np.int64), case=np.array(state.case), dx=np.array([lv["dx"] for lv in state.levels], np.float64))
    for li, lv in enumerate(state.levels):
        arrays["block_pointer_%d" % li] = lv["block_pointer"]
        arrays["obstacle_%d" % li] = lv["obstacle"]
        arrays["rho_%d" % li] = lv["rho"]
        arrays["vel_%d" % li] = lv["vel"]
    with open(path, "wb") as io:                      # an open file: savez appends no suffix of its own
        np.savez(io, **arrays)


def load_state(path: str) -> FlowState:
    with np.load(path, allow_pickle=False) as z:
        n = int(z["n_levels"])
        levels = [dict(block_pointer=z["block_pointer_%d" % li], obstacle=z["obstacle_%d" % li], rho=z["rho_%d" % li],
                       vel=z["vel_%d" % li], dx=float(z["dx"][li])) for li in range(n)]
        return FlowState(levels, z["mesh_offset"], float(z["u_lattice"]), int(z["step"]), str(z["case"]))


def affine_map(state: FlowState, dst_dx_level: float, dst_mesh_offset) -> np.ndarray:
    """map [6] float32 = a_x, a_y, a_z, b_x, b_y, b_z for a destination level of cell size dst_dx_level in a run with mesh offset
    dst_mesh_offset: a cell centre dx (gc + 1/2) of the destination's domain frame is the STL point dx (gc + 1/2) - off_dst, which the
    source run holds at + off_src, in cells of its level index 0: a = dx_dst / dx1_src, b = (off_src - off_dst) / dx1_src. Float64,
    cast once."""
    dx1 = float(state.levels[0]["dx"])
    a = np.full(3, float(dst_dx_level) / dx1, np.float64)
    b = (state.mesh_offset - np.asarray(dst_mesh_offset, dtype=np.float64).reshape(3)) / dx1
    return np.concatenate([a, b]).astype(F32)


# ---- the numpy restatement of k_init_from_source ----
def equilibrium_host(rho: np.ndarray, u: np.ndarray) -> np.ndarray:
    """calculate_equilibrium (src/physics_utils.jl:34-39) for rho [...] and u [..., 3] float32 -> [..., 27] float32, in the device
    function's operand order: cu = (cx ux + cy uy) + cz uz, usq = (ux ux + uy uy) + uz uz, (rho w) (((1 + 3 cu) + (4.5 cu) cu) - 1.5 usq)"""
    cx, cy, cz, w, *_ = build_lattice_arrays()
    rho = np.asarray(rho, dtype=F32)
    u = np.asarray(u, dtype=F32)
    ux, uy, uz = u[..., 0], u[..., 1], u[..., 2]
    out = np.empty(rho.shape + (27,), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        usq = (ux * ux + uy * uy) + uz * uz
        for k in range(27):
            cu = (F32(cx[k]) * ux + F32(cy[k]) * uy) + F32(cz[k]) * uz
            out[..., k] = (rho * w[k]) * (((F32(1.0) + F32(3.0) * cu) + (F32(4.5) * cu) * cu) - F32(1.5) * usq)
    return out


def cell_positions(level, map6) -> np.ndarray:
    """P [8,8,8,nb,3] float32 of every cell of a level (anything with map_x/y/z or active_block_coords)"""
    B = BLOCK_SIZE
    m = np.asarray(map6, dtype=F32).reshape(6)
    coords = np.asarray(level.active_block_coords, dtype=np.int64).reshape(-1, 3)
    nb = coords.shape[0]
    P = np.empty((B, B, B, nb, 3), F32)
    for a in range(3):
        local = np.arange(B, dtype=np.int64).reshape([B if i == a else 1 for i in range(3)] + [1])
        gc = B * (coords[:, a] - 1).reshape(1, 1, 1, nb) + local
        P[..., a] = np.broadcast_to(m[a] * (gc.astype(F32) + F32(0.5)) + m[3 + a], (B, B, B, nb))
    return P


def init_host(level, source_levels: Sequence[tuple], map6, vel_scale, fallback) -> dict:
    """ludwig_level_init_from_source for one destination level (a BlockLevel: active_block_coords, obstacle) on the source
    `source_levels` (streamlines.host_levels tuples) -> dict of rho [8,8,8,nb], vel [8,8,8,nb,3], f [8,8,8,nb,27] (what rho, vel =
    vel_temp = vel_old, f = f_temp = f_old get), counts int64 [4 + n], and per cell outcome [8,8,8,nb] int8 (FOUND .. NON_FINITE; -1 in a
    destination obstacle cell) and source_level [8,8,8,nb] int32 (-1 unless found)"""
    s = F32(vel_scale)
    fb = np.asarray(fallback, dtype=F32).reshape(4)
    P = cell_positions(level, map6)
    shape = P.shape[:-1]
    # points in memory order (x fastest): neighbouring points read neighbouring source cells
    code, q, li, _ = sample_host(np.stack([P[..., a].reshape(-1, order="F") for a in range(3)], axis=1), source_levels)
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(q).all(axis=1)
        outcome = np.where(code == 0, np.where(finite, FOUND, NON_FINITE), code).astype(np.int8)
        found = outcome == FOUND
        vals = np.broadcast_to(fb, q.shape).copy()
        s2 = s * s
        vals[found, 0] = F32(1.0) + (q[found, 0] - F32(1.0)) * s2
        vals[found, 1:4] = q[found, 1:4] * s
    solid = np.asarray(level.obstacle).astype(bool).reshape(-1, order="F")
    vals[solid] = np.array([1.0, 0.0, 0.0, 0.0], F32)
    outcome[solid] = -1
    src_level = np.where(found & ~solid, li, -1).astype(np.int32)
    counts = np.zeros(N_OUTCOMES + len(source_levels), np.int64)
    for k in range(N_OUTCOMES):
        counts[k] = int((outcome == k).sum())
    for k in range(len(source_levels)):
        counts[N_OUTCOMES + k] = int((src_level == k).sum())
    rho = np.asfortranarray(vals[:, 0].reshape(shape, order="F"))
    vel = np.asfortranarray(np.stack([vals[:, 1 + a].reshape(shape, order="F") for a in range(3)], axis=-1))
    return dict(rho=rho, vel=vel, f=np.asfortranarray(equilibrium_host(rho, vel)), counts=counts,
                outcome=outcome.reshape(shape, order="F"), source_level=src_level.reshape(shape, order="F"))


def counts_line(level_id: int, counts) -> str:
    """one log line of a level's counts"""
    c = [int(v) for v in counts]
    per = ", ".join(f"level {k + 1}: {v}" for k, v in enumerate(c[N_OUTCOMES:]))
    head = ", ".join(f"{nm} {c[k]}" for k, nm in enumerate(COUNT_NAMES))
    return f"initial condition, level {level_id}: {sum(c[:N_OUTCOMES])} fluid cells: {head}; found by source {per}"


# ---- the device source (ludwig_flow_source_*) ----
class DeviceFlowSource(Handle):
    """a flow source in device memory: from host arrays (a FlowState or streamlines.host_levels tuples) or, with from_levels, copied on
    the device from live DeviceLevels"""
    _destroy, _closed = "ludwig_flow_source_destroy", "flow source closed"

    def __init__(self, source, device: int = 0):
        from . import _lib
        self._lib = _lib.load()
        levels = source.host_levels() if isinstance(source, FlowState) else list(source)
        n = len(levels)
        self.n_levels = n
        keep = []
        dims, nbs = np.zeros(3 * n, np.int32), np.zeros(n, np.int32)
        bp, ob, rh, vl = ((C.c_void_p * n)() for _ in range(4))
        for li, (block_pointer, obstacle, rho, vel) in enumerate(levels):
            b = np.asfortranarray(block_pointer, dtype=np.int32)
            nb = int(np.asarray(rho).shape[3]) if np.asarray(rho).ndim == 4 else 0
            dims[3 * li: 3 * li + 3] = b.shape if b.ndim == 3 else (0, 0, 0)
            nbs[li] = nb
            arrs = (b, np.asfortranarray(np.asarray(obstacle).astype(np.uint8)), np.asfortranarray(rho, dtype=np.float32),
                    np.asfortranarray(vel, dtype=np.float32))
            if arrs[1].shape != (8, 8, 8, nb) or arrs[2].shape != (8, 8, 8, nb) or arrs[3].shape != (8, 8, 8, nb, 3):
                raise ValueError(f"flow source: level index {li}: obstacle {arrs[1].shape}, rho {arrs[2].shape}, vel {arrs[3].shape} do not "
                                 f"describe {nb} blocks")
            keep.append(arrs)
            for tab, a in zip((bp, ob, rh, vl), arrs):
                tab[li] = a.ctypes.data if a.size else None
        h = C.c_void_p()
        _lib.check(self._lib.ludwig_flow_source_create(int(device), n, dims.ctypes.data, nbs.ctypes.data, bp, ob, rh, vl, C.byref(h)))
        self._h = h

    @classmethod
    def from_levels(cls, levels: Sequence, t_coarse: int) -> "DeviceFlowSource":
        """the newest state of DeviceLevels (all of a hierarchy, level index 0 first) after coarse step t_coarse, copied on the device"""
        from . import _lib
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self.n_levels = len(levels)
        arr = (C.c_void_p * len(levels))(*[lv.handle for lv in levels])
        h = C.c_void_p()
        _lib.check(self._lib.ludwig_flow_source_from_levels(arr, len(levels), int(t_coarse), C.byref(h)))
        self._h = h
        return self


def resolve_state_path(path: str, case_dir: Optional[str]) -> str:
    """advanced.initial_condition.state is relative to the case folder"""
    return path if os.path.isabs(path) or not case_dir else os.path.join(case_dir, path)
