"""Time-step control: host mirror of src/solver_control.jl (the caller of the drop-in boundary).

Same call order and buffer parity as the reference: per level, iseven(t_sub) picks (f, vel) as input and
(f_temp, vel_temp) as output, else swapped (:35-41); a level with children saves its input state before it steps
(:46-48) and then steps its child twice, at 2*t_sub with temporal weight 0.0 and at 2*t_sub+1 with 0.5 (:63-83).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from .blocks import DeviceLevel, has_temporal_storage
from .physics import SolverParams, perform_timestep_v2


def recursive_step_temporal(grids: Sequence[DeviceLevel], current_lvl: int, t_sub: int,
                            parent: Optional[DeviceLevel], parent_tau, temporal_weight, u_vel,
                            params: SolverParams) -> None:
    """recursive_step_temporal! (src/solver_control.jl:86-143). current_lvl is 1-based."""
    if current_lvl > len(grids):
        return
    level = grids[current_lvl - 1]
    has_children = current_lvl < len(grids)
    if has_children and params.use_temporal_interp and has_temporal_storage(level):
        level.copy_to_old(t_sub)                       # copy_to_old!(level, f_in, vel_in)
    perform_timestep_v2(level, parent, parent_tau, u_vel, params, t_sub, temporal_weight)
    if has_children:
        recursive_step_temporal(grids, current_lvl + 1, 2 * t_sub, level, level.tau, np.float32(0.0), u_vel, params)
        recursive_step_temporal(grids, current_lvl + 1, 2 * t_sub + 1, level, level.tau, np.float32(0.5), u_vel, params)


def recursive_step(grids: Sequence[DeviceLevel], current_lvl: int, t_sub: int, parent: Optional[DeviceLevel],
                   parent_tau, u_vel, params: SolverParams) -> None:
    """recursive_step! (src/solver_control.jl:21-84): the same body with the temporal weight fixed at 0.0f0."""
    recursive_step_temporal(grids, current_lvl, t_sub, parent, parent_tau, np.float32(0.0), u_vel, params)


def execute_timestep_batch(grids: Sequence[DeviceLevel], t_start: int, batch_size: int, u_curr,
                           params: SolverParams, native: bool = True, probes=None, surface=None, forces=None, tracers=None) -> None:
    """execute_timestep_batch! (src/solver_control.jl:145-165); t_start is 1-based like the reference's loop.

    native=True (default): the whole batch is one C call (ludwig_execute_timestep_batch runs the same recursion inside
    the library, so a multi-level coarse step is not paced by Python). native=False: the recursion of this module, call
    by call - the two are tested to give identical results.
    probes: a probes.DeviceProbes made over `grids`, sampled after every coarse step start_step + k interval (native: inside the C
    batch, ludwig_execute_timestep_batch_probes; else through its sample() after the coarse step) - the same bits either way.
    surface: a surface_stats.DeviceSurfaceStats on one of `grids`, sampled after every coarse step start_step + k interval (native:
    inside the C batch, ludwig_execute_timestep_batch_sampled; else through its accumulate() after the coarse step).
    forces: a force_series.DeviceForceSeries on one of `grids`, sampled after every coarse step start_step + k interval (native: inside
    the C batch, ludwig_execute_timestep_batch_loads; else through its sample() after the coarse step).
    tracers: a tracers.DeviceTracers made over `grids`, advanced behind every coarse step start_step + k interval (native: inside the C
    batch, ludwig_execute_timestep_batch_tracers; else through its advance() after the coarse step) - the same bits either way."""
    if native:
        import ctypes as C
        from . import _lib
        arr = (C.c_void_p * len(grids))(*[g.handle for g in grids])
        fl = params.to_c()
        if surface is not None or forces is not None:
            smp = _lib.BatchSamplers(probes.handle.value if probes is not None else None, probes.start_step if probes is not None else 0,
                                     probes.interval if probes is not None else 1, surface.handle.value if surface is not None else None,
                                     surface.start_step if surface is not None else 0, surface.interval if surface is not None else 1)
        if tracers is not None:
            any_sampler = probes is not None or surface is not None
            if any_sampler and surface is None and forces is None:
                smp = _lib.BatchSamplers(probes.handle.value, probes.start_step, probes.interval, None, 0, 1)
            _lib.check(_lib.load().ludwig_execute_timestep_batch_tracers(arr, len(grids), int(t_start), int(batch_size),
                                                                         float(np.float32(u_curr)), C.byref(fl),
                                                                         C.byref(smp) if any_sampler else None,
                                                                         forces.handle if forces is not None else None,
                                                                         forces.start_step if forces is not None else 0,
                                                                         forces.interval if forces is not None else 1, tracers.handle,
                                                                         tracers.start_step, tracers.interval))
        elif forces is not None:
            _lib.check(_lib.load().ludwig_execute_timestep_batch_loads(arr, len(grids), int(t_start), int(batch_size),
                                                                       float(np.float32(u_curr)), C.byref(fl), C.byref(smp), forces.handle,
                                                                       forces.start_step, forces.interval))
        elif surface is not None:
            _lib.check(_lib.load().ludwig_execute_timestep_batch_sampled(arr, len(grids), int(t_start), int(batch_size),
                                                                         float(np.float32(u_curr)), C.byref(fl), C.byref(smp)))
        elif probes is None:
            _lib.check(_lib.load().ludwig_execute_timestep_batch(arr, len(grids), int(t_start), int(batch_size),
                                                                 float(np.float32(u_curr)), C.byref(fl)))
        else:
            _lib.check(_lib.load().ludwig_execute_timestep_batch_probes(arr, len(grids), int(t_start), int(batch_size),
                                                                        float(np.float32(u_curr)), C.byref(fl), probes.handle,
                                                                        probes.start_step, probes.interval))
        return
    from .statistics import t_sub_after
    for t_offset in range(batch_size):
        t = t_start + t_offset
        recursive_step(grids, 1, t, None, np.float32(0.5), u_curr, params)
        if probes is not None and t >= probes.start_step and (t - probes.start_step) % probes.interval == 0:
            for lvl in probes.levels_with_probes:
                probes.sample(lvl, t_sub_after(lvl, t))
        if surface is not None and surface.is_sample_step(t):
            surface.accumulate(t_sub_after(surface.level_index, t))
        if forces is not None and forces.is_sample_step(t):
            forces.sample(t_sub_after(forces.level_index, t), t)
        if tracers is not None and tracers.is_advance_step(t):
            tracers.advance(t)
    grids[0].synchronize()                             # KernelAbstractions.synchronize(backend)


def ramp_velocity(batch_end: int, ramp_steps: int, u_target) -> np.float32:
    """Inlet-speed ramp, evaluated once per batch at batch_end (src/main.jl:173-174), Float32 throughout."""
    if batch_end <= ramp_steps:
        arg = np.float32(np.pi) * np.float32(batch_end) / np.float32(ramp_steps)
        prog = np.float32(0.5) * (np.float32(1.0) - np.float32(np.cos(np.float64(arg))))
    else:
        prog = np.float32(1.0)
    return np.float32(u_target) * prog
