"""Case driver: the time loop of src/main.jl:169-232 around the HIP engine (YAML + STL in, Cd/Cl series out).

Loop semantics kept from the reference: steps run in batches of
`gpu.async_depth`; the inlet speed is the cosine ramp evaluated ONCE per batch at `batch_end`; diagnostics fire when
`batch_end % diag_freq < batch_length` and look at the state at batch END (stats from level 1's `rho`, forces from the
finest level's `rho` and `vel` buffer).

The stepping backend is injected (`stepper`), so the same loop drives the HIP library (HipStepper, the product path)
and, in tests only, the CPU oracle.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np

from . import flux_planes as flux_mod
from . import force_series as fseries_mod
from . import forces as forces_mod
from . import isosurface as iso_mod
from . import modes as modes_mod
from . import monitor as monitor_mod
from . import probes as probes_mod
from . import slices as slices_mod
from . import render as render_mod
from . import streamlines as stream_mod
from . import tracers as tracer_mod
from . import statistics as stats_mod
from . import subgrid as subgrid_mod
from . import surface_stats as surface_mod
from . import wall_diagnostics as wall_mod
from . import warm_start as warm_mod
from . import _lib
from .blocks import adapt
from .preprocess import CaseConfig, DomainParameters, setup_multilevel_domain, solver_params
from .solver_control import execute_timestep_batch, ramp_velocity


@dataclass
class DiagRow:
    step: int
    u_lat: float
    rho_min: float
    cd: float
    cl: float
    cs: float = 0.0
    cmy: float = 0.0


def _close_observers(st) -> None:
    """close a stepper's probe, surface, slice, wall-surface, force-series, streamline, tracer, flux-plane, mode and render sets (each
    may be None or absent)"""
    for name in ("probes", "surface", "slices", "wall_surface", "forces", "stream_set", "tracer_set", "fluxes", "modes", "render_set"):
        obs = getattr(st, name, None)
        if obs is not None:
            obs.close()
            setattr(st, name, None)


class HipStepper:
    """grids on one MI355X behind libludwig_hip.so"""

    def __init__(self, host_grids, device: int = 0, upload_state: bool = False):
        """upload_state: start from the host grids' own state arrays instead of the rest state run_case starts from"""
        self.host = host_grids
        self.dev = [adapt(g, device, upload_state=upload_state) for g in host_grids]
        if not upload_state:
            for d in self.dev:
                d.init_equilibrium()           # src/main.jl:126-135 (every state array: nothing of the host's to upload first)
        self.probes = None                     # probes_setup
        self._series = None
        self.surface = None                    # surface_stats_setup
        self.slices = None                     # slices_setup
        self.wall_surface = None               # wall_diagnostics_setup
        self.forces = None                     # force_series_setup
        self._fseries = None
        self._surface_plan = None              # (mesh, params, plan) of the surface statistics, shared with the force series
        self.stream_set = None                 # streamlines_setup
        self.tracer_set = None                 # tracers_setup
        self.fluxes = None                     # flux_planes_setup
        self._flux_series = None
        self.modes = None                      # modes_setup
        self.render_set = None                 # render_setup

    def batch(self, t_start: int, n: int, u_curr, params) -> None:
        if self.probes is None and self.forces is None and self.fluxes is None:
            execute_timestep_batch(self.dev, t_start, n, u_curr, params, surface=self.surface, tracers=self.tracer_set, modes=self.modes)
            return
        # sampled inside the C batch, the rings drained after it; a batch with more samples than a ring holds is cut where the first one
        # fills (the same inlet speed: the same steps, the same bits)
        P, F, X, t, end = self.probes, self.forces, self.fluxes, t_start, t_start + n - 1
        while t <= end:
            seg_end = end
            for ring in (P, F, X):
                if ring is not None:
                    seg_end = min(seg_end, fseries_mod.segment_end(t, end, ring.start_step, ring.interval, ring.capacity))
            execute_timestep_batch(self.dev, t, seg_end - t + 1, u_curr, params, probes=P, surface=self.surface, forces=F,
                                   tracers=self.tracer_set, fluxes=X, modes=self.modes)
            if P is not None:
                self._series.append(*P.download())
            if F is not None:
                self._fseries.append(*F.download())
            if X is not None:
                self._flux_series.append(*X.download())
            t = seg_end + 1

    # -- warm start (warm_start.py; no reference counterpart) --
    def flow_source(self, t_coarse: int):
        """a warm_start.DeviceFlowSource of every level's newest state after coarse step t_coarse, copied on the device"""
        return warm_mod.DeviceFlowSource.from_levels(self.dev, t_coarse)

    def init_from(self, state_or_source, first_step: int, maps, vel_scale=1.0, fallback=(1.0, 0.0, 0.0, 0.0)):
        """fill every level from a warm_start.FlowState (uploaded for the call) or a DeviceFlowSource; maps: one map [6] per level
        (warm_start.affine_map). The run then continues at coarse step first_step: f = f_temp, so the A/B parity of that step finds the
        same state either way. -> the counts of every level (DeviceLevel.init_from_source)"""
        if int(first_step) < 1:
            raise ValueError(f"initial condition: first_step {first_step} < 1")
        own = isinstance(state_or_source, warm_mod.FlowState)
        src = warm_mod.DeviceFlowSource(state_or_source, self.dev[0].device) if own else state_or_source
        try:
            return [d.init_from_source(src, maps[li], vel_scale, fallback) for li, d in enumerate(self.dev)]
        finally:
            if own:
                src.close()

    # -- probes (no reference counterpart) --
    def probes_setup(self, plan, start_step: int = 1, interval: int = 1, capacity: int = 64) -> None:
        """sample the probes of `plan` (probes.plan_probes over this stepper's grids) at coarse steps start_step + k interval"""
        if self.probes is not None:
            self.probes.close()
        self.probes = probes_mod.DeviceProbes(plan, self.dev, capacity, start_step, interval)
        self._series = probes_mod.Series(plan.n)

    def probes_series(self):
        """(coarse steps [n] int64, values [n, n_probes, 4] float32: rho, ux, uy, uz) of every sample so far"""
        return self._series.arrays()

    # -- surface statistics (no reference counterpart) --
    def surface_stats_setup(self, mesh, params, start_step: int = 1, interval: int = 1):
        """accumulate the wall loads of `mesh` on the finest level at coarse steps start_step + k interval, inside every batch; returns
        the surface_stats.SurfacePlan"""
        fin = len(self.host) - 1
        plan = surface_mod.plan_surface(mesh, self.host[fin], params)
        if self.surface is not None:
            self.surface.close()
        self.surface = surface_mod.DeviceSurfaceStats(plan, self.dev[fin], fin, self.host[fin].tau, params, max(int(start_step), 1), interval)
        self._surface_plan = (mesh, params, plan)
        return plan

    def surface_stats_sums(self):
        """(sums [7, n_tri] Float64, samples) of the surface set"""
        return self.surface.download()

    # -- force series (no reference counterpart) --
    def force_series_setup(self, mesh, params, start_step: int = 1, interval: int = 1, capacity: int = 64):
        """record the integrated loads of `mesh` on the finest level at coarse steps start_step + k interval, inside every batch; reuses
        the surface statistics' plan when that observer was set up with this very mesh and params object (else it plans anew); returns
        the surface_stats.SurfacePlan"""
        fin = len(self.host) - 1
        cached = self._surface_plan
        if cached is not None and cached[0] is mesh and cached[1] is params:
            plan = cached[2]
        else:
            plan = surface_mod.plan_surface(mesh, self.host[fin], params)
        if self.forces is not None:
            self.forces.close()
        self.forces = fseries_mod.from_mesh(mesh, plan, self.dev[fin], fin, self.host[fin].tau, params, max(int(start_step), 1), interval,
                                            capacity)
        self._fseries = fseries_mod.Series()
        return plan

    def force_series(self):
        """(coarse steps [n] int64, sums [n, 9] Float64: Fp(3), Fv(3), M(3), covered [n] int64) of every record so far"""
        return self._fseries.arrays()

    def force_series_new(self):
        """the same, of the records drained since the last force_series_new() only (what run_case writes after a batch)"""
        return self._fseries.take_new()

    # -- flux planes (no reference counterpart) --
    def flux_planes_setup(self, plans, start_step: int = 1, interval: int = 1, capacity: int = 64) -> None:
        """reduce the planes of `plans` (flux_planes.plan_flux_plane over this stepper's grids) at coarse steps start_step + k interval,
        inside every batch"""
        if self.fluxes is not None:
            self.fluxes.close()
        self.fluxes = flux_mod.DeviceFluxPlanes(plans, self.dev, capacity, max(int(start_step), 1), interval)
        self._flux_series = flux_mod.Series(len(plans))

    def flux_planes_new(self):
        """(coarse steps [n] int64, sums [n, n_planes, 8] Float64, counts [n, n_planes] int64) of the samples drained since the last
        flux_planes_new() (what run_case writes after a batch)"""
        return self._flux_series.take_new()

    # -- Fourier modes (modes.py; no reference counterpart) --
    def modes_setup(self, W, start_step: int = 1, interval: int = 1) -> None:
        """one device set over every level with the weight table W [n_samples, n_columns] (modes.weight_table). From now on every batch
        adds the state after the coarse steps start_step + k interval times row k % n_samples, inside the C call; a batch must end with
        a window at the latest (run_case cuts there) and the caller resets before the next one."""
        if self.modes is not None:
            self.modes.close()
        self.modes = _lib.ModeSet(self.dev, W, max(int(start_step), 1), interval)

    def modes_reset(self) -> None:
        self.modes.reset()

    def modes_sample(self, t_coarse: int) -> None:
        """between batches: add every level's newest state after coarse step t_coarse with the row of that step (queued)"""
        row = modes_mod.row_of(t_coarse, self.modes.start_step, self.modes.interval, self.modes.n_rows)
        for lvl in range(len(self.dev)):
            self.modes.accumulate(lvl, stats_mod.t_sub_after(lvl, t_coarse), row)

    def modes_sums(self, level: int):
        """(the sums of every table column [n_columns][8,8,8,nb,4] Float64 in the reference layout: rho, ux, uy, uz; samples)"""
        got = [self.modes.download(level, m) for m in range(self.modes.n_columns)]
        return [a for a, _ in got], got[0][1]

    # -- slices (no reference counterpart) --
    def slices_setup(self, plans, start_step: int = 1, interval: int = 1) -> None:
        """one device set over the planes of `plans` (slices.plan_slice over this stepper's grids); the caller samples after the
        coarse steps start_step + k interval (run_case cuts its batches there)"""
        self._slice_steps = slices_mod.check_schedule(start_step, interval)
        if self.slices is not None:
            self.slices.close()
        self.slices = slices_mod.DeviceSlices(plans, self.dev, self.host)

    def slices_sample(self, t_coarse: int):
        """sample every plane on the newest state after coarse step t_coarse (the last batch must have ended there; ValueError if
        t_coarse is no sampled step): one [rows, n] float32 array per plane (slices.ROWS)"""
        slices_mod.check_sample_step(t_coarse, *self._slice_steps)
        self.slices.sample(t_coarse)
        return self.slices.download()

    # -- wall diagnostics (no reference counterpart) --
    def wall_diagnostics_setup(self, mesh, params, plan=None):
        """a wall-surface set for `mesh` on the finest level; plan: the surface statistics' SurfacePlan when that observer is on too
        (one plan, not two). Returns the plan. The census needs no setup."""
        fin = len(self.host) - 1
        if plan is None:
            plan = surface_mod.plan_surface(mesh, self.host[fin], params)
        if self.wall_surface is not None:
            self.wall_surface.close()
        self.wall_surface = wall_mod.DeviceWallSurface(plan, self.dev[fin], params)
        return plan

    def wall_census(self, level: int, t_coarse: int):
        """the wall_diagnostics.Census of a level's newest state after coarse step t_coarse (the last batch must have ended there)"""
        return wall_mod.census(self.dev[level], stats_mod.t_sub_after(level, t_coarse))

    def wall_surface_values(self, t_coarse: int) -> np.ndarray:
        """[7, n_tri] float32 (wall_diagnostics.ROWS) of the finest level's newest state after coarse step t_coarse"""
        self.wall_surface.compute(stats_mod.t_sub_after(len(self.host) - 1, t_coarse))
        return self.wall_surface.download()

    def field(self, level: int, name: str) -> np.ndarray:
        return self.dev[level].download(name)

    def surface_stresses(self, level: int, mesh, params, search_radius: int = 5):
        """per-triangle p, tau on the device (src/forces/surface.jl:138-266); reads the level's `vel` buffer like the reference"""
        h = self.host[level]
        return forces_mod.map_surface_stresses_device(mesh, self.dev[level], h.dx, h.tau, params, search_radius, "vel")

    def rho_min(self, level: int) -> float:
        """compute_flow_stats (src/diagnostics.jl:56-94), reduced on the device"""
        return self.dev[level].rho_min()

    def monitor(self, level: int, t_coarse: int):
        """the monitor.Record of a level's newest state after coarse step t_coarse (the last batch must have ended there), reduced on
        the device"""
        return self.dev[level].monitor(stats_mod.t_sub_after(level, t_coarse))

    # -- time-averaged statistics (no reference counterpart) --
    def stats_reset(self) -> None:
        for d in self.dev:
            d.stats_reset()

    def stats_sample(self, t_coarse: int) -> None:
        """add every level's newest state after coarse step t_coarse to its device sums (queued, no synchronisation)"""
        for lvl, d in enumerate(self.dev):
            d.stats_accumulate(stats_mod.t_sub_after(lvl, t_coarse))

    def stats_sums(self, level: int):
        """(S_rho, S_u, S_uu, n) of a level, Float64 in the reference layout"""
        d = self.dev[level]
        (r, n), (u, _), (uu, _) = (d.stats_download(k) for k in ("rho", "vel", "vel2"))
        return r, u, uu, n

    def statistics(self, level: int):
        """finalised statistics of a level (statistics.finalize)"""
        return stats_mod.finalize(*self.stats_sums(level))

    # -- velocity-gradient fields (no reference counterpart for the output) --
    def gradient_fields(self, level: int, vel_name: str, scale):
        """(vorticity [8,8,8,nb,3], Q [8,8,8,nb]) of a level from its `vel_name` buffer, derivatives times `scale` (Float32)"""
        return self.dev[level].gradient_fields(vel_name, scale)

    # -- iso-surfaces (isosurface.py; no reference counterpart) --
    def isosurfaces_setup(self, start_step: int = 1, interval: int = 1) -> None:
        """the caller extracts after the coarse steps start_step + k interval (run_case cuts its batches there); nothing is allocated
        before the first extraction"""
        self._iso_steps = iso_mod.check_schedule(start_step, interval)

    def isosurface(self, level: int, field: str, value, t_coarse: int, skip=None, cell_lo=(0, 0, 0), cell_hi=None,
                   max_triangles: int = 50_000_000, download: bool = True):
        """DeviceLevel.isosurface of a level's newest state after coarse step t_coarse (the last batch must have ended there), with
        derivatives per unit length (scale 1/dx): (n_triangles, positions, attributes, keys), the arrays None when refused"""
        vel_name = "vel_temp" if stats_mod.t_sub_after(level, t_coarse) % 2 == 0 else "vel"
        return self.dev[level].isosurface(field, value, vel_name, np.float32(1.0 / self.host[level].dx), skip, cell_lo, cell_hi,
                                          max_triangles, download)

    # -- streamlines (streamlines.py; no reference counterpart) --
    def streamlines_setup(self, seeds, sign, step=0.5, min_speed=1.0e-6, max_steps: int = 2000, start_step: int = 1,
                          interval: int = 1) -> None:
        """one device set over every level: seeds [n, 3] float32 in cell units of level 1 (streamlines.seed_positions), sign [n] +-1;
        the caller traces after the coarse steps start_step + k interval (run_case cuts its batches there)"""
        self._stream_steps = stream_mod.check_schedule(start_step, interval)
        if self.stream_set is not None:
            self.stream_set.close()
        self.stream_set = stream_mod.DeviceStreamlines(self.dev, seeds, sign, step, min_speed, max_steps)

    def streamlines(self, t_coarse: int):
        """trace every line through the newest state of all levels after coarse step t_coarse (the last batch must have ended there):
        (counts [n], codes [n], records [n, max_steps + 1, 8])"""
        self.stream_set.trace(t_coarse)
        return self.stream_set.download()

    # -- volume images (render.py; no reference counterpart) --
    def render_setup(self, max_pixels: int, start_step: int = 1, interval: int = 1) -> None:
        """one device set over every level with room for max_pixels pixels; the caller renders after the coarse steps start_step + k
        interval (run_case cuts its batches there)"""
        render_mod.check_schedule(start_step, interval)
        if self.render_set is not None:
            self.render_set.close()
        self.render_set = render_mod.DeviceRender(self.dev, max_pixels)

    def render(self, plan, t_coarse: int):
        """one image of a view (render.ViewPlan) of the newest state of all levels after coarse step t_coarse (the last batch must have
        ended there), derivatives per unit length as in the flow file: (rgba [h, w, 4], codes [h, w], samples [h, w])"""
        self.render_set.image(t_coarse, plan.field, render_mod.level_scales(self.host), **plan.arguments())
        return self.render_set.download()

    # -- tracers (tracers.py; no reference counterpart) --
    def tracers_setup(self, seeds, generations: int = 1, release_every: int = 1, start_step: int = 1, interval: int = 1) -> None:
        """one device set over every level: seeds [n, 3] float32 in cell units of level 1 (streamlines.seed_positions). From now on
        every batch advances it behind the coarse steps start_step + k interval, inside the C call."""
        tracer_mod.check_schedule(start_step, interval, release_every, generations)
        if self.tracer_set is not None:
            self.tracer_set.close()
        self.tracer_set = tracer_mod.DeviceTracers(self.dev, seeds, generations, release_every, start_step, interval)

    def tracers_snapshot(self, t_coarse: int):
        """(records [n_slots, 8], advances so far) on the newest state of all levels after coarse step t_coarse (the last batch must
        have ended there); changes nothing of the set"""
        self.tracer_set.snapshot(t_coarse)
        return self.tracer_set.download()

    # -- subgrid model (subgrid.py; no reference counterpart for the output) --
    def subgrid_fields(self, level: int, vel_name: str):
        """(nu_t [8,8,8,nb], branch code as a float [8,8,8,nb]) of a level from its `vel_name` buffer (Float32)"""
        return self.dev[level].subgrid_fields(vel_name)

    def subgrid_stats_reset(self) -> None:
        for d in self.dev:
            d.subgrid_stats_reset()

    def subgrid_stats_sample(self, t_coarse: int) -> None:
        """add the model's state on every level's newest velocity after coarse step t_coarse to its device sums (queued)"""
        for lvl, d in enumerate(self.dev):
            d.subgrid_stats_accumulate(stats_mod.t_sub_after(lvl, t_coarse))

    def subgrid_stats_sums(self, level: int):
        """(S_nu, S_nunu, S_eps, n) of a level, Float64 in the reference layout"""
        d = self.dev[level]
        (a, n), (b, _), (c, _) = (d.subgrid_stats_download(k) for k in ("nu", "nunu", "eps"))
        return a, b, c, n

    def close(self):
        _close_observers(self)
        for d in self.dev:
            d.close()


class DistributedStepper:
    """grids spread over the ranks of the default torch.distributed group, one MI355X per rank (scope row N3): every
    level is cut on its own into equal parts (partition.level_owners; pass `owners` to choose otherwise), halo +
    parent-data ghosts move after every level step (partition.MultiLevelRunner).

    Diagnostics follow SURVEY section 8e: nothing but scalars crosses ranks on a diagnostics step.
      * rho_min: every rank reduces its owned level-1 cells on its device, one all-reduce MIN.
      * forces: the fluid cell a triangle reads (map_stresses_kernel!, src/forces/surface.jl:138-266) depends on the geometry
        only, so it is found once, on the host, from the global obstacle mask every rank holds; a triangle belongs to the rank
        that owns that cell. Per diagnostics step a rank gathers rho, u of ITS cells on its device (4 floats per owned
        triangle), evaluates the stresses and the nine Float32 sums of integrate_forces_kernel! over its triangles, and one
        all-gather of 10 floats per rank follows; every rank adds the partial sums in rank order. The sums of a rank are
        pairwise Float32 sums over its triangles, so the total differs from the single-device row by Float32 rounding of a
        different summation order (observed <= 1e-6 relative) - bit-equality with one device is traded for not moving fields.
    `field()` still assembles a GLOBAL array, on rank 0 only; it is used on VTU output steps."""

    def __init__(self, host_grids, device: Optional[int] = None, owners=None, stage_through_host: bool = False,
                 overlap: Optional[bool] = None, transport: Optional[str] = None):
        import torch
        import torch.distributed as dist
        from . import partition
        self.dist, self.partition, self.torch = dist, partition, torch
        self.host = host_grids
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.device = device if device is not None else int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(self.device)
        self.owners = owners if owners is not None else partition.level_owners(host_grids, self.world)
        self.stage = stage_through_host
        # overlap: each level's exchange runs under the part of its blocks that reads no ghost (partition.MultiLevelRunner);
        # LUDWIG_NO_OVERLAP=1 (or overlap=False) falls back to step -> exchange -> wait, level by level. transport: "native" = RCCL
        # called from the library (default with the nccl backend), "torch" = torch.distributed from Python (the gloo rehearsals).
        self.overlap = (os.environ.get("LUDWIG_NO_OVERLAP") is None) if overlap is None else bool(overlap)
        self.transport = transport
        self.runner = None
        self._tri = {}                         # level -> static triangle map (see surface_forces)
        self._probe_cfg = None                 # probes_setup: (plan, start_step, interval, capacity)
        self.probes = None                     # this rank's probe set (None: it owns no probe)
        self._surface_cfg = None               # surface_stats_setup: (plan, params, start_step, interval)
        self.surface = None                    # this rank's surface set (None: it holds no copy of the finest level)
        self._slice_plans = None               # slices_setup: the global plans
        self.slices = None                     # this rank's slice set (None: it owns no base block of a valid point)
        self._wall_cfg = None                  # wall_diagnostics_setup: (plan, params)
        self.wall_surface = None               # this rank's wall-surface set (None: it holds no copy of the finest level)
        self._forces_cfg = None                # force_series_setup: (mesh, plan, params, start_step, interval, capacity)
        self.forces = None                     # this rank's force-series set (None: it holds no copy of the finest level)
        self._modes_cfg = None                 # modes_setup: (W, start_step, interval)
        self.modes = None                      # this rank's mode set over the levels it owns blocks of (None: it owns none)
        self._modes_levels = []                # those levels' indices

    def _level_owner(self, level: int) -> np.ndarray:
        g = self.host[level]
        return np.asarray(self.owners[level] if not isinstance(self.owners, np.ndarray) else
                          self.partition.ancestor_owner(g.level_id, g.active_block_coords, self.host[0].active_block_coords, self.owners))

    def _gather(self, mine):
        """one object per rank to rank 0: the list of them there, None elsewhere; collective"""
        parts = [None] * self.world if self.rank == 0 else None
        self.dist.gather_object(mine, parts, dst=0)
        return parts

    def _owned_g2l(self, level: int) -> np.ndarray:
        """global -> local block index of the blocks this rank OWNS on a level; -1 for every other block, its ghosts included"""
        view = self.runner.views[level]
        g2l = np.full(self.host[level].n_blocks, -1, dtype=np.int64)
        g2l[view.local_to_global[: view.n_owned]] = np.arange(view.n_owned)
        return g2l

    def _owning(self, level: int):
        """(device level, view) of a level this rank holds and owns blocks of, else None"""
        lv, view = self.runner.levels[level], self.runner.views[level]
        return (lv, view) if lv is not None and view.n_owned > 0 else None

    @staticmethod
    def _owned_blocks(view, arrays):
        """(local_to_global of a view's owned blocks, their part of every [8, 8, 8, n_local, ...] array): what _scatter_blocks places"""
        return view.local_to_global[: view.n_owned], [a[:, :, :, : view.n_owned] for a in arrays]

    @staticmethod
    def _scatter_blocks(parts, outs) -> None:
        """the ranks' gathered (local_to_global of the owned blocks, one [8, 8, 8, n_owned, ...] array per output, ...) into the global
        arrays `outs` (block axis 3); a rank that owns nothing sent None"""
        for part in parts:
            if part is not None:
                for o, a in zip(outs, part[1]):
                    o[:, :, :, part[0]] = a

    @staticmethod
    def _scatter_columns(parts, outs) -> None:
        """the same along the LAST axis: the ranks' gathered (columns, one [..., n_columns] array per output, ...) into `outs`"""
        for part in parts:
            if part is not None:
                for o, a in zip(outs, part[1:]):
                    o[..., part[0]] = a

    @staticmethod
    def _samples(parts) -> int:
        """the sample count the gathered parts end with (every rank that sent one counted the same samples); 0 when nobody did"""
        return ([0] + [part[-1] for part in parts if part is not None])[-1]

    def _start(self, params) -> None:
        probe_cells, mine = None, None
        if self._probe_cfg is not None:
            # a probe belongs to the rank that owns its base cell's block; its corners in a peer's block are read from the ghost copy,
            # so they join the level's 'rho' and 'vel' halo
            plan = self._probe_cfg[0]
            base_owner = np.array([self._level_owner(int(l))[b] for l, b in zip(plan.level, plan.blocks[:, 0])], dtype=np.int64)
            mine = np.flatnonzero(base_owner == self.rank)
            probe_cells = [np.zeros(0, np.int64) for _ in self.host]
            for p in mine:
                li = int(plan.level[p])
                probe_cells[li] = np.concatenate([probe_cells[li], plan.blocks[p].astype(np.int64) * 512 + plan.cells[p]])
        if self._slice_plans is not None:
            # the same halo rule for slice points: their stencil cells (and face neighbours) in ghost blocks join 'rho' and 'vel'
            self._slice_mine_cache = self._slice_mine()
            extra = self._slice_cells()
            probe_cells = extra if probe_cells is None else [np.concatenate([a, b]) for a, b in zip(probe_cells, extra)]
        self.runner = self.partition.MultiLevelRunner(self.host, self.owners, params, self.rank, self.world, self.device, self.stage,
                                                      overlap=self.overlap, transport=self.transport, upload_state=False,
                                                      probe_cells=probe_cells)
        for lv in self.runner.levels:
            if lv is not None:
                lv.init_equilibrium()          # src/main.jl:126-135 (ghost blocks included: same rest state everywhere)
        if mine is not None and mine.size:
            plan, start, interval, capacity = self._probe_cfg
            local = plan.subset(mine)
            for p in range(local.n):
                g2l = self.runner.views[int(local.level[p])].global_to_local
                local.blocks[p] = [g2l[int(b)] for b in local.blocks[p]]
            self.probes = probes_mod.DeviceProbes(local, self.runner.levels, capacity, start, interval)
            self._probe_cols = mine
            self._probe_pending = 0
            self._series = probes_mod.Series(local.n)          # this rank's probes, in the order of _probe_cols
        if self._surface_cfg is not None:
            self._surface_create()
        if self._slice_plans is not None:
            self._slices_create()
        if self._wall_cfg is not None:
            self._wall_surface_create()
        if self._forces_cfg is not None:
            self._forces_create()
        if self._modes_cfg is not None:
            self._modes_create()

    def batch(self, t_start: int, n: int, u_curr, params) -> None:
        if self.runner is None:
            self._start(params)
        self.runner.params = params
        P, S, F, M = self.probes, self.surface, self.forces, self.modes
        fin = len(self.host) - 1
        for t in range(t_start, t_start + n):
            self.runner.step(t, u_curr)
            if M is not None and stats_mod.is_sample_step(t, M.start_step, M.interval):
                self._modes_accumulate(t)      # owned blocks only: no ghost is read, nothing to join
            if S is not None and S.is_sample_step(t):
                self.runner.join(fin)
                S.accumulate(stats_mod.t_sub_after(fin, t))
            if P is not None and probes_mod.is_sample_step(t, P.start_step, P.interval):
                if self._probe_pending == P.capacity:
                    self._series.append(*P.download())
                    self._probe_pending = 0
                for lvl in P.levels_with_probes:
                    self.runner.join(lvl)     # the level's ghosts (peer corners) are in place
                    P.sample(lvl, stats_mod.t_sub_after(lvl, t))
                self._probe_pending += 1
            if F is not None and F.is_sample_step(t):
                if self._force_pending == F.capacity:
                    self._fseries.append(*F.download())
                    self._force_pending = 0
                self.runner.join(fin)
                F.sample(stats_mod.t_sub_after(fin, t), t)
                self._force_pending += 1
        self.runner.synchronize()
        if P is not None:
            self._series.append(*P.download())
            self._probe_pending = 0
        if F is not None:
            self._fseries.append(*F.download())
            self._force_pending = 0

    # -- probes: each rank samples the probes whose base cell it owns; the series is gathered to rank 0 in probe order --
    def probes_setup(self, plan, start_step: int = 1, interval: int = 1, capacity: int = 64) -> None:
        """before the first batch: the probe corners change the halo plans, which the first batch builds"""
        if self.runner is not None:
            raise RuntimeError("DistributedStepper.probes_setup must come before the first batch")
        self._probe_cfg = (plan, int(start_step), int(interval), int(capacity))

    def probes_series(self):
        """(coarse steps [n] int64, values [n, n_probes, 4] float32) on rank 0 (None elsewhere); collective. Valid at any time after
        probes_setup, also before the first batch or the first sampled step (then n = 0)."""
        mine = None
        if self.probes is not None:
            steps, vals = self._series.arrays()
            mine = (self._probe_cols, steps, vals)
        parts = self._gather(mine)
        if parts is None:
            return None
        n_total = self._probe_cfg[0].n
        got = [p for p in parts if p is not None]
        steps = got[0][1] if got else np.zeros(0, np.int64)
        out = np.full((steps.size, n_total, 4), np.nan, dtype=np.float32)
        for cols, st, vals in got:
            assert np.array_equal(st, steps), "ranks sampled different steps"
            assert vals.shape == (steps.size, len(cols), 4)
            out[:, cols] = vals
        return steps, out

    # -- slices: each rank samples the points whose base cell's block it owns; corners and their face neighbours in a peer's blocks are
    # read from the ghost copies, which the 'rho' / 'vel' halo refreshes; the samples are gathered to rank 0 in plane order --
    def slices_setup(self, plans, start_step: int = 1, interval: int = 1) -> None:
        """before the first batch: the stencil cells change the halo plans, which the first batch builds"""
        if self.runner is not None:
            raise RuntimeError("DistributedStepper.slices_setup must come before the first batch")
        self._slice_steps = slices_mod.check_schedule(start_step, interval)
        self._slice_plans = list(plans)

    def _slice_mine(self):
        """per plan: bool [n], the valid points whose base block this rank owns"""
        out = []
        for plan in self._slice_plans:
            mine = np.zeros(plan.n, bool)
            for li in np.unique(plan.level[plan.valid]):
                sel = np.flatnonzero(plan.valid & (plan.level == li))
                mine[sel] = self._level_owner(int(li))[plan.blocks[sel, 0]] == self.rank
            out.append(mine)
        return out

    def _slice_cells(self):
        """per level, the global cells (block * 512 + cell) this rank's slice points read"""
        cells = [[] for _ in self.host]
        for plan, mine in zip(self._slice_plans, self._slice_mine_cache):
            for li in np.unique(plan.level[mine]):
                cells[int(li)].append(slices_mod.stencil_cells(plan, np.flatnonzero(mine & (plan.level == li)), self.host[int(li)]))
        return [np.concatenate(c) if c else np.zeros(0, np.int64) for c in cells]

    def _slices_create(self) -> None:
        # on purpose over owned AND ghost blocks (not _owned_g2l): a point's corners may lie in a peer's blocks, read from the ghost copies
        g2l = []
        for g, v in zip(self.host, self.runner.views):
            a = np.full(g.n_blocks, -1, dtype=np.int64)
            if v is not None:
                a[np.asarray(v.local_to_global)] = np.arange(len(v.local_to_global))
            g2l.append(a)
        local = [slices_mod.local_plan(p, m, g2l) for p, m in zip(self._slice_plans, self._slice_mine_cache)]
        if not any(p.valid.any() for p in local):
            return
        # as with probes: the sampled levels store rho every step, so a sample never replays an elided store over the ghost rho the
        # halo has just refreshed
        for li in sorted({int(l) for p in local for l in p.level[p.valid]}):
            self.runner.levels[li].set_rho_store(True)
        self.slices = slices_mod.DeviceSlices(local, self.runner.levels, self.host)

    def slices_sample(self, t_coarse: int):
        """every plane sampled after coarse step t_coarse (the last batch must have ended there), one [rows, n] float32 array per plane
        on rank 0 (None elsewhere); collective"""
        slices_mod.check_sample_step(t_coarse, *self._slice_steps)
        mine = None
        if self.slices is not None:
            self.slices.sample(t_coarse)
            vals = self.slices.download()
            mine = [(np.flatnonzero(m), v[:, m]) for m, v in zip(self._slice_mine_cache, vals)]
        parts = self._gather(mine)
        if parts is None:
            return None
        rows = slices_mod.ROWS_GRAD if any(p.gradient for p in self._slice_plans) else slices_mod.ROWS_BASIC
        out = [np.zeros((rows, p.n), dtype=np.float32) for p in self._slice_plans]
        for k, o in enumerate(out):
            self._scatter_columns([part and part[k] for part in parts], [o])
        return out

    # -- surface statistics: each rank accumulates the triangles whose cell it owns (the rule of _triangle_map); per-triangle sums do
    # not depend on the partition, so the gathered sums are one device's bit for bit --
    def surface_stats_setup(self, mesh, params, start_step: int = 1, interval: int = 1):
        """returns the global surface_stats.SurfacePlan; the rank's set is made with the first batch (or now, after it)"""
        if int(interval) < 1:
            raise ValueError(f"surface statistics: interval {interval} < 1")
        fin = len(self.host) - 1
        plan = surface_mod.plan_surface(mesh, self.host[fin], params)
        if self.surface is not None:
            self.surface.close()
            self.surface = None
        self._surface_cfg = (plan, params, max(int(start_step), 1), int(interval))
        if self.runner is not None:
            self._surface_create()
        return plan

    def _surface_share(self, plan):
        """(sel, local): the triangles of a SurfacePlan whose cell this rank owns (the rule of _triangle_map), and the plan of those
        alone with the finest level's blocks renumbered to this rank's owned ones; local is None where the rank holds no copy of that
        level (a level held without an owned block still gets its empty set: it counts the samples)"""
        fin = len(self.host) - 1
        sel = np.flatnonzero(plan.found & (self._level_owner(fin)[np.maximum(plan.blocks, 0)] == self.rank))
        if self.runner.levels[fin] is None:
            assert sel.size == 0
            return sel, None
        local = plan.subset(sel)
        local.blocks = self._owned_g2l(fin)[local.blocks].astype(np.int32)
        assert (local.blocks >= 0).all()
        return sel, local

    def _surface_create(self) -> None:
        plan, params, start, interval = self._surface_cfg
        fin = len(self.host) - 1
        self._surface_sel, local = self._surface_share(plan)
        if local is not None:
            self.surface = surface_mod.DeviceSurfaceStats(local, self.runner.levels[fin], fin, self.host[fin].tau, params, start, interval)

    def surface_stats_sums(self):
        """(sums [7, n_tri] Float64 in triangle order, samples) on rank 0 (None elsewhere); collective"""
        plan = self._surface_cfg[0]
        mine = None
        if self.surface is not None:
            sums, n = self.surface.download()
            mine = (self._surface_sel, sums, n)
        parts = self._gather(mine)
        if parts is None:
            return None
        out = np.zeros((len(surface_mod.COMPONENTS), plan.n), dtype=np.float64)
        self._scatter_columns(parts, [out])
        return out, self._samples(parts)

    # -- force series: each rank reduces the triangles whose cell it owns (the rule of _triangle_map) in global triangle order; a
    # triangle without a cell adds signed zeros only and belongs to nobody. The ranks' records are added in rank order in Float64 on
    # rank 0: other trees than one device's, so the sums agree to Float64 rounding, not bit for bit; the coverage count is exact --
    def force_series_setup(self, mesh, params, start_step: int = 1, interval: int = 1, capacity: int = 64):
        """returns the global surface_stats.SurfacePlan (the surface statistics' when that observer was set up first); the rank's set
        is made with the first batch (or now, after it)"""
        if int(interval) < 1:
            raise ValueError(f"force series: interval {interval} < 1")
        fin = len(self.host) - 1
        plan = self._surface_cfg[0] if self._surface_cfg is not None else surface_mod.plan_surface(mesh, self.host[fin], params)
        if self.forces is not None:
            self.forces.close()
            self.forces = None
        self._forces_cfg = (mesh, plan, params, max(int(start_step), 1), int(interval), int(capacity))
        self._fseries_total = fseries_mod.Series()                   # rank 0: the gathered history
        if self.runner is not None:
            self._forces_create()
        return plan

    def _forces_create(self) -> None:
        mesh, plan, params, start, interval, capacity = self._forces_cfg
        fin = len(self.host) - 1
        self._forces_sel, local = self._surface_share(plan)
        if local is None:
            return
        self.forces = fseries_mod.from_mesh(mesh, local, self.runner.levels[fin], fin, self.host[fin].tau, params, start, interval, capacity,
                                            select=self._forces_sel)
        self._fseries = fseries_mod.Series()
        self._force_pending = 0

    def force_series_new(self):
        """(coarse steps [n] int64, sums [n, 9] Float64, covered [n] int64) of the records drained since the last force_series_new(),
        on rank 0 (None elsewhere); collective. Only these records cross the ranks; rank 0 keeps the history."""
        parts = self._gather(self._fseries.take_new() if self.forces is not None else None)
        if parts is None:
            return None
        got = [p for p in parts if p is not None]
        if not got:
            return np.zeros(0, np.int64), np.zeros((0, 9), np.float64), np.zeros(0, np.int64)
        steps = got[0][0]
        sums = np.zeros((steps.size, 9), dtype=np.float64)
        cov = np.zeros(steps.size, dtype=np.int64)
        for st, s9, c in got:                  # rank order
            assert np.array_equal(st, steps), "ranks sampled different steps"
            sums = sums + s9
            cov = cov + c
        self._fseries_total.append(steps, sums, cov)
        return steps, sums, cov

    def force_series(self):
        """the same of every record so far, on rank 0 (None elsewhere); collective (it gathers what is new first)"""
        return None if self.force_series_new() is None else self._fseries_total.arrays()

    # -- wall diagnostics: every rank takes the census of its owned blocks (integer records: their sum is one device's) and evaluates the
    # triangles whose cell it owns (the rule of _triangle_map; the model's stencil is the cell itself: no ghost is read) --
    def wall_diagnostics_setup(self, mesh, params, plan=None):
        """returns the global surface_stats.SurfacePlan; the rank's set is made with the first batch (or now, after it)"""
        fin = len(self.host) - 1
        if plan is None:
            plan = surface_mod.plan_surface(mesh, self.host[fin], params)
        if self.wall_surface is not None:
            self.wall_surface.close()
            self.wall_surface = None
        self._wall_cfg = (plan, params)
        if self.runner is not None:
            self._wall_surface_create()
        return plan

    def _wall_surface_create(self) -> None:
        plan, params = self._wall_cfg
        self._wall_sel, local = self._surface_share(plan)
        if local is not None:
            self.wall_surface = wall_mod.DeviceWallSurface(local, self.runner.levels[len(self.host) - 1], params)

    def wall_census(self, level: int, t_coarse: int):
        """the wall_diagnostics.Census of the GLOBAL level after coarse step t_coarse on rank 0 (None elsewhere): the ranks' records
        gathered and merged (wall_diagnostics.merge), exactly one device's; collective"""
        held = self._owning(level)
        parts = self._gather(wall_mod.census(held[0], stats_mod.t_sub_after(level, t_coarse)) if held else None)
        return None if parts is None else wall_mod.merge(parts)

    def wall_surface_values(self, t_coarse: int):
        """[7, n_tri] float32 in triangle order on rank 0 (None elsewhere); a triangle without a cell holds the documented zeros;
        collective"""
        plan = self._wall_cfg[0]
        mine = None
        if self.wall_surface is not None:
            self.wall_surface.compute(stats_mod.t_sub_after(len(self.host) - 1, t_coarse))
            mine = (self._wall_sel, self.wall_surface.download())
        parts = self._gather(mine)
        if parts is None:
            return None
        out = np.zeros((len(wall_mod.ROWS), plan.n), dtype=np.float32)
        self._scatter_columns(parts, [out])
        return out

    # -- collectives of a few scalars --
    def _comm_device(self):
        return self.torch.device("cuda", self.device) if self.dist.get_backend() == "nccl" else self.torch.device("cpu")

    def rho_min(self, level: int) -> float:
        held = self._owning(level)
        mine = held[0].rho_min() if held else float("inf")
        # a diverged rank reports NaN (the reference's minimum() propagates it, src/diagnostics.jl:71); what MIN makes of a NaN is
        # the backend's business, so it travels as a flag: [min of the finite values, -1 if any rank saw NaN], one all-reduce MIN
        nan = mine != mine
        t = self.torch.tensor([float("inf") if nan else mine, -1.0 if nan else 0.0], dtype=self.torch.float32, device=self._comm_device())
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN)
        return float("nan") if float(t[1].item()) < 0 else float(t[0].item())

    def monitor(self, level: int, t_coarse: int):
        """the monitor.Record of the GLOBAL level after coarse step t_coarse, on every rank: each rank reduces its owned blocks on its
        device, the small records are gathered and merged on rank 0 (monitor.merge) and the result is sent back; collective"""
        held = self._owning(level)
        parts = self._gather(held[0].monitor(stats_mod.t_sub_after(level, t_coarse)) if held else None)
        out = [monitor_mod.merge(parts) if self.rank == 0 else None]
        self.dist.broadcast_object_list(out, src=0)
        return out[0]

    def _triangle_map(self, level: int, mesh, params, search_radius: int):
        key = (level, search_radius)
        if key not in self._tri:
            g, view = self.host[level], self.runner.views[level]
            nc = forces_mod.nearest_fluid_cells(mesh, g.obstacle, g.block_pointer, g.dx, params, search_radius)
            sel = np.flatnonzero(nc.found & (self._level_owner(level)[nc.block] == self.rank))
            lb = self._owned_g2l(level)[nc.block[sel]]
            assert (lb >= 0).all()
            cell = nc.lx[sel] + 8 * nc.ly[sel] + 64 * nc.lz[sel] + 512 * lb
            sk = 512 * view.level.n_blocks
            dev = self.torch.device("cuda", self.device)
            idx = {"rho": self.torch.as_tensor(cell, dtype=self.torch.int64, device=dev),
                   "vel": self.torch.as_tensor(np.concatenate([cell, cell + sk, cell + 2 * sk]), dtype=self.torch.int64, device=dev)}
            buf = {k: self.torch.empty(v.numel(), dtype=self.torch.float32, device=dev) for k, v in idx.items()}
            self._tri[key] = (nc, sel, idx, buf)
        return self._tri[key]

    def surface_forces(self, level: int, mesh, params, symmetric: bool, search_radius: int = 5, want_maps: bool = False):
        """compute_aerodynamics! (src/forces/surface.jl:592-600) without moving fields: see the class docstring."""
        import ctypes as C
        from . import _lib
        nc, sel, idx, buf = self._triangle_map(level, mesh, params, search_radius)
        lv, g = self.runner.levels[level], self.host[level]
        lib = _lib.load()
        stream = C.c_void_p(self.torch.cuda.current_stream(self.torch.device("cuda", self.device)).cuda_stream)
        if sel.size:
            for name in ("rho", "vel"):      # the level's `vel` buffer, like the reference (src/forces/surface.jl:412)
                _lib.check(lib.ludwig_halo_pack(lv.handle, _lib.FIELD_NAMES[name], C.c_void_p(idx[name].data_ptr()), idx[name].numel(),
                                                C.c_void_p(buf[name].data_ptr()), stream))
            rho_c = buf["rho"].cpu().numpy()
            u_c = buf["vel"].cpu().numpy().reshape(3, -1).T
        else:
            rho_c, u_c = np.zeros(0, np.float32), np.zeros((0, 3), np.float32)
        p, tx, ty, tz = forces_mod.stress_from_cells(rho_c, np.ascontiguousarray(u_c), nc.wall_dist[sel], np.ones(sel.size, bool),
                                                      mesh.normals[sel], g.tau, params)
        part = np.zeros(10, dtype=np.float32)
        part[:9] = forces_mod.partial_force_sums(mesh, p, tx, ty, tz, params, select=sel)
        part[9] = forces_mod.coverage_count(p)
        total, cov = forces_mod.combine_partial_sums(part, self._comm_device())      # fixed order: rank 0, 1, ...
        fr = forces_mod.finish_forces(total, cov, params, symmetric)
        if want_maps:                          # output steps only: per-triangle loads to rank 0 for the surface VTU
            parts = self._gather((sel, p, tx, ty, tz))
            if parts is not None:
                n = mesh.centers.shape[0]
                maps = [np.zeros(n, dtype=np.float32) for _ in range(4)]
                self._scatter_columns(parts, maps)
                fr.maps = tuple(maps)
        return fr

    def field(self, level: int, name: str) -> Optional[np.ndarray]:
        """GLOBAL array of a field, assembled on rank 0 (None elsewhere): result files only, never per diagnostics step."""
        held = self._owning(level)
        parts = self._gather(self._owned_blocks(held[1], [held[0].download(name)]) if held else None)
        if parts is None:
            return None
        ref = getattr(self.host[level], name)
        out = np.zeros(ref.shape, dtype=ref.dtype, order="F")
        self._scatter_blocks(parts, [out])
        return out

    # -- time-averaged statistics: every rank accumulates its owned blocks; results gathered like field() --
    def _held(self):
        return [(lvl, self._owning(lvl)[0]) for lvl in range(len(self.host)) if self._owning(lvl)]

    def stats_reset(self) -> None:
        for _, lv in self._held():
            lv.stats_reset()

    def stats_sample(self, t_coarse: int) -> None:
        for lvl, lv in self._held():
            lv.stats_accumulate(stats_mod.t_sub_after(lvl, t_coarse))

    def stats_sums(self, level: int):
        """(S_rho, S_u, S_uu, n) of the GLOBAL level, assembled on rank 0 (None elsewhere); collective"""
        held, mine = self._owning(level), None
        if held:
            got = [held[0].stats_download(k) for k in ("rho", "vel", "vel2")]
            mine = self._owned_blocks(held[1], [a for a, _ in got]) + (got[0][1],)
        parts = self._gather(mine)
        if parts is None:
            return None
        nb = self.host[level].n_blocks
        out = [np.zeros((8, 8, 8, nb) + ((k,) if k > 1 else ()), dtype=np.float64, order="F") for k in (1, 3, 6)]
        self._scatter_blocks(parts, out)
        n = self._samples(parts)
        return out[0], out[1], out[2], n

    def statistics(self, level: int):
        """finalised statistics of a level on rank 0 (None elsewhere); collective"""
        sums = self.stats_sums(level)
        return None if sums is None else stats_mod.finalize(*sums)

    # -- Fourier modes: every rank accumulates the blocks it owns, inside batch() after each coarse step's level steps; the sums are
    # gathered like the statistics'. No ghost is read, so no halo group changes --
    def modes_setup(self, W, start_step: int = 1, interval: int = 1) -> None:
        self._modes_cfg = (np.ascontiguousarray(W, dtype=np.float64), max(int(start_step), 1), int(interval))
        if self.runner is not None:
            self._modes_create()

    def _modes_create(self) -> None:
        if self.modes is not None:
            self.modes.close()
            self.modes = None
        held = self._held()
        self._modes_levels = [lvl for lvl, _ in held]
        if held:
            self.modes = _lib.ModeSet([lv for _, lv in held], *self._modes_cfg)

    def _modes_accumulate(self, t_coarse: int) -> None:
        M = self.modes
        row = modes_mod.row_of(t_coarse, M.start_step, M.interval, M.n_rows)
        for i, lvl in enumerate(self._modes_levels):
            M.accumulate(i, stats_mod.t_sub_after(lvl, t_coarse), row)

    def modes_reset(self) -> None:
        if self.modes is not None:
            self.modes.reset()

    def modes_sample(self, t_coarse: int) -> None:
        """between batches: every rank adds its owned blocks' newest state after coarse step t_coarse"""
        if self.modes is not None:
            self._modes_accumulate(t_coarse)

    def modes_sums(self, level: int):
        """(the sums of every table column of the GLOBAL level, samples), assembled on rank 0 (None elsewhere); collective"""
        mine = None
        if self.modes is not None and level in self._modes_levels:
            i = self._modes_levels.index(level)
            got = [self.modes.download(i, m) for m in range(self.modes.n_columns)]
            mine = self._owned_blocks(self.runner.views[level], [a for a, _ in got]) + (got[0][1],)
        parts = self._gather(mine)
        if parts is None:
            return None
        out = [np.zeros((8, 8, 8, self.host[level].n_blocks, 4), dtype=np.float64, order="F") for _ in range(self._modes_cfg[0].shape[1])]
        self._scatter_blocks(parts, out)
        n = self._samples(parts)
        return out, n

    # -- velocity-gradient fields: every rank computes on its owned blocks after batch() (its 'vel' halo ghosts are current for
    # both buffers: each level step exchanges the buffer it wrote, and nothing writes that buffer again before the next such step) --
    def gradient_fields(self, level: int, vel_name: str, scale):
        """(vorticity, Q) of the GLOBAL level, assembled on rank 0 (None elsewhere); collective"""
        held = self._owning(level)
        parts = self._gather(self._owned_blocks(held[1], held[0].gradient_fields(vel_name, scale)) if held else None)
        if parts is None:
            return None
        nb = self.host[level].n_blocks
        w_all = np.zeros((8, 8, 8, nb, 3), dtype=np.float32, order="F")
        q_all = np.zeros((8, 8, 8, nb), dtype=np.float32, order="F")
        self._scatter_blocks(parts, [w_all, q_all])
        return w_all, q_all

    # -- iso-surfaces: not over ranks. A cube reads the first layer of seven neighbour blocks; on a rank's ghost blocks the gradient
    # fields do not exist and rho / vel are current only where a halo asks for them --
    def isosurfaces_setup(self, start_step: int = 1, interval: int = 1) -> None:
        raise RuntimeError("advanced.isosurfaces is enabled, but a distributed run cannot extract iso-surfaces yet: ghost blocks hold no "
                           "gradient fields and only part of rho / vel (DESIGN section 8, Next)")

    # -- warm start: not over ranks (a state holds whole levels; each rank holds only its own blocks) --
    def state_files_setup(self, *args, **kwargs) -> None:
        raise RuntimeError("advanced.state_files is enabled, but a distributed run cannot write state files yet: each rank holds only "
                           "its own blocks of a level")

    def init_from(self, *args, **kwargs):
        raise RuntimeError("advanced.initial_condition is set, but a distributed run cannot start from a state file yet: the source "
                           "hierarchy would have to be held by every rank")

    def flow_source(self, *args, **kwargs):
        raise RuntimeError("a distributed run cannot make a flow source (advanced.initial_condition, advanced.state_files): each rank "
                           "holds only its own blocks of a level")

    # -- streamlines: not over ranks. A line wanders through every level and every block, and a rank holds only its own --
    def streamlines_setup(self, *args, **kwargs) -> None:
        raise RuntimeError("advanced.streamlines is enabled, but a distributed run cannot trace streamlines yet: a line crosses the "
                           "ranks' blocks, and each rank holds only its own (DESIGN section 8, Next)")

    # -- volume images: not over ranks, for the streamlines' reason: a ray crosses every level of every rank --
    def render_setup(self, *args, **kwargs) -> None:
        raise RuntimeError("advanced.render is enabled, but a distributed run cannot render images yet: a ray crosses the ranks' "
                           "blocks, and each rank holds only its own (DESIGN section 8, Next)")

    # -- flux planes: not over ranks - a record is one tree over a plane's points in point order, not a sum of per-rank parts --
    def flux_planes_setup(self, *args, **kwargs) -> None:
        raise RuntimeError("advanced.flux_planes is enabled, but a distributed run cannot integrate flux planes yet: a record is one "
                           "fixed tree over a plane's points in point order, not a sum of the ranks' parts")

    # -- tracers: not over ranks, for the streamlines' reason --
    def tracers_setup(self, *args, **kwargs) -> None:
        raise RuntimeError("advanced.tracers is enabled, but a distributed run cannot advect tracers yet: a particle crosses the ranks' "
                           "blocks, and each rank holds only its own (DESIGN section 8, Next)")

    # -- subgrid model: every rank works on its owned blocks after batch(); the face stencil is the gradient fields', so their argument
    # holds unchanged (the 'vel' halo ghosts are current for both buffers) --
    def subgrid_fields(self, level: int, vel_name: str):
        """(nu_t, code) of the GLOBAL level, assembled on rank 0 (None elsewhere); collective"""
        held = self._owning(level)
        parts = self._gather(self._owned_blocks(held[1], held[0].subgrid_fields(vel_name)) if held else None)
        if parts is None:
            return None
        out = [np.zeros((8, 8, 8, self.host[level].n_blocks), dtype=np.float32, order="F") for _ in range(2)]
        self._scatter_blocks(parts, out)
        return out[0], out[1]

    def subgrid_stats_reset(self) -> None:
        for _, lv in self._held():
            lv.subgrid_stats_reset()

    def subgrid_stats_sample(self, t_coarse: int) -> None:
        for lvl, lv in self._held():
            lv.subgrid_stats_accumulate(stats_mod.t_sub_after(lvl, t_coarse))

    def subgrid_stats_sums(self, level: int):
        """(S_nu, S_nunu, S_eps, n) of the GLOBAL level, assembled on rank 0 (None elsewhere); collective"""
        held, mine = self._owning(level), None
        if held:
            got = [held[0].subgrid_stats_download(k) for k in ("nu", "nunu", "eps")]
            mine = self._owned_blocks(held[1], [a for a, _ in got]) + (got[0][1],)
        parts = self._gather(mine)
        if parts is None:
            return None
        out = [np.zeros((8, 8, 8, self.host[level].n_blocks), dtype=np.float64, order="F") for _ in range(3)]
        self._scatter_blocks(parts, out)
        n = self._samples(parts)
        return out[0], out[1], out[2], n

    def close(self):
        _close_observers(self)
        if self.runner is not None:
            self.runner.close()          # plans, communicator, levels; the views and plans stay readable (statistics)


def _aerodynamics(st, grids, mesh, params, symmetric: bool, rho_f=None, want_maps: bool = False):
    """compute_aerodynamics! (src/forces/surface.jl:592-600) on the finest level: stresses on the device when the stepper
    offers it, else from downloaded fields; integration on the host either way. A distributed stepper reduces per rank."""
    fin = len(grids) - 1
    if hasattr(st, "surface_forces"):
        return st.surface_forces(fin, mesh, params, symmetric, want_maps=want_maps)
    if hasattr(st, "surface_stresses"):
        p, tx, ty, tz = st.surface_stresses(fin, mesh, params)
        fr = forces_mod.integrate_surface_forces(mesh, p, tx, ty, tz, params, symmetric)
        fr.maps = (p, tx, ty, tz)
        return fr
    if rho_f is None:
        rho_f = st.field(fin, "rho")
    return forces_mod.compute_aerodynamics(mesh, grids[fin], rho_f, st.field(fin, "vel"), params, symmetric)


def flow_stats(rho: np.ndarray, obstacle: np.ndarray) -> float:
    """rho_min of compute_flow_stats (src/diagnostics.jl:56-94, CUDA branch): minimum over non-obstacle cells"""
    return float(rho[~obstacle].min())


def _refuse_device_only(st, cfg: CaseConfig) -> None:
    """RuntimeError, naming the key and the missing method, for the first enabled feature that needs a method this stepper lacks"""
    eddy_on = "EddyViscosityRatio" in cfg.output_fields
    for on, key, method, what in (
            (cfg.initial_condition_state, "advanced.initial_condition is set", "init_from", "a level is filled from a state file"),
            (cfg.fourier_modes_enabled, "advanced.fourier_modes is enabled", "modes_setup", "the Fourier modes are accumulated"),
            (cfg.wall_diagnostics_enabled, "advanced.wall_diagnostics is enabled", "wall_diagnostics_setup",
             "the wall diagnostics are evaluated"),
            (eddy_on or cfg.statistics_subgrid,
             ("basic.simulation.output_fields.eddy_viscosity" if eddy_on else "advanced.statistics.subgrid") + " is set", "subgrid_fields",
             "the subgrid model's eddy viscosity is evaluated"),
            (cfg.forces_series_enabled, "advanced.forces.series is enabled", "force_series_setup", "the force series is reduced")):
        if on and not hasattr(st, method):
            raise RuntimeError(f"{key}, but {type(st).__name__} offers no {method}: {what} on the device only")


def _every(start_step: int, interval: int):
    """steps_in(t, batch_end) of a cut schedule: the coarse steps start_step + k interval of a batch"""
    return lambda t, batch_end: stats_mod.sample_steps(t, batch_end, start_step, interval)


def run_case(cfg: CaseConfig, stepper_factory: Callable = HipStepper, steps: Optional[int] = None, stl_path: Optional[str] = None,
             log: Optional[Callable[[str], None]] = None, setup=None, out_dir: Optional[str] = None, write_files: bool = True):
    """solve_main (src/main.jl:54-249). Returns (rows, setup_report, params).

    out_dir: when given, the reference's result files are written there (row N4): convergence.csv and forces.csv at every
    diagnostics step, flow_%06d.vtu (+ surface_%06d.vtu) every `output_freq` steps, and with cfg.statistics_enabled
    flow_mean_%06d.vtu (the average over the samples so far, statistics.py) on those steps once a sample exists; "Vorticity" /
    "QCriterion" in cfg.output_fields add those arrays to the flow file, computed on the device from the file's velocity buffer with
    derivatives per unit length of the file's coordinates (scale 1/dx). Unlike the reference (main.jl:79) an
    existing directory is NOT emptied first. write_files=False on all ranks but one of a distributed run.
    With cfg.probes_enabled, probes_points.csv is written once and probes.csv gains the new samples at every diagnostics step and at
    the end of the run (probes.py); batches are not cut for probes.
    With cfg.surface_statistics_enabled, the finest level's wall loads are accumulated per triangle (surface_stats.py) - inside the
    batches where the stepper offers surface_stats_setup, else on the host from downloaded fields with batches cut at the sampled
    steps - and every output step once a sample exists writes surface_mean_%06d.vtu and a forces_mean.csv row.
    With cfg.slices_enabled, every plane is sampled after the coarse steps start_step + k interval - batches are cut there with the
    batch's own inlet speed - on the device where the stepper offers slices_setup, else from downloaded fields (slices.host_sample);
    each sample is written to slice_<name>_%06d.vti and listed in slice_<name>.pvd (slices.py).
    With cfg.isosurfaces_enabled, every surface is extracted after the coarse steps start_step + k interval - batches are cut there as for
    slices - from the newest state of every level that exports blocks, with the blocks the flow file drops skipped: on the device where
    the stepper offers isosurface, else from downloaded fields (isosurface.extract_host). The levels are merged in ascending order into
    iso_<name>_%06d.vtp, listed in iso_<name>.pvd; a sample of more than max_triangles triangles writes no file and logs one line
    (isosurface.py). A stepper whose isosurfaces_setup raises (the distributed one) ends the run before the first step.
    With cfg.streamlines_enabled, every seed group's lines are traced after the coarse steps start_step + k interval - batches are cut
    there as for slices - through the newest state of all levels: on the device where the stepper offers streamlines, else from
    downloaded fields (streamlines.trace_host). Each group is written to stream_<name>_%06d.vtp, listed in stream_<name>.pvd; lines of
    fewer than two vertices are left out of the file and counted in the log (streamlines.py). A stepper whose streamlines_setup raises
    (the distributed one) ends the run before the first step.
    With cfg.render_enabled, every view is rendered after the coarse steps start_step + k interval - batches are cut there as for
    slices - from the newest state of all levels: on the device where the stepper offers render, else from downloaded fields
    (render.host_image). Each image is written to render_<name>_%06d.png and logs its rays per end code and its samples (render.py). A
    stepper whose render_setup raises (the distributed one) ends the run before the first step.
    With cfg.tracers_enabled, the seed groups' particles are advanced behind the coarse steps start_step + k interval INSIDE the batches
    where the stepper offers tracers_setup - no batch is cut for an advance - and batches are cut only after the snapshot steps
    start_step + k output_interval, as for slices; a stepper without tracers_setup goes through tracers.HostTracers on downloaded
    velocity, cutting at every advance step. Each snapshot writes tracers_<name>_%06d.vtp per group, listed in tracers_<name>.pvd, and
    logs one line per group (tracers.py). A stepper whose tracers_setup raises (the distributed one) ends the run before the first step.
    With cfg.flow_monitor_enabled, a monitor.Record of every level is taken at every diagnostics step and after the last step, from the
    state at batch end (where rho_min is taken; no batch is cut) - on the device where the stepper offers monitor, else from downloaded
    fields (monitor.host_monitor); flow_monitor.csv gains one row per level and the warnings go to `log`. With
    cfg.flow_monitor_stop_on_divergence the run ends once a level holds non-finite fluid cells: that step's rows and files are
    written, then monitor.FlowDiverged is raised (on every rank of a distributed run).
    With cfg.wall_diagnostics_enabled, at every diagnostics step and after the last step, from the state at batch end (no batch is cut):
    a wall_diagnostics.Census of every level (when the wall model is on) into wall_model.csv and the forces of pressure plus modelled
    wall shear into wall_forces.csv; on flow output steps surface_%06d.vtu gains wall_diagnostics.finalize's arrays. Device only: a
    stepper without wall_diagnostics_setup raises.
    "EddyViscosityRatio" in cfg.output_fields adds nu_t / nu of the step's own WALE model (subgrid.py) to the flow file, Float32, from the
    file's velocity buffer.
    With cfg.forces_series_enabled (advanced.forces.series), the finest level's integrated loads are reduced on the device inside the
    batches at the coarse steps start_step + k interval (force_series.py) and forces_series.csv gains one row per sampled step after
    every batch, with that batch's inlet speed; `log` gets the mean and rms of Cd, Cl, Cmy over the rows after ramp_steps at the end. No
    batch is cut for it beyond the ring's capacity. Device only: a stepper without force_series_setup raises.
    With cfg.flux_planes_enabled (advanced.flux_planes), every plane and every box face is reduced at the coarse steps start_step + k
    interval (flux_planes.py): inside the batches where the stepper offers flux_planes_setup - no batch is cut beyond the ring's capacity -
    else from downloaded fields (flux_planes.host_sample), cutting batches there as for slices; after every batch fluxes.csv gains one row
    per plane and sampled step and flux_boxes.csv one per box. A stepper whose flux_planes_setup raises (the distributed one) ends the run
    before the first step.
    With cfg.statistics_subgrid the model's sums are sampled at exactly the flow statistics' sampled steps (same
    reset) and flow_mean_%06d.vtu gains subgrid.MEAN_ARRAYS after its own arrays. Device only: a stepper without subgrid_fields raises.
    With cfg.fourier_modes_enabled (advanced.fourier_modes), every level's rho and u are accumulated against the weight table of
    modes.plan_modes at the coarse steps start_step + k interval, inside the batches; window j covers the samples start_step + (j N + n)
    interval, n < N = samples. Batches are cut at a window's last step only - one cut per window, none for the samples. There the sums
    are downloaded, flow_modes_%06d.vtu (output.export_modes_mesh) and one flow_modes.csv row per mode and level are written, and with
    `repeat` the sums are reset for the next window (without it the set is closed). A window unfinished at the end of the run writes
    nothing and says so in `log`. Device only: a stepper without modes_setup raises.
    With cfg.state_files_enabled (advanced.state_files) and an out_dir, state_%06d.npz (warm_start.FlowState: rho and the newest velocity
    of every level, from downloaded fields) is written after the coarse steps that are multiples of `interval` and after the last step
    (interval 0: the last step only); batches are cut there as for slices.
    With cfg.initial_condition_state (advanced.initial_condition), after set-up and the rest state every level is filled from that state
    file on the device (warm_start.py: rho and u resampled, the populations at their equilibrium - NOT what a continued run would hold),
    `log` gets one line of counts per level, and the loop starts at coarse step first_step and runs `steps` steps from there: step
    numbers in every file count from first_step. Device only: a stepper without init_from raises."""
    import time as _time
    from . import output as out_mod
    grids, mesh, params, report = setup if setup is not None else setup_multilevel_domain(cfg, stl_path)
    sp = solver_params(cfg, params)
    writing = out_dir is not None and write_files
    fin = len(grids) - 1
    probes_on, slices_on, iso_on, stream_on = cfg.probes_enabled, cfg.slices_enabled, cfg.isosurfaces_enabled, cfg.streamlines_enabled
    render_on, tracers_on, flux_on, modes_on = cfg.render_enabled, cfg.tracers_enabled, cfg.flux_planes_enabled, cfg.fourier_modes_enabled
    surf_on, wall_on, fseries_on, monitor_on = (cfg.surface_statistics_enabled, cfg.wall_diagnostics_enabled, cfg.forces_series_enabled,
                                                cfg.flow_monitor_enabled)
    stats_on, subgrid_on, eddy_on = cfg.statistics_enabled, cfg.statistics_subgrid, "EddyViscosityRatio" in cfg.output_fields
    # probe points outside the domain or inside the body, a slice or flux plane outside the domain and a frequency the sampling cannot
    # resolve are refused before anything is allocated on a device
    pplan = probes_mod.plan_probes(cfg.probes_points, grids, params.mesh_offset, cfg.probes_names) if probes_on else None
    splans = [slices_mod.plan_slice(spec, grids, params.mesh_offset) for spec in cfg.slices_planes] if slices_on else []
    fplans = [flux_mod.plan_flux_plane(spec, grids, params.mesh_offset) for spec in cfg.flux_planes_planes] if flux_on else []
    mplan = modes_mod.plan_modes(cfg, params, log) if modes_on else None
    st = stepper_factory(grids)
    try:                                 # whatever fails from here on, the stepper is closed once
        _refuse_device_only(st, cfg)     # they depend on cfg and the stepper's type alone: a refused run allocates nothing
        first_step = int(cfg.initial_condition_first_step) if cfg.initial_condition_state else 1
        total_steps = first_step - 1 + (steps if steps is not None else cfg.steps)
        batch = cfg.async_depth

        def begin_csv(name, *header):
            """start out_dir's file `name` with its header line(s); nothing when this run writes no files"""
            if writing:
                with open(os.path.join(out_dir, name), "w") as io:
                    io.writelines(l + "\n" for l in header)

        def append_csv(name, lines):
            """append lines to out_dir's file `name`; nothing when this run writes no files (a generator is then not run) or has no lines"""
            lines = list(lines) if writing else []
            if lines:
                with open(os.path.join(out_dir, name), "a") as io:
                    io.writelines(l + "\n" for l in lines)

        # ---- set-up: the stepper's calls in a fixed order (the surface statistics before the two observers that share their plan) ----
        if cfg.state_files_enabled and hasattr(st, "state_files_setup"):
            st.state_files_setup()               # the distributed stepper refuses
        if cfg.initial_condition_state:
            ic_state = warm_mod.load_state(warm_mod.resolve_state_path(cfg.initial_condition_state, cfg.case_dir))
            ic_scale = cfg.initial_condition_velocity_scale
            if ic_scale is None:                 # auto: both runs' flows at their own lattice speed
                ic_scale = float(cfg.u_lattice) / ic_state.u_lattice
            ic_counts = st.init_from(ic_state, first_step, [warm_mod.affine_map(ic_state, g.dx, params.mesh_offset) for g in grids], ic_scale,
                                     (1.0, float(ramp_velocity(first_step, cfg.ramp_steps, cfg.u_lattice)), 0.0, 0.0))
            if log:
                log(f"initial condition: {cfg.initial_condition_state} (case {ic_state.case!r}, step {ic_state.step}, "
                    f"{ic_state.n_levels} levels), velocity scale {ic_scale:.6g}, first step {first_step}; the populations restart at "
                    "equilibrium")
                for g, c in zip(grids, ic_counts):
                    log(warm_mod.counts_line(g.level_id, c))
        if iso_on and hasattr(st, "isosurfaces_setup"):
            st.isosurfaces_setup(cfg.isosurfaces_start_step, cfg.isosurfaces_interval)
        if stream_on:
            stream_plan = stream_mod.SeedPlan([(s.name, np.asarray(s.points, dtype=np.float64)) for s in cfg.streamlines_seeds],
                                              cfg.streamlines_direction, params.mesh_offset, grids[0].dx)
            if hasattr(st, "streamlines_setup"):
                st.streamlines_setup(stream_plan.seeds, stream_plan.sign, cfg.streamlines_step, cfg.streamlines_min_speed,
                                     cfg.streamlines_max_steps, cfg.streamlines_start_step, cfg.streamlines_interval)
        if render_on:
            render_plans = [render_mod.ViewPlan(v, cfg.render_width, cfg.render_height, params.mesh_offset, grids[0].dx)
                            for v in cfg.render_views]
            if hasattr(st, "render_setup"):
                st.render_setup(cfg.render_max_pixels, cfg.render_start_step, cfg.render_interval)
        tr_start, tr_interval = cfg.tracers_start_step, cfg.tracers_interval
        tr_host = None                       # the host fallback (a stepper without tracers_setup)
        if tracers_on:
            tr_plan = tracer_mod.TracerPlan([(s.name, np.asarray(s.points, dtype=np.float64)) for s in cfg.tracers_seeds],
                                            params.mesh_offset, grids[0].dx)
            if hasattr(st, "tracers_setup"):
                st.tracers_setup(tr_plan.seeds, cfg.tracers_generations, cfg.tracers_release_every, tr_start, tr_interval)
            else:
                tr_host = tracer_mod.HostTracers(tr_plan.seeds, cfg.tracers_generations, cfg.tracers_release_every, tr_interval)
            warn = tracer_mod.jump_warning(tr_interval, float(cfg.u_lattice), len(grids))
            if warn and log:
                log(warn)
        dev_fluxes = flux_on and hasattr(st, "flux_planes_setup")      # else the host fallback from downloaded fields
        if dev_fluxes:
            st.flux_planes_setup(fplans, cfg.flux_planes_start_step, cfg.flux_planes_interval, max(batch, 1))
        if flux_on and cfg.flux_planes_boxes and cfg.symmetric_analysis and log:
            log("flux planes: symmetric_analysis is on; the control-volume force of a box is that of the modelled half, not doubled")
        if probes_on:
            st.probes_setup(pplan, cfg.probes_start_step, cfg.probes_interval, max(batch, 1))
        dev_slices = slices_on and hasattr(st, "slices_setup")
        if dev_slices:
            st.slices_setup(splans, cfg.slices_start_step, cfg.slices_interval)
        surf_start, surf_interval = cfg.surface_statistics_start_step, cfg.surface_statistics_interval
        surf_host = None                     # the host fallback (a stepper without surface_stats_setup)
        if surf_on:
            if hasattr(st, "surface_stats_setup"):
                splan = st.surface_stats_setup(mesh, params, surf_start, surf_interval)
            else:
                splan = surface_mod.plan_surface(mesh, grids[fin], params)
                surf_host = surface_mod.HostSurfaceStats(splan, grids[fin].tau, params, surf_start, surf_interval)
        if wall_on:
            st.wall_diagnostics_setup(mesh, params, splan if surf_on else None)      # one plan for both surface observers
        if fseries_on:                       # after the surface statistics: one plan for both
            st.force_series_setup(mesh, params, cfg.forces_series_start_step, cfg.forces_series_interval, max(batch, 1))
        if modes_on:
            st.modes_setup(mplan.W, mplan.start_step, mplan.interval)
        state_on = bool(cfg.state_files_enabled) and writing
        wall_band = cfg.wall_diagnostics_band

        # ---- the files this run starts ----
        if writing:
            os.makedirs(out_dir, exist_ok=True)
            if cfg.forces_enabled:
                out_mod.write_force_csv_header(os.path.join(out_dir, "forces.csv"))
            if slices_on:
                slice_writer = slices_mod.SliceWriter(out_dir, splans, params.time_scale)
            if stream_on:
                stream_writer = stream_mod.StreamlineWriter(out_dir, stream_plan, params.time_scale)
            if tracers_on:
                tracer_writer = tracer_mod.TracerWriter(out_dir, tr_plan, params.time_scale, cfg.tracers_generations,
                                                        cfg.tracers_release_every, tr_start, tr_interval)
            if iso_on:
                iso_writer = iso_mod.IsoWriter(out_dir, [s.name for s in cfg.isosurfaces_surfaces], params.time_scale)
            if probes_on:
                probes_mod.write_points_csv(os.path.join(out_dir, "probes_points.csv"), pplan, grids)
                begin_csv("probes.csv", probes_mod.series_csv_header(pplan.names))
            begin_csv("convergence.csv", out_mod.CONVERGENCE_CSV_HEADER)
            if surf_on:
                begin_csv("forces_mean.csv", surface_mod.FORCES_MEAN_CSV_HEADER)
            if fseries_on:
                begin_csv("forces_series.csv", fseries_mod.csv_header())
            if flux_on:
                begin_csv("fluxes.csv", flux_mod.FLUXES_CSV_HEADER)
            if flux_on and cfg.flux_planes_boxes:
                begin_csv("flux_boxes.csv", flux_mod.BOXES_CSV_COMMENT, flux_mod.BOXES_CSV_HEADER)
            if modes_on:
                begin_csv("flow_modes.csv", modes_mod.CSV_HEADER)
            if monitor_on:
                begin_csv("flow_monitor.csv", monitor_mod.CSV_HEADER)
            if wall_on:
                begin_csv("wall_model.csv", wall_mod.wall_model_csv_header(cfg.y_plus_target, wall_band))
                begin_csv("wall_forces.csv", wall_mod.WALL_FORCES_CSV_HEADER)

        # ---- what is taken at a diagnostics step, from the state at batch end ----
        def take_monitor(step, state_step):
            """a record of every level from the state after coarse step state_step; rows and warnings out; the first diverged level's
            FlowDiverged or None (collective in a distributed run)"""
            diverged = None
            for lvl, g in enumerate(grids):
                if hasattr(st, "monitor"):
                    rec = st.monitor(lvl, state_step)
                else:
                    vel_name = "vel_temp" if stats_mod.t_sub_after(lvl, state_step) % 2 == 0 else "vel"
                    rho_l, vel_l = st.field(lvl, "rho"), st.field(lvl, vel_name)
                    rec = monitor_mod.host_monitor(rho_l, vel_l, g.obstacle, g.active_block_coords) if rho_l is not None else None
                if rec is None:
                    continue
                if writing:
                    append_csv("flow_monitor.csv", [monitor_mod.csv_row(step, state_step, g.level_id, rec, g.dx, params.mesh_offset)])
                if log:
                    for line in monitor_mod.warnings_of(rec, step, g.level_id, g.dx, params.mesh_offset):
                        log(line)
                if rec.n_bad > 0 and diverged is None:
                    diverged = monitor_mod.FlowDiverged(step, g.level_id, rec.first_bad,
                                                        monitor_mod.cell_coordinates(rec.first_bad, g.dx, params.mesh_offset), rec.n_bad)
            return diverged
        wall_taken = [None, None]            # the coarse step of the last wall-surface values, and the values

        def wall_values(state_step):
            """the wall-surface values of the state after coarse step state_step, evaluated once per step (collective in a distributed run)"""
            if wall_taken[0] != state_step:
                wall_taken[:] = [state_step, st.wall_surface_values(state_step)]
            return wall_taken[1]

        def take_wall(step, state_step):
            """a census of every level (with the wall model on) and the modelled surface loads from the state after coarse step
            state_step; rows out (collective in a distributed run)"""
            if sp.wall_model_active:
                for lvl, g in enumerate(grids):
                    rec = st.wall_census(lvl, state_step)
                    if writing and rec is not None:
                        append_csv("wall_model.csv", [wall_mod.wall_model_csv_row(step, g.level_id, rec, wall_band)])
            vals = wall_values(state_step)
            if writing and vals is not None:
                fr_model = wall_mod.model_forces(mesh, vals, params, cfg.symmetric_analysis)
                append_csv("wall_forces.csv", [wall_mod.wall_forces_csv_row(step, mesh, vals, fr_model)])
        probes_written = [0]

        def flush_probes():
            """append the samples not yet in probes.csv (collective in a distributed run)"""
            series = st.probes_series()
            if writing and series is not None:
                p_steps, p_vals = series
                append_csv("probes.csv", probes_mod.series_csv_rows(p_steps[probes_written[0]:], p_vals[probes_written[0]:], params.time_scale))
                probes_written[0] = p_steps.size

        # ---- what is drained after every batch ----
        fseries_coeffs = []                  # (Cd, Cl, Cmy) of the rows after the ramp

        def flush_force_series(u_batch):
            """append the records the batch that has just ended drained - only those leave the stepper - to forces_series.csv (collective
            in a distributed run)"""
            series = st.force_series_new()
            if series is None:
                return
            f_steps, f_sums, f_cov = series
            lines = []
            for i in range(f_steps.size):
                fr_i = forces_mod.finish_forces(f_sums[i], int(f_cov[i]), params, cfg.symmetric_analysis)
                lines.append(fseries_mod.csv_row(int(f_steps[i]), float(f_steps[i]) * params.time_scale, fr_i, u_batch))
                if f_steps[i] > cfg.ramp_steps:
                    fseries_coeffs.append((fr_i.Cd, fr_i.Cl, fr_i.Cmy))
            append_csv("forces_series.csv", lines)
        flux_host = []                       # the host fallback's samples of the batch: (step, sums, counts)
        flux_box_cd = {}                     # box name -> Cd of the rows after the ramp

        def flush_fluxes():
            """append the samples the batch that has just ended took to fluxes.csv and flux_boxes.csv"""
            if dev_fluxes:
                f_steps, f_sums, f_counts = st.flux_planes_new()
            else:
                f_steps = np.array([s for s, _, _ in flux_host], dtype=np.int64)
                f_sums, f_counts = [a for _, a, _ in flux_host], [c for _, _, c in flux_host]
                flux_host.clear()
            plane_rows, box_rows, box_values = flux_mod.csv_rows(fplans, cfg.flux_planes_boxes, f_steps, f_sums, f_counts, params)
            for step, name, b in box_values:
                if step > cfg.ramp_steps:
                    flux_box_cd.setdefault(name, []).append(b.Cd)
            append_csv("fluxes.csv", plane_rows)
            append_csv("flux_boxes.csv", box_rows)

        # ---- what is taken at a cut: each take(step) acts on the state after coarse step `step` ----
        stats_window = [0, 0, 0]             # samples, first and last sampled step

        def take_statistics(step):
            """a sample of the flow statistics, and of the subgrid model's sums with them; start_step resets both"""
            if step == cfg.statistics_start_step:
                st.stats_reset()
                if subgrid_on:
                    st.subgrid_stats_reset()
                stats_window[:] = [0, step, step]
            st.stats_sample(step)
            if subgrid_on:
                st.subgrid_stats_sample(step)
            stats_window[0] += 1
            stats_window[2] = step

        def take_surface_host(step):
            """a sample of the host fallback's surface statistics from downloaded fields"""
            t_sub = stats_mod.t_sub_after(fin, step)
            surf_host.accumulate(st.field(fin, "rho"), st.field(fin, "vel_temp" if t_sub % 2 == 0 else "vel"))

        def take_slices(step):
            """every plane; files out"""
            got = st.slices_sample(step) if dev_slices else slices_mod.host_sample(st, splans, grids, step)
            if writing:
                slice_writer.write(step, got)
        if iso_on:
            iso_skips = iso_mod.skip_flags(grids)
            iso_boxes = {s.name: [iso_mod.cell_box(s.bounds, g.dx, params.mesh_offset) for g in grids] for s in cfg.isosurfaces_surfaces}

        def take_isosurfaces(step):
            """every surface, levels merged in ascending order; files out"""
            cap = int(cfg.isosurfaces_max_triangles)
            for spec in cfg.isosurfaces_surfaces:
                boxes = iso_boxes[spec.name]
                if hasattr(st, "isosurface"):
                    parts, total, refused = [], 0, False
                    for li, g in enumerate(grids):
                        if iso_skips[li].all():
                            continue
                        # once the cap is passed the remaining levels are only counted
                        n, pos, att, keys = st.isosurface(li, spec.field, spec.value, step, iso_skips[li], boxes[li][0], boxes[li][1],
                                                          0 if refused else cap - total)
                        total += n
                        if pos is None:
                            refused = True
                        else:
                            parts.append((li, g.dx, pos, att, keys))
                else:
                    parts = iso_mod.host_extract_levels(st, grids, spec.field, spec.value, step, boxes, iso_skips)
                    total = sum(p[2].shape[0] for p in parts)
                    refused = total > cap
                if refused:
                    if log:
                        log(f"isosurface {spec.name!r}: step {step}: {total} triangles, more than advanced.isosurfaces.max_triangles = "
                            f"{cap}; no file written")
                elif writing:
                    iso_writer.write(step, spec.name, iso_mod.merge_levels(parts))

        def take_streamlines(step):
            """every group's lines; files out, one log line per group"""
            if hasattr(st, "streamlines"):
                counts, codes, records = st.streamlines(step)
            else:
                counts, codes, records = stream_mod.trace_host(stream_mod.stepper_levels(st, grids, step), stream_plan.seeds,
                                                               stream_plan.sign, cfg.streamlines_step, cfg.streamlines_min_speed,
                                                               cfg.streamlines_max_steps)
            if writing:
                stream_writer.write(step, counts, codes, records)
            if log:
                for gi, name in enumerate(stream_plan.names):
                    log(f"streamlines {name!r}: step {step}: {stream_mod.summary(stream_plan, gi, counts, codes)}")

        def take_render(step):
            """every view; files out, one log line per image"""
            for plan in render_plans:
                rgba, codes, samples = st.render(plan, step) if hasattr(st, "render") else render_mod.host_image(st, grids, plan, step)
                if writing:
                    render_mod.write_png(os.path.join(out_dir, render_mod.render_file_name(plan.name, step)), render_mod.quantise(rgba))
                if log:
                    log(f"render {plan.name!r}: step {step}: {render_mod.summary(codes, samples)}")

        def take_tracers(step):
            """the advance of the host fallback behind coarse step `step`, and at a snapshot step the snapshot: files out, one log line
            per group"""
            levels = tracer_mod.stepper_levels(st, grids, step) if tr_host is not None else None
            if tr_host is not None:
                tr_host.advance(levels)
            if not stats_mod.is_sample_step(step, tr_start, cfg.tracers_output_interval):
                return
            rec, n_adv = (tr_host.snapshot(levels), tr_host.n_advances) if tr_host is not None else st.tracers_snapshot(step)
            if writing:
                tracer_writer.write(step, rec, n_adv)
            if log:
                for gi, name in enumerate(tr_plan.names):
                    log(f"tracers {name!r}: step {step}: {tracer_mod.summary(tr_plan, gi, rec, cfg.tracers_generations)}")

        def take_flux_host(step):
            """a sample of the host fallback's flux planes from downloaded fields, kept for flush_fluxes"""
            flux_host.append((step, *flux_mod.host_sample(st, fplans, step)))
        modes_live = [modes_on]              # False once a window has ended without `repeat`

        def modes_steps(t, batch_end):
            """a sample cuts nothing: only a window's last step does (the first one alone without `repeat`)"""
            if not modes_live[0]:
                return []
            ends = modes_mod.window_end_steps(t, batch_end, mplan.start_step, mplan.interval, mplan.samples)
            return ends if mplan.repeat else ends[:1]

        def take_modes(step):
            """the window that ends with coarse step `step`: sums down, files out, then the reset for the next window (collective in a
            distributed run)"""
            first = step - (mplan.samples - 1) * mplan.interval
            finals = {}
            for lvl in range(len(grids)):
                got = st.modes_sums(lvl)                                                                  # collective
                if got is None:
                    continue
                if got[1] != mplan.samples:
                    raise RuntimeError(f"fourier modes: level {lvl + 1} holds {got[1]} samples at step {step}, the window has "
                                       f"{mplan.samples}")
                finals[lvl] = modes_mod.finalize(np.stack(got[0]), mplan.W)
            if writing and finals:
                out_mod.export_modes_mesh(step, grids, finals.__getitem__, (first, step, mplan.samples, mplan.interval), mplan.frequencies_hz,
                                          out_dir)
                append_csv("flow_modes.csv", (modes_mod.csv_row(mplan, first, step, k, g.level_id,
                                                                *modes_mod.level_energy(finals[lvl][1][k], g.obstacle))
                                              for k in range(mplan.n_modes) for lvl, g in enumerate(grids)))
            if log:
                log(f"fourier modes: window of steps {first}..{step} ({mplan.samples} samples) written at step {step}")
            if mplan.repeat:
                st.modes_reset()
            else:
                modes_live[0] = False
                if st.modes is not None:
                    st.modes.close()
                    st.modes = None

        def state_steps(t, batch_end):
            """the multiples of the interval, and the last step"""
            every = cfg.state_files_interval
            steps = set(stats_mod.sample_steps(t, batch_end, every, every)) if every > 0 else set()
            return steps | {total_steps} if batch_end == total_steps else steps

        def take_state(step):
            """state_%06d.npz from downloaded fields"""
            warm_mod.save_state(os.path.join(out_dir, warm_mod.state_file_name(step)),
                                warm_mod.state_from_stepper(st, grids, step, params.mesh_offset, float(cfg.u_lattice),
                                                            os.path.basename(cfg.case_dir)))
            if log:
                log(f"state file {warm_mod.state_file_name(step)} written")

        # the cut schedule, in the order of action at a cut: (steps_in(t, batch_end) -> that output's cut steps of a batch, take(step)).
        # What a stepper samples inside its batches (device tracers' advances, device flux planes, the modes' samples) cuts nothing.
        cutters = [(steps_in, take) for on, steps_in, take in (
            (stats_on, _every(cfg.statistics_start_step, cfg.statistics_interval), take_statistics),
            (surf_host is not None, _every(surf_start, surf_interval), take_surface_host),
            (slices_on, _every(cfg.slices_start_step, cfg.slices_interval), take_slices),
            (iso_on, _every(cfg.isosurfaces_start_step, cfg.isosurfaces_interval), take_isosurfaces),
            (stream_on, _every(cfg.streamlines_start_step, cfg.streamlines_interval), take_streamlines),
            (render_on, _every(cfg.render_start_step, cfg.render_interval), take_render),
            # the host fallback cuts at every advance step, the device at the snapshot steps only
            (tracers_on, _every(tr_start, tr_interval if tr_host is not None else cfg.tracers_output_interval), take_tracers),
            (flux_on and not dev_fluxes, _every(cfg.flux_planes_start_step, cfg.flux_planes_interval), take_flux_host),
            (modes_on, modes_steps, take_modes),
            (state_on, state_steps, take_state)) if on]

        def run_batch(t, batch_end, u_curr):
            """coarse steps t..batch_end, cut after every step of the schedule - with the batch's own inlet speed: the same steps, the
            same bits - where the takes of that step act in the schedule's order"""
            takes = {}
            for steps_in, take in cutters:
                for step in steps_in(t, batch_end):
                    takes.setdefault(step, []).append(take)
            seg = t
            for step in sorted(takes):
                st.batch(seg, step - seg + 1, u_curr, sp)
                for take in takes[step]:
                    take(step)
                seg = step + 1
            if seg <= batch_end:
                st.batch(seg, batch_end - seg + 1, u_curr, sp)

        t0 = last_diag = _time.time()
        total_cells = sum(g.n_blocks * 512 for g in grids)
        rows: List[DiagRow] = []
        fr = None                            # the newest loads: the output step reuses those of a diagnostics step at the same step

        def diagnostics_step(t, batch_end, u_curr):
            """when a multiple of diag_freq lies in t..batch_end: a row, the probes' new samples, the monitor and the wall diagnostics from
            the state at batch end; after the last step the monitor and the wall diagnostics in any case. -> the monitor's FlowDiverged
            or None"""
            nonlocal fr, last_diag
            diag_step = (batch_end // cfg.diag_freq) * cfg.diag_freq
            at_diag = t <= diag_step <= batch_end
            if at_diag:
                rho1 = None
                if hasattr(st, "rho_min"):
                    rho_min = st.rho_min(0)
                else:
                    rho1 = st.field(0, "rho")
                    rho_min = flow_stats(rho1, grids[0].obstacle)
                cd = cl = cs = cmy = float("nan")
                if cfg.forces_enabled:
                    fr = _aerodynamics(st, grids, mesh, params, cfg.symmetric_analysis, rho1 if len(grids) == 1 else None)
                    cd, cl, cs, cmy = fr.Cd, fr.Cl, fr.Cs, fr.Cmy
                rows.append(DiagRow(diag_step, float(u_curr), rho_min, cd, cl, cs, cmy))
                now = _time.time()
                mlups = (total_cells * cfg.diag_freq) / (max(now - last_diag, 1e-9) * 1e6)     # src/main.jl:189
                last_diag = now
                if writing:
                    time_phys = float(diag_step) * params.time_scale
                    if cfg.forces_enabled:
                        out_mod.append_force_csv(os.path.join(out_dir, "forces.csv"), diag_step, time_phys, fr, u_curr)
                    append_csv("convergence.csv", [out_mod.convergence_csv_row(diag_step, now - t0, time_phys, u_curr, rho_min, mlups,
                                                                               cd if cfg.forces_enabled else None,
                                                                               cl if cfg.forces_enabled else None)])
                if log:
                    log(f"{diag_step:8d} | {float(u_curr):.4f} | {rho_min:.4f} | {cd:8.4f} | {cl:8.4f}")
                if probes_on:
                    flush_probes()
            elif batch_end != total_steps:
                return None
            step = diag_step if at_diag else batch_end       # the last step is no diagnostics step: a record of the end state
            diverged = take_monitor(step, batch_end) if monitor_on else None
            if wall_on:
                take_wall(step, batch_end)
            return diverged
        # derived flow arrays on output steps: (VTU name, index into gradient_fields' result, components)
        grad_names = [g for g in (("Vorticity", 0, 3), ("QCriterion", 1, 1)) if g[0] in cfg.output_fields]

        def output_step(t, batch_end):
            """when a multiple of output_freq lies in t..batch_end: the flow, surface and mean files of that step (src/main.jl:213-231)"""
            nonlocal fr
            out_step = (batch_end // cfg.output_freq) * cfg.output_freq
            if out_dir is None or not t <= out_step <= batch_end:
                return
            fetched = {}

            def fields(lvl, name):
                if name == "obstacle":
                    return grids[lvl].obstacle
                if (lvl, name) not in fetched:
                    fetched[(lvl, name)] = st.field(lvl, name)          # collective in a distributed run
                return fetched[(lvl, name)]

            levels = sorted({l for l, _ in out_mod.select_export_blocks([g.active_block_coords for g in grids])})
            vel_name = "vel_temp" if out_step % 2 == 0 else "vel"
            for lvl in levels:
                fields(lvl, "rho"); fields(lvl, vel_name)
            derived = None
            if grad_names:
                # the buffer the file's Velocity comes from, derivatives per unit length of the file's coordinates
                grad = {lvl: st.gradient_fields(lvl, vel_name, np.float32(1.0 / grids[lvl].dx)) for lvl in levels}      # collective
                derived = [(name, (lambda lvl, k=k: grad[lvl][k]), ncomp) for name, k, ncomp in grad_names]
            if eddy_on:
                # nu_t of the buffer the file's Velocity comes from over the level's nu, both Float32
                eddy = {}
                for lvl in levels:
                    got = st.subgrid_fields(lvl, vel_name)                                               # collective
                    eddy[lvl] = subgrid_mod.ratio_field(got[0], grids[lvl].tau) if got is not None else None
                derived = (derived or []) + [("EddyViscosityRatio", eddy.__getitem__, 1)]
            if cfg.forces_enabled and (fr is None or fr.maps is None or out_step != (out_step // cfg.diag_freq) * cfg.diag_freq):
                fr = _aerodynamics(st, grids, mesh, params, cfg.symmetric_analysis, want_maps=True)
            wall_vals = wall_values(batch_end) if wall_on and cfg.forces_enabled else None          # collective
            if writing:
                out_mod.export_merged_mesh(out_step, grids, fields, out_dir, cfg.output_fields, derived=derived)
                if cfg.forces_enabled:
                    extra = list(wall_mod.finalize(wall_vals, params).items()) if wall_vals is not None else None
                    out_mod.save_surface_vtk(os.path.join(out_dir, "surface_%06d" % out_step), mesh, *fr.maps, extra=extra)
            if stats_on and stats_window[0] > 0:
                finals = {lvl: st.statistics(lvl) for lvl in levels}                                     # collective
                sgs, sgs_extra = {}, None
                if subgrid_on:
                    for lvl in sorted(finals):
                        sums = st.subgrid_stats_sums(lvl)                                                # collective
                        if sums is not None:
                            sgs[lvl] = subgrid_mod.finalize(*sums, subgrid_mod.level_viscosity(grids[lvl].tau),
                                                            cfg.statistics_subgrid_ck, finals[lvl]["tke"])
                    sgs_extra = [(name, (lambda lvl, k=k: sgs[lvl][k])) for name, k in subgrid_mod.MEAN_ARRAYS]
                if writing:
                    out_mod.export_mean_mesh(out_step, grids, finals.__getitem__, tuple(stats_window), out_dir, extra=sgs_extra)
            if surf_on:
                got = surf_host.download() if surf_host is not None else st.surface_stats_sums()        # collective
                if writing and got is not None and got[1] > 0:
                    window = surface_mod.window_of(got[1], surf_start, surf_interval)
                    fin_stats = surface_mod.finalize(got[0], got[1], params)
                    surface_mod.save_surface_mean_vtk(os.path.join(out_dir, "surface_mean_%06d" % out_step), mesh, fin_stats, splan.found,
                                                      window)
                    fr_mean = surface_mod.mean_forces(mesh, fin_stats, params, cfg.symmetric_analysis)
                    append_csv("forces_mean.csv", [surface_mod.forces_mean_csv_row(out_step, window, fr_mean)])

        # ---- the time loop ----
        t = first_step
        while t <= total_steps:
            batch_end = min(t + batch - 1, total_steps)
            u_curr = ramp_velocity(batch_end, cfg.ramp_steps, cfg.u_lattice)
            run_batch(t, batch_end, u_curr)
            if fseries_on:
                flush_force_series(u_curr)
            if flux_on:
                flush_fluxes()
            diverged = diagnostics_step(t, batch_end, u_curr)
            output_step(t, batch_end)
            if diverged is not None and cfg.flow_monitor_stop_on_divergence:
                if probes_on:
                    flush_probes()
                raise diverged
            t = batch_end + 1
        if probes_on:
            flush_probes()
        if modes_live[0] and log:
            done = modes_mod.window_end_steps(1, total_steps, mplan.start_step, mplan.interval, mplan.samples)
            began = (done[-1] + mplan.interval) if done else mplan.start_step
            if began <= total_steps:
                log(f"fourier modes: the window that began at step {began} is unfinished at step {total_steps}: nothing written for it")
        if fseries_on and log:
            for name, k in (("Cd", 0), ("Cl", 1), ("Cmy", 2)):
                m, r = fseries_mod.mean_rms(c[k] for c in fseries_coeffs)
                log(f"force series {name}: mean {m:.6f} rms {r:.6f} over {len(fseries_coeffs)} rows after step {cfg.ramp_steps}")
        if fseries_on and flux_on and log:
            surface_cd, _ = fseries_mod.mean_rms(c[0] for c in fseries_coeffs)
            for name, cds in flux_box_cd.items():
                m, _ = fseries_mod.mean_rms(cds)
                log(f"flux box {name!r}: mean control-volume Cd {m:.6f} over {len(cds)} rows after step {cfg.ramp_steps} "
                    f"(surface Cd {surface_cd:.6f})")
    finally:
        if hasattr(st, "close"):
            st.close()
    return rows, report, params
