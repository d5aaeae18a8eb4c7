"""Host pre-processing (scope row N1): YAML + STL -> BlockLevels, restating the reference's one-time setup.

  config keys        src/config_loader.jl:109-197 (Appendix C of SURVEY.md)
  scaling            src/physics_scaling.jl:59-176
  STL                src/geometry.jl:86-209
  block sets         src/domain.jl:56-247, src/domain_topology.jl:9-133
  voxelizer / fill   src/domain_generation.jl:10-203
  sponge             src/domain_generation.jl:205-289
  wall distance      src/domain_generation.jl:371-434
  Bouzidi q-map      src/bouzidi_setup.jl:64-167, src/bouzidi_math.jl:9-102

All of it is Float64 host arithmetic that runs once per case; it is numpy here. Where the reference loops over cells and
triangles, the loops are vectorised with conservative pre-filters that cannot change a result (noted in place).
Anchors: the setup integers printed in the reference's run logs (tests/golden/sphere_re266k_setup.json).
"""
from __future__ import annotations

import math
import os
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np
import yaml

from .blocks import BLOCK_SIZE, BlockLevel, build_neighbor_table
from .physics import SolverParams

BS = BLOCK_SIZE


# ----------------------------------------------------------------------------------------------------------------
# configuration, src/config_loader.jl:109-197
# ----------------------------------------------------------------------------------------------------------------
def _get(d, *keys, default=None, required=False):
    cur = d
    for k in keys:
        if not isinstance(cur, dict) or k not in cur:
            if required:
                raise KeyError("Missing config key: " + " -> ".join(keys))
            return default
        cur = cur[k]
    return default if (cur is None and default is not None) else cur


@dataclass
class CaseConfig:
    stl_file: str
    stl_scale: float
    surface_resolution: int
    num_levels: int
    output_dir: str
    steps: int
    ramp_steps: int
    output_freq: int
    symmetric_analysis: bool = False
    reference_area_full_model: float = 0.0
    reference_chord: float = 0.0
    reference_length_for_meshing: float = 0.0
    reference_dimension: str = "x"
    fluid_density: float = 1.225
    fluid_kinematic_viscosity: float = 1.5e-5
    flow_velocity: float = 10.0
    u_lattice: np.float32 = np.float32(0.01)
    c_wale: np.float32 = np.float32(0.20)
    tau_min: np.float32 = np.float32(0.505)
    inlet_turbulence_intensity: np.float32 = np.float32(0.01)
    nu_sgs_background: np.float32 = np.float32(0.0005)
    sponge_blend_distributions: bool = True
    temporal_interpolation: bool = True
    auto_levels: bool = False
    max_levels: int = 12
    min_coarse_blocks: int = 4
    wall_model_enabled: bool = False
    domain_upstream: float = 0.75
    domain_downstream: float = 1.5
    domain_lateral: float = 0.75
    domain_height: float = 0.75
    sponge_thickness: np.float32 = np.float32(0.10)
    block_size_config: int = 8
    refinement_margin: int = 2
    refinement_strategy: str = "geometry_first"
    wake_enabled: bool = False
    wake_length: float = 0.25
    wake_width_factor: float = 0.1
    wake_height_factor: float = 0.1
    boundary_method: str = "bouzidi"
    bouzidi_levels: int = 1
    q_min_threshold: np.float32 = np.float32(0.001)
    forces_enabled: bool = True
    moment_center: Tuple[float, float, float] = (0.25, 0.0, 0.0)
    # force series, advanced.forces.series (no reference counterpart): the integrated loads of the finest level reduced on the device
    # at every `interval`-th coarse step from `start_step`, written to forces_series.csv (force_series.py)
    forces_series_enabled: bool = False
    forces_series_start_step: int = 1
    forces_series_interval: int = 1
    diag_freq: int = 500
    async_depth: int = 8
    case_dir: str = ""
    output_fields: Tuple[str, ...] = ("Density", "Velocity", "VelocityMagnitude", "Obstacle", "Level")   # io_vtk.jl:116-120
    # time-averaged statistics, advanced.statistics (no reference counterpart; its loader ignores the keys): flow_mean_%06d.vtu
    statistics_enabled: bool = False
    statistics_start_step: int = 1      # first sampled coarse step (the sums are reset there); YAML default: ramp_steps
    statistics_interval: int = 10       # coarse steps between samples
    # advanced.statistics.subgrid (subgrid.py): the subgrid model's sums at the flow statistics' sampled steps, five more arrays in
    # flow_mean_%06d.vtu; subgrid_ck: the constant of k_sgs = (nu_t / (c_k Delta))^2
    statistics_subgrid: bool = False
    statistics_subgrid_ck: float = 0.094
    # surface statistics, advanced.surface_statistics (no reference counterpart): per-triangle mean / rms wall loads of the finest level,
    # written to surface_mean_%06d.vtu and forces_mean.csv on output steps (surface_stats.py)
    surface_statistics_enabled: bool = False
    surface_statistics_start_step: int = 1      # first sampled coarse step; YAML default: ramp_steps
    surface_statistics_interval: int = 1        # coarse steps between samples
    # probes, advanced.probes (no reference counterpart): rho, u at points every `interval` coarse steps from `start_step`, written to
    # probes.csv / probes_points.csv; points in the STL's frame after stl_scale (probes.py)
    probes_enabled: bool = False
    probes_start_step: int = 1
    probes_interval: int = 1
    probes_points: Tuple[Tuple[float, float, float], ...] = ()
    probes_names: Tuple[str, ...] = ()
    # slices, advanced.slices (no reference counterpart): planar grids of points sampled every `interval` coarse steps from
    # `start_step`, written to slice_<name>_%06d.vti and slice_<name>.pvd (slices.py)
    slices_enabled: bool = False
    slices_start_step: int = 1
    slices_interval: int = 1
    slices_planes: Tuple["SlicePlane", ...] = ()
    # iso-surfaces, advanced.isosurfaces (no reference counterpart): surfaces extracted on the device every `interval` coarse steps
    # from `start_step`, written to iso_<name>_%06d.vtp and iso_<name>.pvd (isosurface.py)
    isosurfaces_enabled: bool = False
    isosurfaces_start_step: int = 1
    isosurfaces_interval: int = 1
    isosurfaces_max_triangles: int = 50_000_000
    isosurfaces_surfaces: Tuple["IsoSurfaceSpec", ...] = ()
    # streamlines, advanced.streamlines (no reference counterpart): lines traced on the device through every level every `interval` coarse
    # steps from `start_step`, written to stream_<name>_%06d.vtp and stream_<name>.pvd (streamlines.py)
    streamlines_enabled: bool = False
    streamlines_start_step: int = 1
    streamlines_interval: int = 100
    streamlines_step: float = 0.5
    streamlines_max_steps: int = 2000
    streamlines_min_speed: float = 1.0e-6
    streamlines_direction: str = "both"
    streamlines_max_vertices: int = 20_000_000
    streamlines_seeds: Tuple["StreamlineSeeds", ...] = ()
    # volume images, advanced.render (no reference counterpart): every view ray-marched on the device through every level every
    # `interval` coarse steps from `start_step`, written to render_<name>_%06d.png (render.py)
    render_enabled: bool = False
    render_start_step: int = 1
    render_interval: int = 100
    render_width: int = 1280
    render_height: int = 720
    render_max_pixels: int = 8_294_400
    render_views: Tuple["RenderView", ...] = ()
    # tracers, advanced.tracers (no reference counterpart): particles advected on the device inside every batch, one advance every
    # `interval` coarse steps from `start_step`, one release per seed every `release_every` advances into a ring of `generations`; every
    # `output_interval` coarse steps a snapshot goes to tracers_<name>_%06d.vtp and tracers_<name>.pvd (tracers.py)
    tracers_enabled: bool = False
    tracers_start_step: int = 1
    tracers_interval: int = 1
    tracers_release_every: int = 10
    tracers_generations: int = 64
    tracers_output_interval: int = 100
    tracers_max_particles: int = 4_000_000
    tracers_seeds: Tuple["StreamlineSeeds", ...] = ()
    # flux planes, advanced.flux_planes (no reference counterpart): mass, momentum, pressure and kinetic-energy flux through planes and
    # boxes, reduced on the device inside every batch at the coarse steps start_step + k interval and written to fluxes.csv and
    # flux_boxes.csv (flux_planes.py); flux_planes_planes holds the planes and then every box's six faces
    flux_planes_enabled: bool = False
    flux_planes_start_step: int = 1
    flux_planes_interval: int = 1
    flux_planes_planes: Tuple["FluxPlane", ...] = ()
    flux_planes_boxes: Tuple["FluxBox", ...] = ()
    # Fourier modes, advanced.fourier_modes (no reference counterpart): per cell the windowed DFT of rho and u at a few frequencies,
    # accumulated on the device inside every batch at the coarse steps start_step + k interval; every `samples` samples a window ends and
    # flow_modes_%06d.vtu and flow_modes.csv rows are written (modes.py). frequencies in Hz, strouhal as f L / U of the case
    fourier_modes_enabled: bool = False
    fourier_modes_start_step: int = 1
    fourier_modes_interval: int = 1
    fourier_modes_samples: int = 256
    fourier_modes_window: str = "hann"
    fourier_modes_frequencies: Tuple[float, ...] = ()
    fourier_modes_strouhal: Tuple[float, ...] = ()
    fourier_modes_repeat: bool = True
    # flow monitor, advanced.flow_monitor (no reference counterpart; its advanced.diagnostics.stability_check is read by nobody, there or
    # here): a health record of every level at every diagnostics step, written to flow_monitor.csv (monitor.py)
    flow_monitor_enabled: bool = False
    flow_monitor_stop_on_divergence: bool = False       # end the run with monitor.FlowDiverged once a level holds non-finite fluid cells
    # wall diagnostics, advanced.wall_diagnostics (no reference counterpart; the reference reads y_plus_target and uses it nowhere): the y+,
    # friction velocity and modelled wall shear of the wall model at every diagnostics step, written to wall_model.csv, wall_forces.csv
    # and the surface file (wall_diagnostics.py)
    wall_diagnostics_enabled: bool = False
    wall_diagnostics_band: Tuple[float, float] = (30.0, 300.0)      # the y+ range ShareInBand counts, 0 < lo < hi
    y_plus_target: float = 100.0                        # advanced.high_re.wall_model.y_plus_target, echoed in wall_model.csv
    # warm start (no reference counterpart; warm_start.py). advanced.state_files: state_%06d.npz - rho and the newest velocity of every
    # level - after the coarse steps that are multiples of `interval` and after the last step (interval 0: the last step only).
    # advanced.initial_condition: every level is filled from such a file after set-up, the populations at their equilibrium, and the
    # step loop starts at first_step; velocity_scale None = auto: this case's u_lattice over the state's
    state_files_enabled: bool = False
    state_files_interval: int = 0
    initial_condition_state: str = ""                   # path, relative to the case folder; empty: start from rest
    initial_condition_first_step: int = 1
    initial_condition_velocity_scale: Optional[float] = None

    @property
    def reference_area_config(self) -> float:
        return self.reference_area_full_model / 2.0 if self.symmetric_analysis else self.reference_area_full_model


def load_case_configuration(config_path: str, overrides: Optional[dict] = None) -> CaseConfig:
    """load_case_configuration (src/config_loader.jl:109-197). `overrides` patches the parsed YAML tree, e.g.
    {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}}} (how the Re 266k log was produced)."""
    with open(config_path) as fh:
        cfg = yaml.safe_load(fh)

    def merge(dst, src):
        for k, v in src.items():
            if isinstance(v, dict) and isinstance(dst.get(k), dict):
                merge(dst[k], v)
            else:
                dst[k] = v
    if overrides:
        merge(cfg, overrides)
    f32 = np.float32
    g = lambda *k, **kw: _get(cfg, *k, **kw)
    ramp_steps = int(g("basic", "simulation", "ramp_steps", required=True))
    # averaging the ramp means nothing: sampling starts at ramp_steps unless told otherwise (at step 1 at the earliest)
    stats_start = int(g("advanced", "statistics", "start_step", default=ramp_steps))
    stats_interval = int(g("advanced", "statistics", "interval", default=10))
    if stats_interval < 1:
        raise ValueError(f"advanced.statistics.interval must be >= 1, got {stats_interval}")
    stats_subgrid = bool(g("advanced", "statistics", "subgrid", default=False))
    stats_subgrid_ck = float(g("advanced", "statistics", "subgrid_ck", default=0.094))
    if stats_subgrid and not bool(g("advanced", "statistics", "enabled", default=False)):
        raise ValueError("advanced.statistics.subgrid is true, but advanced.statistics.enabled is not: the subgrid measures are "
                         "sampled with the flow statistics")
    if stats_subgrid and not stats_subgrid_ck > 0.0:
        raise ValueError(f"advanced.statistics.subgrid_ck must be > 0, got {stats_subgrid_ck}")
    surf_start = int(g("advanced", "surface_statistics", "start_step", default=ramp_steps))
    surf_interval = int(g("advanced", "surface_statistics", "interval", default=1))
    if surf_interval < 1:
        raise ValueError(f"advanced.surface_statistics.interval must be >= 1, got {surf_interval}")
    forces_series = _forces_series_config(g("advanced", "forces", "series", default=None),
                                          bool(g("advanced", "forces", "enabled", default=True)))
    probes = _probes_config(g("advanced", "probes", default=None))
    slices = _slices_config(g("advanced", "slices", default=None))
    isosurfaces = _isosurfaces_config(g("advanced", "isosurfaces", default=None))
    streamlines = _streamlines_config(g("advanced", "streamlines", default=None))
    render = _render_config(g("advanced", "render", default=None))
    tracers = _tracers_config(g("advanced", "tracers", default=None), int(g("basic", "simulation", "steps", required=True)))
    flux_planes = _flux_planes_config(g("advanced", "flux_planes", default=None))
    fourier_modes = _fourier_modes_config(g("advanced", "fourier_modes", default=None))
    flow_monitor = _flow_monitor_config(g("advanced", "flow_monitor", default=None))
    wall_diag = _wall_diagnostics_config(g("advanced", "wall_diagnostics", default=None))
    warm = _warm_start_config(g("advanced", "state_files", default=None), g("advanced", "initial_condition", default=None))
    return CaseConfig(
        stl_file=g("basic", "stl_file", required=True), stl_scale=float(g("basic", "stl_scale", required=True)),
        surface_resolution=int(g("basic", "surface_resolution", required=True)), num_levels=int(g("basic", "num_levels", required=True)),
        output_dir=g("basic", "simulation", "output_dir", required=True), steps=int(g("basic", "simulation", "steps", required=True)),
        ramp_steps=int(g("basic", "simulation", "ramp_steps", required=True)), output_freq=int(g("basic", "simulation", "output_freq", required=True)),
        symmetric_analysis=bool(g("advanced", "refinement", "symmetric_analysis", default=False)),
        reference_area_full_model=float(g("basic", "reference_area_of_full_model", default=0.0)),
        reference_chord=float(g("basic", "reference_chord", default=0.0)),
        reference_length_for_meshing=float(g("basic", "reference_length_for_meshing", default=0.0)),
        reference_dimension=str(g("basic", "reference_dimension", default="x")),
        fluid_density=float(g("basic", "fluid", "density", default=1.225)),
        fluid_kinematic_viscosity=float(g("basic", "fluid", "kinematic_viscosity", default=1.5e-5)),
        flow_velocity=float(g("basic", "flow", "velocity", default=10.0)),
        u_lattice=f32(g("advanced", "numerics", "u_lattice", default=0.01)), c_wale=f32(g("advanced", "numerics", "c_wale", default=0.20)),
        tau_min=f32(g("advanced", "numerics", "tau_min", default=0.505)),
        inlet_turbulence_intensity=f32(g("advanced", "numerics", "inlet_turbulence_intensity", default=0.01)),
        nu_sgs_background=f32(g("advanced", "numerics", "nu_sgs_background", default=0.0005)),
        sponge_blend_distributions=bool(g("advanced", "numerics", "sponge_blend_distributions", default=True)),
        temporal_interpolation=bool(g("advanced", "numerics", "temporal_interpolation", default=True)),
        auto_levels=bool(g("advanced", "high_re", "auto_levels", default=False)), max_levels=int(g("advanced", "high_re", "max_levels", default=12)),
        min_coarse_blocks=int(g("advanced", "high_re", "min_coarse_blocks", default=4)),
        wall_model_enabled=bool(g("advanced", "high_re", "wall_model", "enabled", default=False)),
        domain_upstream=float(g("advanced", "domain", "upstream", default=0.75)), domain_downstream=float(g("advanced", "domain", "downstream", default=1.5)),
        domain_lateral=float(g("advanced", "domain", "lateral", default=0.75)), domain_height=float(g("advanced", "domain", "height", default=0.75)),
        sponge_thickness=f32(g("advanced", "domain", "sponge_thickness", default=0.10)),
        block_size_config=int(g("advanced", "refinement", "block_size", default=8)), refinement_margin=int(g("advanced", "refinement", "margin", default=2)),
        refinement_strategy=str(g("advanced", "refinement", "strategy", default="geometry_first")),
        wake_enabled=bool(g("advanced", "refinement", "wake_enabled", default=False)), wake_length=float(g("advanced", "refinement", "wake_length", default=0.25)),
        wake_width_factor=float(g("advanced", "refinement", "wake_width_factor", default=0.1)),
        wake_height_factor=float(g("advanced", "refinement", "wake_height_factor", default=0.1)),
        boundary_method=str(g("advanced", "boundary", "method", default="bouzidi")), bouzidi_levels=int(g("advanced", "boundary", "bouzidi_levels", default=1)),
        q_min_threshold=f32(g("advanced", "boundary", "q_min_threshold", default=0.001)),
        forces_enabled=bool(g("advanced", "forces", "enabled", default=True)),
        moment_center=tuple(float(v) for v in g("advanced", "forces", "moment_center", default=[0.25, 0.0, 0.0])),
        diag_freq=int(g("advanced", "diagnostics", "freq", default=500)), async_depth=int(g("advanced", "gpu", "async_depth", default=8)),
        case_dir=os.path.dirname(os.path.abspath(config_path)),
        # bouzidi is read by the reference's loader (config_loader.jl:148) but never written by io_vtk.jl. vorticity (the reference's
        # loader defaults it to true, config_loader.jl:145, and never writes it) and q_criterion (not a reference key) add device-computed
        # arrays to the flow file; both default to FALSE here, because the reference writes neither and every shipped config says false.
        # eddy_viscosity (not a reference key, default false) adds EddyViscosityRatio, nu_t / nu of the step's own WALE model (subgrid.py).
        output_fields=tuple(name for key, name in (("density", "Density"), ("velocity", "Velocity"), ("velocity_magnitude", "VelocityMagnitude"),
                                                   ("obstacle", "Obstacle"), ("level", "Level"))
                            if bool(g("basic", "simulation", "output_fields", key, default=True)))
                      + tuple(name for key, name in (("vorticity", "Vorticity"), ("q_criterion", "QCriterion"),
                                                     ("eddy_viscosity", "EddyViscosityRatio"))
                              if bool(g("basic", "simulation", "output_fields", key, default=False))),
        statistics_enabled=bool(g("advanced", "statistics", "enabled", default=False)),
        statistics_start_step=max(stats_start, 1), statistics_interval=stats_interval,
        statistics_subgrid=stats_subgrid, statistics_subgrid_ck=stats_subgrid_ck,
        surface_statistics_enabled=bool(g("advanced", "surface_statistics", "enabled", default=False)),
        surface_statistics_start_step=max(surf_start, 1), surface_statistics_interval=surf_interval,
        **forces_series,
        **probes,
        **slices,
        **isosurfaces,
        **streamlines,
        **render,
        **tracers,
        **flux_planes,
        **fourier_modes,
        **flow_monitor,
        **wall_diag,
        **warm,
        y_plus_target=float(g("advanced", "high_re", "wall_model", "y_plus_target", default=100.0)),
    )


def _forces_series_config(fc, forces_enabled: bool) -> dict:
    """advanced.forces.series: {enabled: false, start_step: 1, interval: 1} -> CaseConfig fields. Absent or disabled: the defaults
    (nothing is allocated, launched or written)."""
    if fc is None:
        return {}
    if not isinstance(fc, dict):
        raise ValueError("advanced.forces.series must be a mapping")
    if not bool(fc.get("enabled", False)):
        return {}
    if not forces_enabled:
        raise ValueError("advanced.forces.series.enabled is true, but advanced.forces.enabled is not: the series is the force "
                         "integration, sampled every step")
    start, interval = int(fc.get("start_step", 1)), int(fc.get("interval", 1))
    if interval < 1:
        raise ValueError(f"advanced.forces.series.interval must be >= 1, got {interval}")
    return {"forces_series_enabled": True, "forces_series_start_step": max(start, 1), "forces_series_interval": interval}


def _probes_config(pc) -> dict:
    """advanced.probes: {enabled: false, start_step: 1, interval: 1, points: [[x, y, z], ...], names: [...]} -> CaseConfig fields.
    Absent or disabled: the defaults (nothing is planned, allocated or written)."""
    if pc is None:
        return {}
    if not isinstance(pc, dict):
        raise ValueError("advanced.probes must be a mapping")
    if not bool(pc.get("enabled", False)):
        return {}
    start, interval = int(pc.get("start_step", 1)), int(pc.get("interval", 1))
    if interval < 1:
        raise ValueError(f"advanced.probes.interval must be >= 1, got {interval}")
    if start < 1:
        raise ValueError(f"advanced.probes.start_step must be >= 1, got {start}")
    raw = pc.get("points") or []
    pts = []
    for i, p in enumerate(raw):
        if not isinstance(p, (list, tuple)) or len(p) != 3:
            raise ValueError(f"advanced.probes.points[{i}] must be [x, y, z], got {p!r}")
        v = tuple(float(c) for c in p)
        if not all(math.isfinite(c) for c in v):
            raise ValueError(f"advanced.probes.points[{i}] is not finite: {p!r}")
        pts.append(v)
    if not pts:
        raise ValueError("advanced.probes.enabled needs at least one point")
    names = pc.get("names")
    names = [f"p{i}" for i in range(len(pts))] if names is None else [str(n) for n in names]
    if len(names) != len(pts):
        raise ValueError(f"advanced.probes: {len(names)} names for {len(pts)} points")
    for n in names:
        if not n or any(ch in n for ch in ',"\'\n\r') or n != n.strip():
            raise ValueError(f"advanced.probes.names: {n!r} is not a plain CSV column name")
    if len(set(names)) != len(names):
        raise ValueError("advanced.probes.names must be unique")
    return dict(probes_enabled=True, probes_start_step=start, probes_interval=interval, probes_points=tuple(pts),
                probes_names=tuple(names))


def _warm_start_config(sc, ic) -> dict:
    """advanced.state_files: {enabled: false, interval: 0} and advanced.initial_condition: {state: <path>, first_step: 1, velocity_scale:
    auto} -> CaseConfig fields. Absent (or state_files disabled): the defaults - nothing is allocated, launched or written."""
    out = {}
    if sc is not None:
        if not isinstance(sc, dict):
            raise ValueError("advanced.state_files must be a mapping")
        if bool(sc.get("enabled", False)):
            interval = int(sc.get("interval", 0))
            if interval < 0:
                raise ValueError(f"advanced.state_files.interval must be >= 0, got {interval}")
            out.update(state_files_enabled=True, state_files_interval=interval)
    if ic is not None:
        if not isinstance(ic, dict):
            raise ValueError("advanced.initial_condition must be a mapping")
        state = ic.get("state")
        if not isinstance(state, str) or not state:
            raise ValueError("advanced.initial_condition.state must be the path of a state file")
        first = int(ic.get("first_step", 1))
        if first < 1:
            raise ValueError(f"advanced.initial_condition.first_step must be >= 1, got {first}")
        scale = ic.get("velocity_scale", "auto")
        if scale == "auto" or scale is None:
            scale = None
        else:
            try:
                scale = float(scale)
            except (TypeError, ValueError):
                raise ValueError(f"advanced.initial_condition.velocity_scale must be a number or auto, got {scale!r}") from None
            if not (math.isfinite(scale) and scale > 0.0):
                raise ValueError(f"advanced.initial_condition.velocity_scale must be positive and finite, got {scale}")
        out.update(initial_condition_state=state, initial_condition_first_step=first, initial_condition_velocity_scale=scale)
    return out


def _flow_monitor_config(mc) -> dict:
    """advanced.flow_monitor: {enabled: false, stop_on_divergence: false} -> CaseConfig fields. Absent: the defaults."""
    if mc is None:
        return {}
    if not isinstance(mc, dict):
        raise ValueError("advanced.flow_monitor must be a mapping")
    vals = {}
    for key in ("enabled", "stop_on_divergence"):
        v = mc.get(key, False)
        if not isinstance(v, bool):
            raise ValueError(f"advanced.flow_monitor.{key} must be true or false, got {v!r}")
        vals[key] = v
    return dict(flow_monitor_enabled=vals["enabled"], flow_monitor_stop_on_divergence=vals["stop_on_divergence"])


def _wall_diagnostics_config(wc) -> dict:
    """advanced.wall_diagnostics: {enabled: false, band: [30.0, 300.0]} -> CaseConfig fields. Absent: the defaults."""
    from .wall_diagnostics import check_band
    if wc is None:
        return {}
    if not isinstance(wc, dict):
        raise ValueError("advanced.wall_diagnostics must be a mapping")
    enabled = wc.get("enabled", False)
    if not isinstance(enabled, bool):
        raise ValueError(f"advanced.wall_diagnostics.enabled must be true or false, got {enabled!r}")
    return dict(wall_diagnostics_enabled=enabled, wall_diagnostics_band=check_band(wc.get("band", (30.0, 300.0))))


SLICE_FIELDS = ("density", "velocity", "velocity_magnitude", "vorticity", "q_criterion")   # basic.simulation.output_fields keys
SLICE_MAX_POINTS = 1 << 24                                  # per plane


@dataclass(frozen=True)
class SlicePlane:
    """one plane of advanced.slices.planes (semantics: slices.py)"""
    name: str
    normal: int                                             # axis: 0 = x, 1 = y, 2 = z
    position: float                                         # STL frame after stl_scale
    bounds: Optional[Tuple[Tuple[float, float], Tuple[float, float]]] = None   # the two in-plane axes in x, y, z order; None: the domain
    spacing: Optional[float] = None                         # None: dx of the finest level
    fields: Tuple[str, ...] = ("density", "velocity", "velocity_magnitude")


def slice_axis_points(lo: float, hi: float, h: float) -> int:
    """points along one in-plane axis: floor((hi - lo) / h) + 1"""
    return int(math.floor((hi - lo) / h)) + 1


def _slices_config(sc) -> dict:
    """advanced.slices: {enabled: false, start_step: 1, interval: 1, planes: [{name, normal, position, bounds?, spacing?, fields?}]}
    -> CaseConfig fields. Absent or disabled: the defaults. What needs the domain (a plane outside it, the default bounds' point count)
    is checked when the plane is planned (slices.plane_grid)."""
    if sc is None:
        return {}
    if not isinstance(sc, dict):
        raise ValueError("advanced.slices must be a mapping")
    if not bool(sc.get("enabled", False)):
        return {}
    start, interval = int(sc.get("start_step", 1)), int(sc.get("interval", 1))
    if interval < 1:
        raise ValueError(f"advanced.slices.interval must be >= 1, got {interval}")
    if start < 1:
        raise ValueError(f"advanced.slices.start_step must be >= 1, got {start}")
    raw = sc.get("planes") or []
    if not isinstance(raw, (list, tuple)) or not raw:
        raise ValueError("advanced.slices.enabled needs at least one plane")
    planes, seen = [], set()
    for i, pc in enumerate(raw):
        where = f"advanced.slices.planes[{i}]"
        if not isinstance(pc, dict):
            raise ValueError(f"{where} must be a mapping")
        name = str(pc.get("name", ""))
        if not name or not all(ch.isalnum() or ch in "_-." for ch in name) or name.startswith("."):
            raise ValueError(f"{where}.name {name!r} is not a plain file-name stem")
        if name in seen:
            raise ValueError(f"{where}.name {name!r} is not unique")
        seen.add(name)
        where = f"advanced.slices plane {name!r}"
        normal = str(pc.get("normal", "")).lower()
        if normal not in ("x", "y", "z"):
            raise ValueError(f"{where}: normal {pc.get('normal')!r} is not x, y or z")
        if "position" not in pc:
            raise ValueError(f"{where}: position is required")
        position = float(pc["position"])
        if not math.isfinite(position):
            raise ValueError(f"{where}: position {position} is not finite")
        bounds = pc.get("bounds")
        if bounds is not None:
            ok = isinstance(bounds, (list, tuple)) and len(bounds) == 2 and all(isinstance(b, (list, tuple)) and len(b) == 2 for b in bounds)
            if not ok:
                raise ValueError(f"{where}: bounds must be [[a0, a1], [b0, b1]], got {bounds!r}")
            bounds = tuple((float(b[0]), float(b[1])) for b in bounds)
            for lo, hi in bounds:
                if not (math.isfinite(lo) and math.isfinite(hi)) or not lo < hi:
                    raise ValueError(f"{where}: bounds {list(map(list, bounds))} must be finite with lower < upper")
        spacing = pc.get("spacing")
        if spacing is not None:
            spacing = float(spacing)
            if not (math.isfinite(spacing) and spacing > 0):
                raise ValueError(f"{where}: spacing {spacing} must be > 0")
        fields = pc.get("fields")
        fields = ("density", "velocity", "velocity_magnitude") if fields is None else tuple(str(f) for f in fields)
        for f in fields:
            if f not in SLICE_FIELDS:
                raise ValueError(f"{where}: unknown field {f!r} (one of {', '.join(SLICE_FIELDS)})")
        if not fields or len(set(fields)) != len(fields):
            raise ValueError(f"{where}: fields must be a non-empty list without repeats")
        if bounds is not None and spacing is not None:
            n = slice_axis_points(*bounds[0], spacing) * slice_axis_points(*bounds[1], spacing)
            if n > SLICE_MAX_POINTS:
                raise ValueError(f"{where}: {n} points, more than {SLICE_MAX_POINTS} per plane")
        planes.append(SlicePlane(name, "xyz".index(normal), position, bounds, spacing, tuple(f for f in SLICE_FIELDS if f in fields)))
    return dict(slices_enabled=True, slices_start_step=start, slices_interval=interval, slices_planes=tuple(planes))


@dataclass(frozen=True)
class FluxPlane:
    """one plane of advanced.flux_planes.planes, or one face of a box (semantics: flux_planes.py)"""
    name: str
    normal: int                                             # axis: 0 = x, 1 = y, 2 = z
    position: float                                         # STL frame after stl_scale
    bounds: Optional[Tuple[Tuple[float, float], Tuple[float, float]]] = None   # the two in-plane axes in x, y, z order; None: the domain
    spacing: Optional[float] = None                         # None: dx of the finest level
    direction: int = 1                                      # +1: flux along the +axis counts positive; -1: along the -axis
    box: Optional[str] = None                               # the box this plane is a face of


@dataclass(frozen=True)
class FluxBox:
    """one box of advanced.flux_planes.boxes: its faces are the FluxPlanes <name>_xmin .. <name>_zmax with outward directions"""
    name: str
    bounds: Tuple[Tuple[float, float], Tuple[float, float], Tuple[float, float]]
    spacing: Optional[float] = None


def _file_stem(where: str, name: str, seen: set) -> None:
    if not name or not all(ch.isalnum() or ch in "_-." for ch in name) or name.startswith("."):
        raise ValueError(f"{where}.name {name!r} is not a plain file-name stem")
    if name in seen:
        raise ValueError(f"{where}.name {name!r} is not unique")
    seen.add(name)


def _flux_spacing(where: str, spacing) -> Optional[float]:
    if spacing is None:
        return None
    spacing = float(spacing)
    if not (math.isfinite(spacing) and spacing > 0):
        raise ValueError(f"{where}: spacing {spacing} must be > 0")
    return spacing


def _flux_bounds(where: str, bounds, n: int, shape: str):
    ok = isinstance(bounds, (list, tuple)) and len(bounds) == n and all(isinstance(b, (list, tuple)) and len(b) == 2 for b in bounds)
    if not ok:
        raise ValueError(f"{where}: bounds must be {shape}, got {bounds!r}")
    bounds = tuple((float(b[0]), float(b[1])) for b in bounds)
    for lo, hi in bounds:
        if not (math.isfinite(lo) and math.isfinite(hi)) or not lo < hi:
            raise ValueError(f"{where}: bounds {list(map(list, bounds))} must be finite with lower < upper")
    return bounds


def flux_box_faces(box: FluxBox) -> Tuple[FluxPlane, ...]:
    """the six faces of a box, xmin, xmax, ymin, ymax, zmin, zmax, each with the outward direction"""
    faces = []
    for a in range(3):
        inplane = tuple(box.bounds[b] for b in range(3) if b != a)
        for side, d in ((0, -1), (1, 1)):
            faces.append(FluxPlane(f"{box.name}_{'xyz'[a]}{('min', 'max')[side]}", a, box.bounds[a][side], inplane, box.spacing, d, box.name))
    return tuple(faces)


def _flux_planes_config(fc) -> dict:
    """advanced.flux_planes: {enabled: false, start_step: 1, interval: 1, planes: [{name, normal, position, bounds?, spacing?,
    direction?}], boxes: [{name, bounds: [[x0, x1], [y0, y1], [z0, z1]], spacing?}]} -> CaseConfig fields. Absent or disabled: the
    defaults. What needs the domain (a plane outside it, the default bounds' point count) is checked when the plane is planned
    (flux_planes.flux_grid)."""
    if fc is None:
        return {}
    if not isinstance(fc, dict):
        raise ValueError("advanced.flux_planes must be a mapping")
    if not bool(fc.get("enabled", False)):
        return {}
    start, interval = int(fc.get("start_step", 1)), int(fc.get("interval", 1))
    if interval < 1:
        raise ValueError(f"advanced.flux_planes.interval must be >= 1, got {interval}")
    if start < 1:
        raise ValueError(f"advanced.flux_planes.start_step must be >= 1, got {start}")
    raw_planes, raw_boxes = fc.get("planes") or [], fc.get("boxes") or []
    if not isinstance(raw_planes, (list, tuple)) or not isinstance(raw_boxes, (list, tuple)) or not (raw_planes or raw_boxes):
        raise ValueError("advanced.flux_planes.enabled needs at least one plane or box")
    planes, boxes, seen = [], [], set()
    for i, pc in enumerate(raw_planes):
        where = f"advanced.flux_planes.planes[{i}]"
        if not isinstance(pc, dict):
            raise ValueError(f"{where} must be a mapping")
        name = str(pc.get("name", ""))
        _file_stem(where, name, seen)
        where = f"advanced.flux_planes plane {name!r}"
        normal = str(pc.get("normal", "")).lower()
        if normal not in ("x", "y", "z"):
            raise ValueError(f"{where}: normal {pc.get('normal')!r} is not x, y or z")
        if "position" not in pc:
            raise ValueError(f"{where}: position is required")
        position = float(pc["position"])
        if not math.isfinite(position):
            raise ValueError(f"{where}: position {position} is not finite")
        bounds = pc.get("bounds")
        if bounds is not None:
            bounds = _flux_bounds(where, bounds, 2, "[[a0, a1], [b0, b1]]")
        spacing = _flux_spacing(where, pc.get("spacing"))
        direction = pc.get("direction", 1)
        if isinstance(direction, bool) or direction not in (1, -1):
            raise ValueError(f"{where}: direction {direction!r} is not 1 or -1")
        planes.append(FluxPlane(name, "xyz".index(normal), position, bounds, spacing, int(direction)))
    for i, bc in enumerate(raw_boxes):
        where = f"advanced.flux_planes.boxes[{i}]"
        if not isinstance(bc, dict):
            raise ValueError(f"{where} must be a mapping")
        name = str(bc.get("name", ""))
        _file_stem(where, name, seen)
        where = f"advanced.flux_planes box {name!r}"
        bounds = _flux_bounds(where, bc.get("bounds"), 3, "[[x0, x1], [y0, y1], [z0, z1]]")
        boxes.append(FluxBox(name, bounds, _flux_spacing(where, bc.get("spacing"))))
    for b in boxes:
        for f in flux_box_faces(b):
            _file_stem(f"advanced.flux_planes box {b.name!r} face", f.name, seen)
            planes.append(f)
    return dict(flux_planes_enabled=True, flux_planes_start_step=start, flux_planes_interval=interval, flux_planes_planes=tuple(planes),
                flux_planes_boxes=tuple(boxes))


def _fourier_modes_config(mc) -> dict:
    """advanced.fourier_modes: {enabled: false, start_step: 1, interval: 1, samples: 256, window: hann, frequencies: [Hz, ...],
    strouhal: [St, ...], repeat: true} -> CaseConfig fields. Absent or disabled: the defaults (nothing is allocated, launched or
    written). What needs the case's scales - the Strouhal conversion, the Nyquist limit - is checked by modes.plan_modes."""
    if mc is None:
        return {}
    if not isinstance(mc, dict):
        raise ValueError("advanced.fourier_modes must be a mapping")
    if not bool(mc.get("enabled", False)):
        return {}
    start, interval, samples = int(mc.get("start_step", 1)), int(mc.get("interval", 1)), int(mc.get("samples", 256))
    if interval < 1:
        raise ValueError(f"advanced.fourier_modes.interval must be >= 1, got {interval}")
    if start < 1:
        raise ValueError(f"advanced.fourier_modes.start_step must be >= 1, got {start}")
    if not 1 <= samples <= 65536:
        raise ValueError(f"advanced.fourier_modes.samples must be in 1..65536, got {samples}")
    window = str(mc.get("window", "hann")).lower()
    if window not in ("hann", "rectangular"):
        raise ValueError(f"advanced.fourier_modes.window must be hann or rectangular, got {mc.get('window')!r}")
    lists = {}
    for key in ("frequencies", "strouhal"):
        raw = mc.get(key) or []
        if not isinstance(raw, (list, tuple)):
            raise ValueError(f"advanced.fourier_modes.{key} must be a list of numbers")
        vals = tuple(float(v) for v in raw)
        for v in vals:
            if not (math.isfinite(v) and v > 0.0):
                raise ValueError(f"advanced.fourier_modes.{key}: {v} must be finite and > 0")
        lists[key] = vals
    n = len(lists["frequencies"]) + len(lists["strouhal"])
    if not 1 <= n <= 16:
        raise ValueError(f"advanced.fourier_modes: frequencies and strouhal must name 1 to 16 modes in all, got {n}")
    return dict(fourier_modes_enabled=True, fourier_modes_start_step=start, fourier_modes_interval=interval, fourier_modes_samples=samples,
                fourier_modes_window=window, fourier_modes_frequencies=lists["frequencies"], fourier_modes_strouhal=lists["strouhal"],
                fourier_modes_repeat=bool(mc.get("repeat", True)))


ISOSURFACE_FIELDS = ("density", "velocity_magnitude", "q_criterion", "vorticity_magnitude")      # isosurface.FIELDS


@dataclass(frozen=True)
class IsoSurfaceSpec:
    """one surface of advanced.isosurfaces.surfaces (semantics: isosurface.py)"""
    name: str
    field: str                                              # one of ISOSURFACE_FIELDS
    value: float
    bounds: Optional[Tuple[Tuple[float, float], Tuple[float, float], Tuple[float, float]]] = None   # x, y, z; STL frame; None: everything


def _isosurfaces_config(ic) -> dict:
    """advanced.isosurfaces: {enabled: false, start_step: 1, interval: 1, max_triangles: 50000000, surfaces: [{name, field, value,
    bounds?}]} -> CaseConfig fields. Absent or disabled: the defaults."""
    if ic is None:
        return {}
    if not isinstance(ic, dict):
        raise ValueError("advanced.isosurfaces must be a mapping")
    if not bool(ic.get("enabled", False)):
        return {}
    start, interval, cap = int(ic.get("start_step", 1)), int(ic.get("interval", 1)), int(ic.get("max_triangles", 50_000_000))
    if interval < 1:
        raise ValueError(f"advanced.isosurfaces.interval must be >= 1, got {interval}")
    if start < 1:
        raise ValueError(f"advanced.isosurfaces.start_step must be >= 1, got {start}")
    if cap < 1:
        raise ValueError(f"advanced.isosurfaces.max_triangles must be >= 1, got {cap}")
    raw = ic.get("surfaces") or []
    if not isinstance(raw, (list, tuple)) or not raw:
        raise ValueError("advanced.isosurfaces.enabled needs at least one entry in advanced.isosurfaces.surfaces")
    surfaces, seen = [], set()
    for i, sc in enumerate(raw):
        where = f"advanced.isosurfaces.surfaces[{i}]"
        if not isinstance(sc, dict):
            raise ValueError(f"{where} must be a mapping")
        name = str(sc.get("name", ""))
        if not name or not all(ch.isalnum() or ch in "_-." for ch in name) or name.startswith("."):
            raise ValueError(f"{where}.name {name!r} is not a plain file-name stem")
        if name in seen:
            raise ValueError(f"{where}.name {name!r} is not unique")
        seen.add(name)
        field = str(sc.get("field", ""))
        if field not in ISOSURFACE_FIELDS:
            raise ValueError(f"{where}.field {sc.get('field')!r} is unknown (one of {', '.join(ISOSURFACE_FIELDS)})")
        if "value" not in sc:
            raise ValueError(f"{where}.value is required")
        try:
            value = float(sc["value"])
        except (TypeError, ValueError):
            raise ValueError(f"{where}.value {sc['value']!r} is not a number") from None
        if not math.isfinite(value):
            raise ValueError(f"{where}.value {value} is not finite")
        bounds = sc.get("bounds")
        if bounds is not None:
            ok = isinstance(bounds, (list, tuple)) and len(bounds) == 3 and all(isinstance(b, (list, tuple)) and len(b) == 2 for b in bounds)
            if not ok:
                raise ValueError(f"{where}.bounds must be [[x0, x1], [y0, y1], [z0, z1]], got {bounds!r}")
            bounds = tuple((float(b[0]), float(b[1])) for b in bounds)
            for lo, hi in bounds:
                if not (math.isfinite(lo) and math.isfinite(hi)) or not lo < hi:
                    raise ValueError(f"{where}.bounds {list(map(list, bounds))} must be finite with lower < upper")
        surfaces.append(IsoSurfaceSpec(name, field, value, bounds))
    return dict(isosurfaces_enabled=True, isosurfaces_start_step=start, isosurfaces_interval=interval, isosurfaces_max_triangles=cap,
                isosurfaces_surfaces=tuple(surfaces))


STREAMLINE_DIRECTIONS = ("forward", "backward", "both")                                          # streamlines.DIRECTIONS


@dataclass(frozen=True)
class StreamlineSeeds:
    """one group of advanced.streamlines.seeds: its name and its seed points, expanded (semantics: streamlines.py)"""
    name: str
    points: Tuple[Tuple[float, float, float], ...]          # STL frame after stl_scale


def _streamlines_config(sc) -> dict:
    """advanced.streamlines: {enabled: false, start_step: 1, interval: 100, step: 0.5, max_steps: 2000, min_speed: 1e-6, direction: both,
    max_vertices: 20000000, seeds: [{name, points: [[x, y, z], ...]} | {name, line: {from, to, count}}]} -> CaseConfig fields. Absent or
    disabled: the defaults."""
    if sc is None:
        return {}
    if not isinstance(sc, dict):
        raise ValueError("advanced.streamlines must be a mapping")
    if not bool(sc.get("enabled", False)):
        return {}
    from .streamlines import expand_group
    start, interval = int(sc.get("start_step", 1)), int(sc.get("interval", 100))
    if interval < 1:
        raise ValueError(f"advanced.streamlines.interval must be >= 1, got {interval}")
    if start < 1:
        raise ValueError(f"advanced.streamlines.start_step must be >= 1, got {start}")
    try:
        step, min_speed = float(sc.get("step", 0.5)), float(sc.get("min_speed", 1.0e-6))
    except (TypeError, ValueError):
        raise ValueError("advanced.streamlines.step and advanced.streamlines.min_speed must be numbers") from None
    if not (math.isfinite(step) and step > 0.0):
        raise ValueError(f"advanced.streamlines.step must be positive and finite, got {step}")
    if not (math.isfinite(min_speed) and min_speed >= 0.0):
        raise ValueError(f"advanced.streamlines.min_speed must be finite and >= 0, got {min_speed}")
    max_steps, cap = int(sc.get("max_steps", 2000)), int(sc.get("max_vertices", 20_000_000))
    if max_steps < 0:
        raise ValueError(f"advanced.streamlines.max_steps must be >= 0, got {max_steps}")
    if cap < 1:
        raise ValueError(f"advanced.streamlines.max_vertices must be >= 1, got {cap}")
    direction = str(sc.get("direction", "both"))
    if direction not in STREAMLINE_DIRECTIONS:
        raise ValueError(f"advanced.streamlines.direction {sc.get('direction')!r} is unknown (one of {', '.join(STREAMLINE_DIRECTIONS)})")
    raw = sc.get("seeds") or []
    if not isinstance(raw, (list, tuple)) or not raw:
        raise ValueError("advanced.streamlines.enabled needs at least one entry in advanced.streamlines.seeds")
    groups, seen, n_seeds = [], set(), 0
    for i, gc in enumerate(raw):
        where = f"advanced.streamlines.seeds[{i}]"
        if not isinstance(gc, dict):
            raise ValueError(f"{where} must be a mapping")
        name = str(gc.get("name", ""))
        if not name or not all(ch.isalnum() or ch in "_-." for ch in name) or name.startswith("."):
            raise ValueError(f"{where}.name {name!r} is not a plain file-name stem")
        if name in seen:
            raise ValueError(f"{where}.name {name!r} is not unique")
        seen.add(name)
        pts = expand_group(gc, where)
        n_seeds += pts.shape[0]
        groups.append(StreamlineSeeds(name, tuple(tuple(float(v) for v in p) for p in pts)))
    lines = n_seeds * (2 if direction == "both" else 1)
    if lines * (max_steps + 1) > cap:
        raise ValueError(f"advanced.streamlines: {lines} lines of up to max_steps + 1 = {max_steps + 1} vertices are more than "
                         f"advanced.streamlines.max_vertices = {cap}")
    return dict(streamlines_enabled=True, streamlines_start_step=start, streamlines_interval=interval, streamlines_step=step,
                streamlines_max_steps=max_steps, streamlines_min_speed=min_speed, streamlines_direction=direction,
                streamlines_max_vertices=cap, streamlines_seeds=tuple(groups))


@dataclass(frozen=True)
class RenderView:
    """one entry of advanced.render.views (semantics: render.py); camera points in the STL frame after stl_scale"""
    name: str
    field: str                                              # isosurface.FIELDS
    lo: float
    hi: float
    colormap: Tuple[Tuple[float, float, float, float, float], ...]   # control points [x, r, g, b, opacity]
    opacity: float                                          # times the control points' opacity: extinction per coarse cell length
    camera: Tuple[Tuple[str, object], ...]                  # the camera mapping's items, validated
    step: float
    max_samples: int
    background: Tuple[float, float, float]
    body_color: Tuple[float, float, float]


def _render_config(rc) -> dict:
    """advanced.render: {enabled: false, start_step: 1, interval: 100, width: 1280, height: 720, max_pixels: 8294400, views: [{name, field,
    range: [lo, hi], colormap: gray | heat | coolwarm | [[x, r, g, b, opacity], ...], opacity: 1.0, camera: {type, position, look_at, up,
    fov | extent}, step: 0.5, max_samples: 4096, background: [0, 0, 0], body_color: [0.7, 0.7, 0.7]}]} -> CaseConfig fields. Absent or
    disabled: the defaults."""
    if rc is None:
        return {}
    if not isinstance(rc, dict):
        raise ValueError("advanced.render must be a mapping")
    if not bool(rc.get("enabled", False)):
        return {}
    from .isosurface import FIELDS
    from .render import Camera, control_points
    try:
        start, interval = int(rc.get("start_step", 1)), int(rc.get("interval", 100))
        width, height, cap = int(rc.get("width", 1280)), int(rc.get("height", 720)), int(rc.get("max_pixels", 8_294_400))
    except (TypeError, ValueError):
        raise ValueError("advanced.render: start_step, interval, width, height and max_pixels must be integers") from None
    for key, v in (("interval", interval), ("start_step", start), ("width", width), ("height", height), ("max_pixels", cap)):
        if v < 1:
            raise ValueError(f"advanced.render.{key} must be >= 1, got {v}")
    if width * height > cap:
        raise ValueError(f"advanced.render: width x height = {width * height} pixels are more than advanced.render.max_pixels = {cap}")
    raw = rc.get("views") or []
    if not isinstance(raw, (list, tuple)) or not raw:
        raise ValueError("advanced.render.enabled needs at least one entry in advanced.render.views")

    def colour(vc, key, default, where):
        try:
            c = tuple(float(v) for v in vc.get(key, default))
        except (TypeError, ValueError):
            raise ValueError(f"{where}.{key} must be [r, g, b]") from None
        if len(c) != 3 or not all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in c):
            raise ValueError(f"{where}.{key} must be three numbers in 0..1, got {list(c)}")
        return c
    views, seen = [], set()
    for i, vc in enumerate(raw):
        where = f"advanced.render.views[{i}]"
        if not isinstance(vc, dict):
            raise ValueError(f"{where} must be a mapping")
        name = str(vc.get("name", ""))
        if not name or not all(ch.isalnum() or ch in "_-." for ch in name) or name.startswith("."):
            raise ValueError(f"{where}.name {name!r} is not a plain file-name stem")
        if name in seen:
            raise ValueError(f"{where}.name {name!r} is not unique")
        seen.add(name)
        field = str(vc.get("field", ""))
        if field not in FIELDS:
            raise ValueError(f"{where}.field {vc.get('field')!r} is unknown (one of {', '.join(FIELDS)})")
        try:
            lo, hi = (float(v) for v in vc["range"])
        except (KeyError, TypeError, ValueError):
            raise ValueError(f"{where}.range must be [lo, hi]") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and float(np.float32(hi)) > float(np.float32(lo))):
            raise ValueError(f"{where}.range must be finite with hi > lo in float32, got [{lo}, {hi}]")
        points = control_points(vc.get("colormap", "gray"), f"{where}.colormap")
        try:
            opacity, step = float(vc.get("opacity", 1.0)), float(vc.get("step", 0.5))
            max_samples = int(vc.get("max_samples", 4096))
        except (TypeError, ValueError):
            raise ValueError(f"{where}.opacity, {where}.step and {where}.max_samples must be numbers") from None
        if not (math.isfinite(opacity) and opacity >= 0.0):
            raise ValueError(f"{where}.opacity must be finite and >= 0, got {opacity}")
        if not (math.isfinite(step) and step > 0.0):
            raise ValueError(f"{where}.step must be positive and finite, got {step}")
        if max_samples < 1:
            raise ValueError(f"{where}.max_samples must be >= 1, got {max_samples}")
        cam = vc.get("camera")
        Camera.build(cam, width, height, where=f"{where}.camera")          # refuses what it cannot build
        cam_items = tuple((str(k), tuple(float(x) for x in v) if isinstance(v, (list, tuple)) else v) for k, v in sorted(cam.items()))
        views.append(RenderView(name, field, lo, hi, tuple(tuple(float(v) for v in p) for p in points), opacity, cam_items, step,
                                max_samples, colour(vc, "background", (0.0, 0.0, 0.0), where), colour(vc, "body_color", (0.7, 0.7, 0.7), where)))
    return dict(render_enabled=True, render_start_step=start, render_interval=interval, render_width=width, render_height=height,
                render_max_pixels=cap, render_views=tuple(views))


def _tracers_config(tc, steps: int) -> dict:
    """advanced.tracers: {enabled: false, start_step: 1, interval: 1, release_every: 10, generations: 64, output_interval: 100,
    max_particles: 4000000, seeds: [{name, points: [[x, y, z], ...]} | {name, line: {from, to, count}}]} -> CaseConfig fields. interval:
    coarse steps per advance (= dt); release_every: in advances; output_interval: in coarse steps, a multiple of interval. Absent or
    disabled: the defaults."""
    if tc is None:
        return {}
    if not isinstance(tc, dict):
        raise ValueError("advanced.tracers must be a mapping")
    if not bool(tc.get("enabled", False)):
        return {}
    from .streamlines import expand_group
    from .tracers import check_capacity
    try:
        start, interval = int(tc.get("start_step", 1)), int(tc.get("interval", 1))
        release, gens = int(tc.get("release_every", 10)), int(tc.get("generations", 64))
        out_interval, cap = int(tc.get("output_interval", 100)), int(tc.get("max_particles", 4_000_000))
    except (TypeError, ValueError):
        raise ValueError("advanced.tracers: start_step, interval, release_every, generations, output_interval and max_particles must be "
                         "integers") from None
    for key, v in (("interval", interval), ("start_step", start), ("release_every", release), ("generations", gens),
                   ("output_interval", out_interval), ("max_particles", cap)):
        if v < 1:
            raise ValueError(f"advanced.tracers.{key} must be >= 1, got {v}")
    if out_interval % interval != 0:
        raise ValueError(f"advanced.tracers.output_interval {out_interval} must be a multiple of advanced.tracers.interval {interval}")
    raw = tc.get("seeds") or []
    if not isinstance(raw, (list, tuple)) or not raw:
        raise ValueError("advanced.tracers.enabled needs at least one entry in advanced.tracers.seeds")
    groups, seen, n_seeds = [], set(), 0
    for i, gc in enumerate(raw):
        where = f"advanced.tracers.seeds[{i}]"
        if not isinstance(gc, dict):
            raise ValueError(f"{where} must be a mapping")
        name = str(gc.get("name", ""))
        if not name or not all(ch.isalnum() or ch in "_-." for ch in name) or name.startswith("."):
            raise ValueError(f"{where}.name {name!r} is not a plain file-name stem")
        if name in seen:
            raise ValueError(f"{where}.name {name!r} is not unique")
        seen.add(name)
        pts = expand_group(gc, where)
        n_seeds += pts.shape[0]
        groups.append(StreamlineSeeds(name, tuple(tuple(float(v) for v in p) for p in pts)))
    check_capacity(n_seeds, gens, cap, steps, start, interval, release)
    return dict(tracers_enabled=True, tracers_start_step=start, tracers_interval=interval, tracers_release_every=release,
                tracers_generations=gens, tracers_output_interval=out_interval, tracers_max_particles=cap, tracers_seeds=tuple(groups))


# ----------------------------------------------------------------------------------------------------------------
# geometry, src/geometry.jl
# ----------------------------------------------------------------------------------------------------------------
@dataclass
class SolverMesh:
    triangles: np.ndarray      # [n,3,3] Float64 (Float32 file values widened, times scale)
    min_bounds: np.ndarray
    max_bounds: np.ndarray
    normals: np.ndarray        # [n,3]
    areas: np.ndarray          # [n]
    centers: np.ndarray        # [n,3]


def load_mesh(filename: str, scale: float = 1.0) -> SolverMesh:
    """load_mesh (src/geometry.jl:160-209): binary/ASCII sniffing, Float32 -> Float64 * scale, properties from vertices."""
    size = os.path.getsize(filename)
    is_binary = True
    with open(filename, "rb") as fh:
        if size < 84:
            is_binary = False
        else:
            head = fh.read(5)
            if head.decode("latin1").lower().startswith("solid"):
                fh.seek(80)
                count = struct.unpack("<I", fh.read(4))[0]
                if size != 84 + count * 50:
                    is_binary = False
    if is_binary:
        raw = open(filename, "rb").read()
        count = struct.unpack("<I", raw[80:84])[0]
        rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=count, offset=84)
        tris = rec["v"].astype(np.float64) * scale
    else:
        verts, cur = [], []
        for line in open(filename):
            s = line.strip()
            if s.startswith("vertex"):
                p = s.split()
                if len(p) >= 4:
                    cur.append([float(p[1]) * scale, float(p[2]) * scale, float(p[3]) * scale])
            elif s.startswith("endloop"):
                if len(cur) == 3:
                    verts.append(cur)
                cur = []
        tris = np.asarray(verts, dtype=np.float64).reshape(-1, 3, 3)
    if tris.shape[0] == 0:
        raise ValueError("No triangles loaded.")
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    cp = np.cross(e1, e2)
    area = 0.5 * np.linalg.norm(cp, axis=1)
    normal = np.where((area > 1e-12)[:, None], cp / np.maximum(2.0 * area, 1e-300)[:, None], 0.0)
    centers = (tris[:, 0] + tris[:, 1] + tris[:, 2]) / 3.0
    flat = tris.reshape(-1, 3)
    return SolverMesh(tris, flat.min(axis=0), flat.max(axis=0), normal, area, centers)


# ----------------------------------------------------------------------------------------------------------------
# scaling, src/physics_scaling.jl:59-176
# ----------------------------------------------------------------------------------------------------------------
@dataclass
class DomainParameters:
    num_levels: int
    mesh_min: np.ndarray
    mesh_max: np.ndarray
    mesh_center: np.ndarray
    mesh_extent: np.ndarray
    reference_length: float
    reference_chord: float
    reference_area: float
    moment_center: Tuple[float, float, float]
    domain_size: Tuple[float, float, float]
    mesh_offset: np.ndarray
    dx_fine: float
    dx_coarse: float
    dx_levels: List[float]
    nx_coarse: int
    ny_coarse: int
    nz_coarse: int
    bx_max: int
    by_max: int
    bz_max: int
    tau_levels: List[np.float32]
    re_number: float
    u_physical: float
    rho_physical: float
    nu_physical: float
    length_scale: float
    time_scale: float
    velocity_scale: float
    force_scale: float
    tau_fine: float
    wall_model_active: bool


def compute_domain_from_mesh(mesh_min, mesh_max, cfg: CaseConfig) -> DomainParameters:
    mesh_min = np.asarray(mesh_min, dtype=np.float64)
    mesh_max = np.asarray(mesh_max, dtype=np.float64)
    center = (mesh_min + mesh_max) / 2
    extent = mesh_max - mesh_min
    if cfg.reference_length_for_meshing > 0:
        L = cfg.reference_length_for_meshing
    else:
        L = {"x": extent[0], "y": extent[1], "z": extent[2]}.get(cfg.reference_dimension, float(extent.max()))
    chord = cfg.reference_chord if cfg.reference_chord > 0 else float(extent[0])
    area = cfg.reference_area_config if cfg.reference_area_config > 0 else (
        extent[1] * extent[2] * 2 if cfg.symmetric_analysis else extent[1] * extent[2])
    u_phys, nu_phys, rho_phys = cfg.flow_velocity, cfg.fluid_kinematic_viscosity, cfg.fluid_density
    re = u_phys * L / nu_phys
    tau_fine_computed = 3.0 * (float(cfg.u_lattice) * cfg.surface_resolution / re) + 0.5        # :66-69
    tau_fine = max(tau_fine_computed, float(cfg.tau_min))
    dom_x = L * (cfg.domain_upstream + cfg.domain_downstream) + extent[0]
    dom_y = (mesh_max[1] + L * cfg.domain_lateral) if cfg.symmetric_analysis else (extent[1] + 2 * L * cfg.domain_lateral)
    dom_z = extent[2] + 2 * L * cfg.domain_height
    dx_fine = L / cfg.surface_resolution
    min_domain = min(dom_x, dom_y, dom_z)
    ratio = min_domain / (dx_fine * cfg.min_coarse_blocks * cfg.block_size_config)
    max_levels_domain = 1 if ratio < 1.0 else int(math.floor(1 + math.log2(ratio)))
    if cfg.num_levels > 0:
        num_levels = min(cfg.num_levels, max_levels_domain)
    else:
        num_levels = min(max_levels_domain, cfg.max_levels) if cfg.auto_levels else min(8, max_levels_domain)
    dx_coarse = dx_fine * 2 ** (num_levels - 1)
    dx_levels = [dx_fine * 2 ** (num_levels - lvl) for lvl in range(1, num_levels + 1)]
    B = cfg.block_size_config
    ncoarse = lambda d: max(B, int(math.ceil(math.ceil(d / dx_coarse) / B) * B))
    nx, ny, nz = ncoarse(dom_x), ncoarse(dom_y), ncoarse(dom_z)
    dom_x, dom_y, dom_z = nx * dx_coarse, ny * dx_coarse, nz * dx_coarse
    mesh_x = L * cfg.domain_upstream
    mesh_y = 0.0 if cfg.symmetric_analysis else (dom_y / 2 - center[1])
    mesh_z = dom_z / 2 - center[2]
    offset = np.array([mesh_x - mesh_min[0], mesh_y, mesh_z])
    length_scale = dx_fine
    velocity_scale = u_phys / float(cfg.u_lattice)
    time_scale = length_scale / velocity_scale
    tau_levels = [np.float32(tau_fine if lvl == num_levels else 0.5 + (tau_fine - 0.5) * 2.0 ** (num_levels - lvl))
                  for lvl in range(1, num_levels + 1)]
    force_scale = rho_phys * length_scale ** 4 / time_scale ** 2
    mc = cfg.moment_center
    moment_center = (mesh_min[0] + offset[0] + mc[0] * chord, center[1] + offset[1] + mc[1] * chord, center[2] + offset[2] + mc[2] * chord)
    return DomainParameters(num_levels, mesh_min, mesh_max, center, extent, L, chord, float(area), moment_center, (dom_x, dom_y, dom_z),
                            offset, dx_fine, dx_coarse, dx_levels, nx, ny, nz, nx // B, ny // B, nz // B, tau_levels, re, u_phys,
                            rho_phys, nu_phys, length_scale, time_scale, velocity_scale, force_scale, tau_fine, cfg.wall_model_enabled)


# ----------------------------------------------------------------------------------------------------------------
# block topology, src/domain_topology.jl:9-133
# ----------------------------------------------------------------------------------------------------------------
Coord = Tuple[int, int, int]


def get_active_blocks_for_level(mesh: SolverMesh, dx: float, offset, bmax: Coord) -> Set[Coord]:
    margin = dx * 0.01
    inv = 1.0 / (BS * dx)
    t = mesh.triangles + np.asarray(offset)
    tmin, tmax = t.min(axis=1), t.max(axis=1)
    lo = np.floor((tmin - margin) * inv).astype(np.int64) + 1
    hi = np.floor((tmax + margin) * inv).astype(np.int64) + 1
    lo = np.maximum(lo, 1)
    hi = np.minimum(hi, np.asarray(bmax))
    out: Set[Coord] = set()
    for (a, b) in {(tuple(l), tuple(h)) for l, h in zip(lo, hi)}:
        for bz in range(a[2], b[2] + 1):
            for by in range(a[1], b[1] + 1):
                for bx in range(a[0], b[0] + 1):
                    out.add((bx, by, bz))
    return out


def _siblings(c: Coord):
    p = ((c[0] + 1) // 2, (c[1] + 1) // 2, (c[2] + 1) // 2)
    for dbz in (0, 1):
        for dby in (0, 1):
            for dbx in (0, 1):
                yield (2 * p[0] - 1 + dbx, 2 * p[1] - 1 + dby, 2 * p[2] - 1 + dbz)


def _inside(c: Coord, bmax: Coord) -> bool:
    return 1 <= c[0] <= bmax[0] and 1 <= c[1] <= bmax[1] and 1 <= c[2] <= bmax[2]


def add_halo_blocks_with_siblings(active: Set[Coord], layers: int, bmax: Coord) -> None:
    offs = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
    for _ in range(layers):
        new = set()
        for (bx, by, bz) in active:
            for (dx, dy, dz) in offs:
                n = (bx + dx, by + dy, bz + dz)
                if _inside(n, bmax) and n not in active:
                    new.add(n)
        sib = set()
        for c in new:
            for s in _siblings(c):
                if _inside(s, bmax) and s not in active and s not in new:
                    sib.add(s)
        active |= new
        active |= sib


def ensure_complete_parent_coverage(active: Set[Coord], bmax: Coord) -> None:
    added, it = True, 0
    while added and it < 10:
        added = False
        it += 1
        sib = set()
        for c in active:
            for s in _siblings(c):
                if _inside(s, bmax) and s not in active:
                    sib.add(s)
                    added = True
        active |= sib


# ----------------------------------------------------------------------------------------------------------------
# dense helper: a level's cells as one boolean volume (blocks that do not exist are "inactive")
# ----------------------------------------------------------------------------------------------------------------
class _Dense:
    def __init__(self, coords: Sequence[Coord]):
        c = np.asarray(coords, dtype=np.int64)
        self.lo = c.min(axis=0)
        self.nb = c.max(axis=0) - self.lo + 1
        self.rel = c - self.lo
        self.shape = tuple(int(v) for v in self.nb * BS)
        self.active = np.zeros(self.shape, dtype=bool)
        for (x, y, z) in self.rel:
            self.active[x * BS:(x + 1) * BS, y * BS:(y + 1) * BS, z * BS:(z + 1) * BS] = True

    def to_dense(self, arr4: np.ndarray) -> np.ndarray:
        out = np.zeros(self.shape, dtype=arr4.dtype)
        for i, (x, y, z) in enumerate(self.rel):
            out[x * BS:(x + 1) * BS, y * BS:(y + 1) * BS, z * BS:(z + 1) * BS] = arr4[:, :, :, i]
        return out

    def to_blocks(self, dense: np.ndarray, n: int) -> np.ndarray:
        out = np.zeros((BS, BS, BS, n), dtype=dense.dtype, order="F")
        for i, (x, y, z) in enumerate(self.rel):
            out[:, :, :, i] = dense[x * BS:(x + 1) * BS, y * BS:(y + 1) * BS, z * BS:(z + 1) * BS]
        return out


def _cell_centers(coords, dx: float):
    """cell centres ((b-1)*8 + l - 0.5) dx, arrays of shape (8,8,8,nb) (src/domain_generation.jl:91-93)"""
    c = np.asarray(coords, dtype=np.float64)
    l = np.arange(1, BS + 1, dtype=np.float64)
    px = ((c[:, 0][None, None, None, :] - 1) * BS + l[:, None, None, None] - 0.5) * dx
    py = ((c[:, 1][None, None, None, :] - 1) * BS + l[None, :, None, None] - 0.5) * dx
    pz = ((c[:, 2][None, None, None, :] - 1) * BS + l[None, None, :, None] - 0.5) * dx
    shp = (BS, BS, BS, len(coords))
    return np.broadcast_to(px, shp), np.broadcast_to(py, shp), np.broadcast_to(pz, shp)


def _block_triangle_map(mesh: SolverMesh, coords, dx: float, offset, margin: float) -> List[np.ndarray]:
    """build_block_triangle_map (src/domain_generation.jl:34-72) / ..._for_bouzidi (src/bouzidi_setup.jl:11-52)"""
    lookup = {tuple(c): i for i, c in enumerate(coords)}
    t = mesh.triangles + np.asarray(offset)
    lo = np.floor((t.min(axis=1) - margin) / (BS * dx)).astype(np.int64) + 1
    hi = np.floor((t.max(axis=1) + margin) / (BS * dx)).astype(np.int64) + 1
    lo = np.maximum(lo, 1)
    lists: List[List[int]] = [[] for _ in coords]
    for ti in range(t.shape[0]):
        for bz in range(lo[ti, 2], hi[ti, 2] + 1):
            for by in range(lo[ti, 1], hi[ti, 1] + 1):
                for bx in range(lo[ti, 0], hi[ti, 0] + 1):
                    i = lookup.get((bx, by, bz))
                    if i is not None:
                        lists[i].append(ti)
    return [np.asarray(l, dtype=np.int64) for l in lists]


# ----------------------------------------------------------------------------------------------------------------
# voxelizer, src/domain_generation.jl:10-112
# ----------------------------------------------------------------------------------------------------------------
def _tri_box_overlap(centers: np.ndarray, half: float, v1: np.ndarray, v2: np.ndarray, v3: np.ndarray) -> np.ndarray:
    """triangle_intersects_aabb for every (cell, triangle) pair: AABB slabs + the 9 edge-cross axes (the reference has
    no triangle-plane test). centers [C,3]; v* [T,3]; returns bool [C,T]."""
    h = half * 1.001
    t1 = v1[None, :, :] - centers[:, None, :]
    t2 = v2[None, :, :] - centers[:, None, :]
    t3 = v3[None, :, :] - centers[:, None, :]
    mn = np.minimum(np.minimum(t1, t2), t3)
    mx = np.maximum(np.maximum(t1, t2), t3)
    ok = ~((mn > h).any(axis=2) | (mx < -h).any(axis=2))
    if not ok.any():
        return ok
    f = [t2 - t1, t3 - t2, t1 - t3]
    for i in range(3):
        u = np.zeros(3)
        u[i] = 1.0
        for j in range(3):
            axis = np.cross(u, f[j])
            use = (axis * axis).sum(axis=2) >= 1e-10
            p1 = (t1 * axis).sum(axis=2); p2 = (t2 * axis).sum(axis=2); p3 = (t3 * axis).sum(axis=2)
            aa = np.abs(axis)
            r = (h * aa[..., 0] + h * aa[..., 1]) + h * aa[..., 2]          # :28, term by term
            sep = (np.minimum(p1, np.minimum(p2, p3)) > r) | (np.maximum(p1, np.maximum(p2, p3)) < -r)
            ok &= ~(use & sep)
    return ok


def _candidate_pairs(tmin: np.ndarray, tmax: np.ndarray, reach: float, dx: float, dense: "_Dense"):
    """All (cell, triangle) pairs whose cell CENTRE lies within `reach` of the triangle's bounding box (per axis), for
    cells of existing blocks. Returns (flat dense cell index, triangle index, cell centre [P,3])."""
    org = dense.lo.astype(np.float64) - 1.0                     # block coord 1 starts at cell 0
    lo = np.ceil((tmin - reach) / dx - 0.5 - 1e-9).astype(np.int64) - (org * BS).astype(np.int64)
    hi = np.floor((tmax + reach) / dx - 0.5 + 1e-9).astype(np.int64) - (org * BS).astype(np.int64)
    shp = np.asarray(dense.shape)
    lo = np.maximum(lo, 0)
    hi = np.minimum(hi, shp - 1)
    ext = np.maximum(hi - lo + 1, 0)
    cnt = ext[:, 0] * ext[:, 1] * ext[:, 2]
    tri = np.repeat(np.arange(len(cnt)), cnt)
    start = np.repeat(np.cumsum(cnt) - cnt, cnt)
    r = np.arange(cnt.sum()) - start
    ex, ey = ext[tri, 0], ext[tri, 1]
    ix = lo[tri, 0] + r % ex
    iy = lo[tri, 1] + (r // ex) % ey
    iz = lo[tri, 2] + r // (ex * ey)
    keep = dense.active[ix, iy, iz]
    ix, iy, iz, tri = ix[keep], iy[keep], iz[keep], tri[keep]
    base = (org * BS)
    centre = np.stack([(ix + base[0] + 0.5) * dx, (iy + base[1] + 0.5) * dx, (iz + base[2] + 0.5) * dx], axis=1)
    return np.ravel_multi_index((ix, iy, iz), dense.shape), tri, centre


def _tri_box_overlap_pairs(c: np.ndarray, half: float, v1: np.ndarray, v2: np.ndarray, v3: np.ndarray) -> np.ndarray:
    """triangle_intersects_aabb (src/domain_generation.jl:10-32) for a list of (cell centre, triangle) pairs [P,3]:
    AABB slabs + the 9 edge-cross axes (the reference has no triangle-plane test)."""
    h = half * 1.001
    t1, t2, t3 = v1 - c, v2 - c, v3 - c
    mn = np.minimum(np.minimum(t1, t2), t3)
    mx = np.maximum(np.maximum(t1, t2), t3)
    ok = ~((mn > h).any(axis=1) | (mx < -h).any(axis=1))
    f = [t2 - t1, t3 - t2, t1 - t3]
    for i in range(3):
        u = np.zeros(3)
        u[i] = 1.0
        for j in range(3):
            axis = np.cross(u, f[j])
            use = (axis * axis).sum(axis=1) >= 1e-10
            p1 = (t1 * axis).sum(axis=1); p2 = (t2 * axis).sum(axis=1); p3 = (t3 * axis).sum(axis=1)
            aa = np.abs(axis)
            r = (h * aa[:, 0] + h * aa[:, 1]) + h * aa[:, 2]                # :28, term by term
            sep = (np.minimum(p1, np.minimum(p2, p3)) > r) | (np.maximum(p1, np.maximum(p2, p3)) < -r)
            ok &= ~(use & sep)
    return ok


def _native_inputs(coords, mesh: SolverMesh, offset):
    """(library, int32 [nb,3] block coordinates, Float64 [T,3,3] triangles with the mesh offset added, threads)"""
    from . import _setup_lib
    lib = _setup_lib.load()
    c = np.ascontiguousarray(np.asarray(coords, dtype=np.int32).reshape(-1, 3))
    tri = None if mesh is None else np.ascontiguousarray(mesh.triangles + np.asarray(offset), dtype=np.float64)
    return lib, c, tri, _setup_lib.n_threads()


def _ptr(a: np.ndarray):
    return a.ctypes.data


def voxelize_blocks(coords, mesh: SolverMesh, dx: float, offset, method: str = "native") -> np.ndarray:
    """voxelize_blocks! (src/domain_generation.jl:74-112). The reference tests every cell of a block against the
    triangles binned to that block (margin 2 dx); a triangle can only touch a cell's 0.75 dx half-box if the cell centre
    is within 0.75075 dx of the triangle's bounding box, so testing exactly those pairs gives the same voxels.
    method "native": libludwig_setup.so, block by block like the reference; "numpy": the restatement below (the checker)."""
    n = len(coords)
    if method == "native":
        from . import _setup_lib
        lib, c, tri, nt = _native_inputs(coords, mesh, offset)
        obs = np.zeros((BS, BS, BS, n), dtype=np.uint8, order="F")
        _setup_lib.check(lib.lws_voxelize(_ptr(tri), tri.shape[0], float(dx), _ptr(c), n, _ptr(obs), nt), "lws_voxelize")
        return obs.view(np.bool_)
    d = _Dense(coords)
    tri = mesh.triangles + np.asarray(offset)
    cell, ti, centre = _candidate_pairs(tri.min(axis=1), tri.max(axis=1), 0.75 * dx * 1.001, dx, d)
    hit = _tri_box_overlap_pairs(centre, 0.75 * dx, tri[ti, 0], tri[ti, 1], tri[ti, 2])
    dense = np.zeros(d.shape, dtype=bool)
    dense.reshape(-1)[cell[hit]] = True
    return d.to_blocks(dense, n)


def perform_flood_fill(obstacle: np.ndarray, coords, method: str = "native") -> int:
    """6-connected fill of everything not reachable from the fluid cells of the min-x blocks (src/domain_generation.jl:114-203).
    Returns the number of interior voxels turned solid (the count the reference prints)."""
    if method == "native":
        from . import _setup_lib
        lib, c, _, _ = _native_inputs(coords, None, None)
        assert obstacle.flags.f_contiguous and obstacle.dtype == np.bool_
        return _setup_lib.check(lib.lws_flood_fill(_ptr(c), len(coords), _ptr(obstacle)), "lws_flood_fill")
    from scipy import ndimage
    d = _Dense(coords)
    obs = d.to_dense(obstacle)
    free = d.active & ~obs
    lab, _ = ndimage.label(free, structure=ndimage.generate_binary_structure(3, 1))
    c = np.asarray(coords)
    seed = np.zeros(d.shape, dtype=bool)
    for (x, y, z) in d.rel[c[:, 0] == c[:, 0].min()]:
        seed[x * BS:(x + 1) * BS, y * BS:(y + 1) * BS, z * BS:(z + 1) * BS] = True
    reach_labels = np.unique(lab[seed & free])
    reach_labels = reach_labels[reach_labels > 0]
    visited = np.isin(lab, reach_labels)
    fill = free & ~visited
    obstacle[...] = d.to_blocks(obs | fill, len(coords))
    return int(fill.sum())


# ----------------------------------------------------------------------------------------------------------------
# sponge, src/domain_generation.jl:205-289
# ----------------------------------------------------------------------------------------------------------------
def _profile(x: np.ndarray, thickness: float) -> np.ndarray:
    return np.where(x <= 0.0, 1.0, np.where(x >= thickness, 0.0, 0.5 * (1.0 + np.cos(np.pi * x / thickness))))


def apply_sponge(coords, params: DomainParameters, lvl_scale: int, cfg: CaseConfig) -> np.ndarray:
    dx = params.dx_coarse / lvl_scale
    Lx, Ly, Lz = params.domain_size
    st = float(cfg.sponge_thickness)
    outlet_t = Lx * max(st, 0.15)
    inlet_t = Lx * 0.02
    y_t, z_t = Ly * st * 0.5, Lz * st * 0.5
    outlet_start, y_top, z_back = Lx - outlet_t, Ly - y_t, Lz - z_t
    # every term depends on ONE coordinate and the result is their maximum: evaluate the profiles on the [8, nb] coordinate arrays
    # of each axis and combine by broadcasting (same expressions on the same Float64 inputs as the cell-by-cell form)
    c = np.asarray(coords, dtype=np.float64)
    l = np.arange(1, BS + 1, dtype=np.float64)
    px, py, pz = (((c[:, a][None, :] - 1) * BS + l[:, None] - 0.5) * dx for a in range(3))
    vx = np.zeros(px.shape)
    vx = np.where(px > outlet_start, np.maximum(vx, _profile(outlet_t - (px - outlet_start), outlet_t) * 1.0), vx)
    vx = np.where(px < inlet_t, np.maximum(vx, _profile(px, inlet_t) * 0.05), vx)
    vy = np.zeros(py.shape)
    if not cfg.symmetric_analysis:
        vy = np.where(py < y_t, np.maximum(vy, _profile(py, y_t) * 0.1), vy)
    vy = np.where(py > y_top, np.maximum(vy, _profile(y_t - (py - y_top), y_t) * 0.1), vy)
    vz = np.zeros(pz.shape)
    vz = np.where(pz < z_t, np.maximum(vz, _profile(pz, z_t) * 0.1), vz)
    vz = np.where(pz > z_back, np.maximum(vz, _profile(z_t - (pz - z_back), z_t) * 0.1), vz)
    vx, vy, vz = (v.astype(np.float32) for v in (vx, vy, vz))          # rounding is monotone: max then round = round then max
    # built as C-ordered [nb, z, y, x] (memory order of the Fortran [x, y, z, nb] array the level holds), returned as that view
    val = np.maximum(np.maximum(vx.T[:, None, None, :], vy.T[:, None, :, None]), vz.T[:, :, None, None])
    return val.transpose(3, 2, 1, 0)


# ----------------------------------------------------------------------------------------------------------------
# wall distance, src/domain_generation.jl:371-434 (values are metres used as lattice units downstream: Appendix A.6)
# ----------------------------------------------------------------------------------------------------------------
def compute_wall_distances(coords, obstacle: np.ndarray, dx: float, method: str = "native") -> np.ndarray:
    if method == "native":
        from . import _setup_lib
        lib, c, _, nt = _native_inputs(coords, None, None)
        assert obstacle.flags.f_contiguous and obstacle.dtype == np.bool_
        wall = np.full(obstacle.shape, np.float32(100.0), dtype=np.float32, order="F")
        _setup_lib.check(lib.lws_wall_distance(_ptr(c), len(coords), _ptr(obstacle), float(dx), _ptr(wall), nt), "lws_wall_distance")
        return wall
    d = _Dense(coords)
    obs = d.to_dense(obstacle)
    best = np.full(d.shape, np.float32(100.0), dtype=np.float32)
    near = np.zeros(d.shape, dtype=bool)
    pad_o = np.pad(obs, 1)
    fdx = np.float32(dx)
    sx, sy, sz = d.shape
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dxo in (-1, 0, 1):
                if (dxo, dy, dz) == (0, 0, 0):
                    continue
                nb_obs = pad_o[1 + dxo:1 + dxo + sx, 1 + dy:1 + dy + sy, 1 + dz:1 + dz + sz]   # missing blocks hold False
                dist = np.float32(np.sqrt(np.float32(dxo * dxo + dy * dy + dz * dz))) * fdx
                near |= nb_obs
                best = np.where(nb_obs, np.minimum(best, dist), best)
    res = np.where(near & ~obs & d.active, best, np.float32(100.0)).astype(np.float32)
    return d.to_blocks(res, len(coords))


# ----------------------------------------------------------------------------------------------------------------
# Bouzidi q-map, src/bouzidi_setup.jl:64-167 + src/bouzidi_math.jl:9-102
# ----------------------------------------------------------------------------------------------------------------
def _boundary_cell_lists(mark: np.ndarray):
    """sorted boundary-cell lists (block, then z, y, x) from a bool [8,8,8,nb] (F order) marker"""
    flat = np.flatnonzero(mark.reshape(-1, order="F"))
    b, cell = flat // 512, flat % 512
    return ((b + 1).astype(np.int32), (cell % 8 + 1).astype(np.int8), ((cell // 8) % 8 + 1).astype(np.int8),
            (cell // 64 + 1).astype(np.int8), int(flat.shape[0]))


def compute_bouzidi_qmap_sparse(coords, mesh: SolverMesh, dx: float, offset, shell: Optional[np.ndarray] = None, method: str = "native"):
    """Returns (q_map Float16 [8,8,8,nb,27], cell_block, cell_x, cell_y, cell_z (1-based), n_boundary_cells).

    The reference casts, from every cell of every block that has triangles binned to it (margin 2.5 dx), 26 rays against
    all binned triangles and keeps q = t_min / (dx |c|) if 0 < q <= 1. A link is at most sqrt(3) dx long, so only
    triangles whose bounding box is within sqrt(3) dx of the cell centre can give q <= 1, and a farther triangle can
    never undercut a nearer hit: evaluating exactly those (cell, triangle) pairs gives the same q-map. The list order is
    thread-dependent in the reference and irrelevant (Appendix A.11); here it is sorted.
    method "native": libludwig_setup.so (a thread per block, as the reference); "numpy": the restatement below (the checker)."""
    n = len(coords)
    if method == "native":
        from . import _setup_lib
        lib, c, tri, nt = _native_inputs(coords, mesh, offset)
        q_map = np.zeros((BS, BS, BS, n, 27), dtype=np.float16, order="F")
        mark = np.zeros((BS, BS, BS, n), dtype=np.uint8, order="F")
        nbc = _setup_lib.check(lib.lws_bouzidi_qmap(_ptr(tri), tri.shape[0], float(dx), _ptr(c), n, _ptr(q_map), _ptr(mark), nt),
                               "lws_bouzidi_qmap")
        cb, cx, cy, cz, cnt = _boundary_cell_lists(mark)
        assert cnt == nbc
        return q_map, cb, cx, cy, cz, nbc
    d = _Dense(coords)
    tri = mesh.triangles + np.asarray(offset)
    cell, ti, o = _candidate_pairs(tri.min(axis=1), tri.max(axis=1), math.sqrt(3.0) * dx * 1.0001, dx, d)
    order = np.argsort(cell, kind="stable")
    cell, ti, o = cell[order], ti[order], o[order]
    ucell, first = np.unique(cell, return_index=True)
    v1 = tri[ti, 0]
    e1, e2 = tri[ti, 1] - v1, tri[ti, 2] - v1
    sv = o - v1
    qv = np.cross(sv, e1)
    t_num = (e2 * qv).sum(axis=1)
    EPS = 1e-9
    qdense = np.zeros((27,) + d.shape, dtype=np.float16)
    any_hit = np.zeros(len(ucell), dtype=bool)
    k = -1
    for cz in (-1, 0, 1):
        for cy in (-1, 0, 1):
            for cx in (-1, 0, 1):
                k += 1
                if (cx, cy, cz) == (0, 0, 0):
                    continue
                cm = math.sqrt(cx * cx + cy * cy + cz * cz)
                dn = np.array([cx, cy, cz], dtype=np.float64) / cm
                h = np.cross(dn, e2)
                a = (e1 * h).sum(axis=1)
                good = np.abs(a) >= EPS
                f = 1.0 / np.where(good, a, 1.0)
                u = f * (sv * h).sum(axis=1)
                v = f * (qv * dn).sum(axis=1)
                t = f * t_num
                hit = good & ~((u < 0.0) | (u > 1.0)) & ~((v < 0.0) | (u + v > 1.0)) & (t > EPS)
                tmin = np.minimum.reduceat(np.where(hit, t, np.inf), first)
                q = tmin / (dx * cm)
                ok = np.isfinite(tmin) & (q > 0.0) & (q <= 1.0)
                qdense[k].reshape(-1)[ucell[ok]] = q[ok].astype(np.float16)
                any_hit |= ok
    q_map = np.zeros((BS, BS, BS, n, 27), dtype=np.float16, order="F")
    for kk in range(27):
        q_map[..., kk] = d.to_blocks(qdense[kk], n)
    mark = np.zeros(d.shape, dtype=bool)
    mark.reshape(-1)[ucell[any_hit]] = True
    arr = np.argwhere(d.to_blocks(mark, n))                 # (x, y, z, b) 0-based
    arr = arr[np.lexsort((arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3]))]
    return (q_map, (arr[:, 3] + 1).astype(np.int32), (arr[:, 0] + 1).astype(np.int8), (arr[:, 1] + 1).astype(np.int8),
            (arr[:, 2] + 1).astype(np.int8), int(arr.shape[0]))


# ----------------------------------------------------------------------------------------------------------------
# orchestration, src/domain.jl:20-266
# ----------------------------------------------------------------------------------------------------------------
@dataclass
class SetupReport:
    """The numbers the reference prints while it builds the domain (its only setup KATs)."""
    level_blocks: List[int] = field(default_factory=list)
    halo_blocks_added: List[Optional[int]] = field(default_factory=list)
    flood_fill_filled: List[int] = field(default_factory=list)
    sponge_fraction: List[float] = field(default_factory=list)
    sponge_max: List[float] = field(default_factory=list)
    near_wall_cells: List[int] = field(default_factory=list)
    bouzidi_cells: List[int] = field(default_factory=list)


def setup_multilevel_domain(cfg: CaseConfig, stl_path: Optional[str] = None, method: Optional[str] = None):
    """setup_multilevel_domain(stl_path) (src/domain.jl:268-280) -> (grids, mesh, params, report).
    method: "native" (default; libludwig_setup.so, threads over blocks) or "numpy" (the restatement the native code is checked
    against; env LUDWIG_SETUP_METHOD). There is no silent fall-back from one to the other."""
    method = method or os.environ.get("LUDWIG_SETUP_METHOD", "native")
    if method not in ("native", "numpy"):
        raise ValueError(f"setup method {method!r}: native or numpy")
    stl = stl_path or os.path.join(cfg.case_dir, cfg.stl_file)
    mesh = load_mesh(stl, scale=cfg.stl_scale)
    params = compute_domain_from_mesh(mesh.min_bounds, mesh.max_bounds, cfg)
    rep = SetupReport()
    off = params.mesh_offset
    pmin, pmax = params.mesh_min + off, params.mesh_max + off
    wake_start_x = pmax[0] - params.reference_length * 0.1
    wake_end_x = pmax[0] + params.reference_length * cfg.wake_length
    wcy, wcz = (pmin[1] + pmax[1]) / 2.0, (pmin[2] + pmax[2]) / 2.0
    ww, wh = (pmax[1] - pmin[1]) * cfg.wake_width_factor, (pmax[2] - pmin[2]) * cfg.wake_height_factor
    wy0, wy1, wz0, wz1 = wcy - ww / 2.0, wcy + ww / 2.0, wcz - wh / 2.0, wcz + wh / 2.0
    grids: List[BlockLevel] = []
    for lvl in range(1, params.num_levels + 1):
        scale = 2 ** (lvl - 1)
        dx = params.dx_coarse / scale
        bmax = (params.bx_max * scale, params.by_max * scale, params.bz_max * scale)
        active: Set[Coord] = set()
        if lvl == 1:
            active = {(bx, by, bz) for bz in range(1, bmax[2] + 1) for by in range(1, bmax[1] + 1) for bx in range(1, bmax[0] + 1)}
        else:
            prev = grids[-1]
            prev_bs = BS * params.dx_coarse / 2 ** (lvl - 2)
            if cfg.refinement_strategy == "geometry_first":
                active |= get_active_blocks_for_level(mesh, dx, off, bmax)
                if cfg.wake_enabled:
                    for (cbx, cby, cbz) in prev.active_block_coords:
                        ox = ((cbx - 1) * prev_bs <= wake_end_x) and (cbx * prev_bs >= wake_start_x)
                        oy = ((cby - 1) * prev_bs <= wy1) and (cby * prev_bs >= wy0)
                        oz = ((cbz - 1) * prev_bs <= wz1) and (cbz * prev_bs >= wz0)
                        if ox and oy and oz:
                            for db in range(8):
                                fb = (2 * cbx - 1 + (db & 1), 2 * cby - 1 + ((db >> 1) & 1), 2 * cbz - 1 + ((db >> 2) & 1))
                                if _inside(fb, bmax):
                                    active.add(fb)
                pset = set(prev.active_block_coords)
                active = {c for c in active if ((c[0] + 1) // 2, (c[1] + 1) // 2, (c[2] + 1) // 2) in pset}
            else:
                for b_idx, (cbx, cby, cbz) in enumerate(prev.active_block_coords):
                    if prev.obstacle[:, :, :, b_idx].any():
                        for db in range(8):
                            active.add((2 * cbx - 1 + (db & 1), 2 * cby - 1 + ((db >> 1) & 1), 2 * cbz - 1 + ((db >> 2) & 1)))
        n_before = len(active)
        add_halo_blocks_with_siblings(active, cfg.refinement_margin, bmax)
        ensure_complete_parent_coverage(active, bmax)
        rep.halo_blocks_added.append(len(active) - n_before if lvl > 1 else None)
        coords = sorted(active)
        table = build_neighbor_table(coords, *bmax)
        obstacle = voxelize_blocks(coords, mesh, dx, off, method=method)
        shell = obstacle.copy()
        rep.flood_fill_filled.append(perform_flood_fill(obstacle, coords, method=method))
        sponge = apply_sponge(coords, params, scale, cfg)
        rep.sponge_fraction.append(float((sponge > 0).mean()))
        rep.sponge_max.append(float(sponge.max()))
        wall = None
        if cfg.wall_model_enabled:
            wall = compute_wall_distances(coords, obstacle, dx, method=method)
            rep.near_wall_cells.append(int((wall != np.float32(100.0)).sum()))
        use_bouzidi = cfg.boundary_method == "bouzidi" and lvl > params.num_levels - cfg.bouzidi_levels
        kw = {}
        if use_bouzidi:
            q, cb, cx, cy, cz, nbc = compute_bouzidi_qmap_sparse(coords, mesh, dx, off, shell, method=method)
            kw = dict(bouzidi_q_map=q, bouzidi_cell_block=cb, bouzidi_cell_x=cx, bouzidi_cell_y=cy, bouzidi_cell_z=cz, n_boundary_cells=nbc)
            rep.bouzidi_cells.append(nbc)
        level = BlockLevel(lvl, coords, table, float(np.float32(dx)), np.float32(1.0) / np.float32(scale), params.tau_levels[lvl - 1],
                           enable_temporal_interpolation=cfg.temporal_interpolation, **kw)
        level.obstacle[...] = obstacle
        level.sponge[...] = sponge
        if wall is not None:
            level.wall_dist[...] = wall
        rep.level_blocks.append(len(coords))
        grids.append(level)
    return grids, mesh, params, rep


def solver_params(cfg: CaseConfig, params: DomainParameters) -> SolverParams:
    """the scalar arguments src/main.jl:176-180 passes to execute_timestep_batch!"""
    return SolverParams(domain_nx=params.nx_coarse, domain_ny=params.ny_coarse, domain_nz=params.nz_coarse,
                        wall_model_active=params.wall_model_active, c_wale=float(cfg.c_wale), nu_sgs_bg=float(cfg.nu_sgs_background),
                        inlet_turbulence=float(cfg.inlet_turbulence_intensity), use_temporal_interp=cfg.temporal_interpolation,
                        sponge_blend_dist=cfg.sponge_blend_distributions, symmetric_analysis=cfg.symmetric_analysis,
                        q_min_threshold=float(cfg.q_min_threshold))
