"""ctypes binding of libludwig_hip.so (include/ludwig_hip.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails, this module raises.
The product path never routes through oracle/ or any CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LUDWIG_HIP_LIB") or os.path.join(_HERE, "csrc", "libludwig_hip.so")   # override: diagnostics only

# enum LudwigField
F, F_TEMP, F_POST, F_OLD, RHO, RHO_OLD, VEL, VEL_TEMP, VEL_OLD, OBSTACLE, SPONGE, WALL_DIST = range(12)
FIELD_NAMES = {
    "f": F, "f_temp": F_TEMP, "f_post_collision": F_POST, "f_old": F_OLD, "rho": RHO, "rho_old": RHO_OLD,
    "vel": VEL, "vel_temp": VEL_TEMP, "vel_old": VEL_OLD, "obstacle": OBSTACLE, "sponge": SPONGE,
    "wall_dist": WALL_DIST,
}
# enum LudwigStat: accumulated statistic -> (id, components)
STAT_RHO, STAT_VEL, STAT_VEL2 = range(3)
STAT_NAMES = {"rho": (STAT_RHO, 1), "vel": (STAT_VEL, 3), "vel2": (STAT_VEL2, 6)}
# enum LudwigGradField: velocity-gradient field -> (id, components)
GRAD_VORTICITY, GRAD_Q = range(2)
GRAD_NAMES = {"vorticity": (GRAD_VORTICITY, 3), "q": (GRAD_Q, 1)}
# ludwig_slices_create flags
SLICE_GRADIENT = 1
# enum LudwigIsoScalar (isosurface.FIELDS, in this order) and the status of an extraction refused by its cap (no error)
ISO_NAMES = {"density": 0, "velocity_magnitude": 1, "q_criterion": 2, "vorticity_magnitude": 3}
ISO_REFUSED = 1
# enum LudwigSubgridField / LudwigSubgridSum: one component each
SUBGRID_FIELD_NAMES = {"nu": 0, "code": 1}
SUBGRID_SUM_NAMES = {"nu": 0, "nunu": 1, "eps": 2}
# enum LudwigPart
PART_ALL, PART_BOUNDARY, PART_INTERIOR = 0, 1, 2

# LUDWIG_OBSERVE_*: the kind of a BatchObserver entry
OBSERVE_PROBES, OBSERVE_SURFACE, OBSERVE_FORCES, OBSERVE_TRACERS, OBSERVE_FLUXES = range(5)
OBSERVE_MODES = 5

# every symbol include/ludwig_hip.h declares (tests check the .so exports exactly these)
EXPORTED_SYMBOLS = [
    "ludwig_abi_version", "ludwig_last_error", "ludwig_device_count",
    "ludwig_level_create", "ludwig_level_destroy", "ludwig_level_set_stream", "ludwig_level_add_post_collision_readers", "ludwig_level_set_order",
    "ludwig_level_upload", "ludwig_level_download", "ludwig_level_field_ptr",
    "ludwig_init_equilibrium", "ludwig_step", "ludwig_stream_collide", "ludwig_bouzidi_correction",
    "ludwig_save_old", "ludwig_execute_timestep_batch", "ludwig_execute_timestep_batch_observed", "ludwig_sync", "ludwig_halo_pack", "ludwig_halo_unpack", "ludwig_level_info",
    "ludwig_map_surface_stresses", "ludwig_level_rho_min", "ludwig_level_block_order",
    "ludwig_stream_create", "ludwig_stream_destroy", "ludwig_level_field_layout", "ludwig_level_set_rho_store",
    "ludwig_comm_unique_id", "ludwig_comm_create", "ludwig_comm_destroy", "ludwig_comm_allreduce_f32",
    "ludwig_halo_plan_create", "ludwig_halo_plan_destroy", "ludwig_halo_exchange", "ludwig_halo_wait",
    "ludwig_halo_plan_pack", "ludwig_halo_plan_unpack", "ludwig_halo_plan_buffers", "ludwig_halo_plan_timing", "ludwig_halo_plan_in_stream",
    "ludwig_halo_plan_exchange_ms", "ludwig_step_distributed",
    "ludwig_level_stats_reset", "ludwig_level_stats_accumulate", "ludwig_level_stats_download",
    "ludwig_level_gradient_fields_compute", "ludwig_level_gradient_fields_download",
    "ludwig_level_subgrid_fields_compute", "ludwig_level_subgrid_fields_download", "ludwig_level_subgrid_stats_reset",
    "ludwig_level_subgrid_stats_accumulate", "ludwig_level_subgrid_stats_download",
    "ludwig_probes_create", "ludwig_probes_destroy", "ludwig_probes_sample", "ludwig_probes_download",
    "ludwig_execute_timestep_batch_probes",
    "ludwig_surface_stats_create", "ludwig_surface_stats_destroy", "ludwig_surface_stats_reset", "ludwig_surface_stats_accumulate",
    "ludwig_surface_stats_download", "ludwig_execute_timestep_batch_sampled",
    "ludwig_slices_create", "ludwig_slices_destroy", "ludwig_slices_sample", "ludwig_slices_download",
    "ludwig_streamlines_create", "ludwig_streamlines_destroy", "ludwig_streamlines_trace", "ludwig_streamlines_download",
    "ludwig_render_create", "ludwig_render_destroy", "ludwig_render_image", "ludwig_render_download",
    "ludwig_tracers_create", "ludwig_tracers_destroy", "ludwig_tracers_advance", "ludwig_tracers_snapshot", "ludwig_tracers_download",
    "ludwig_execute_timestep_batch_tracers",
    "ludwig_level_monitor",
    "ludwig_level_isosurface_extract", "ludwig_level_isosurface_download",
    "ludwig_level_wall_census", "ludwig_wall_surface_create", "ludwig_wall_surface_destroy", "ludwig_wall_surface_compute",
    "ludwig_wall_surface_download",
    "ludwig_force_series_create", "ludwig_force_series_destroy", "ludwig_force_series_sample", "ludwig_force_series_download",
    "ludwig_execute_timestep_batch_loads",
    "ludwig_flux_planes_create", "ludwig_flux_planes_destroy", "ludwig_flux_planes_sample", "ludwig_flux_planes_download",
    "ludwig_modes_create", "ludwig_modes_destroy", "ludwig_modes_reset", "ludwig_modes_accumulate", "ludwig_modes_download",
    "ludwig_record_step_rule", "ludwig_level_record_steps",
    "ludwig_flow_source_create", "ludwig_flow_source_from_levels", "ludwig_flow_source_destroy", "ludwig_level_init_from_source",
]
UNIQUE_ID_BYTES = 128
HALO_GROUPS = ("f", "vel", "f_post", "rho")      # group index of partition.FIELD_GROUPS in a LudwigHaloPlanDesc


class LudwigError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libludwig_hip error {code}: {msg}")
        self.code = code


class LevelHost(C.Structure):
    _fields_ = [
        ("level_id", C.c_int32), ("n_blocks", C.c_int32), ("n_owned", C.c_int32), ("tau", C.c_float),
        ("grid_dim_x", C.c_int32), ("grid_dim_y", C.c_int32), ("grid_dim_z", C.c_int32),
        ("block_pointer", C.c_void_p), ("neighbor_table", C.c_void_p),
        ("map_x", C.c_void_p), ("map_y", C.c_void_p), ("map_z", C.c_void_p),
        ("obstacle", C.c_void_p), ("sponge", C.c_void_p), ("wall_dist", C.c_void_p),
        ("enable_temporal_interpolation", C.c_int32), ("n_boundary_cells", C.c_int32),
        ("bouzidi_q_map", C.c_void_p), ("bouzidi_cell_block", C.c_void_p),
        ("bouzidi_cell_x", C.c_void_p), ("bouzidi_cell_y", C.c_void_p), ("bouzidi_cell_z", C.c_void_p),
        ("comm_boundary", C.c_void_p), ("store_post_collision_everywhere", C.c_int32),
    ]


class StepFlags(C.Structure):
    _fields_ = [
        ("domain_nx", C.c_int32), ("domain_ny", C.c_int32), ("domain_nz", C.c_int32),
        ("is_symmetric", C.c_int32), ("wall_model_active", C.c_int32), ("use_temporal_interp", C.c_int32),
        ("sponge_blend_distributions", C.c_int32),
        ("c_wale", C.c_float), ("nu_sgs_background", C.c_float), ("inlet_turbulence", C.c_float),
        ("q_min_threshold", C.c_float),
    ]


class SurfaceParams(C.Structure):
    _fields_ = [
        ("dx", C.c_float), ("tau", C.c_float), ("offset_x", C.c_float), ("offset_y", C.c_float), ("offset_z", C.c_float),
        ("pressure_scale", C.c_float), ("stress_scale", C.c_float), ("search_radius", C.c_int32),
    ]


class BatchObserver(C.Structure):
    _fields_ = [("kind", C.c_int32), ("set", C.c_void_p), ("start_step", C.c_int64), ("interval", C.c_int32)]


class BatchSamplers(C.Structure):
    _fields_ = [
        ("probes", C.c_void_p), ("probes_start_step", C.c_int64), ("probes_interval", C.c_int32),
        ("surface", C.c_void_p), ("surface_start_step", C.c_int64), ("surface_interval", C.c_int32),
    ]


WALL_BINS = 194


class WallCensus(C.Structure):
    _fields_ = [
        ("near_cells", C.c_uint64), ("evaluated", C.c_uint64), ("log_law", C.c_uint64), ("forced", C.c_uint64),
        ("non_finite", C.c_uint64), ("min_bits", C.c_uint32), ("max_bits", C.c_uint32), ("hist", C.c_uint64 * WALL_BINS),
    ]


class HaloPlanDesc(C.Structure):
    _fields_ = [
        ("n_peers", C.c_int32), ("peer_ranks", C.c_void_p),
        ("send_count", C.c_void_p * 4), ("recv_count", C.c_void_p * 4),
        ("send_index", C.c_void_p * 4), ("recv_index", C.c_void_p * 4),
    ]


class LevelInfo(C.Structure):
    _fields_ = [
        ("n_blocks", C.c_int32), ("n_owned", C.c_int32), ("n_fast_blocks", C.c_int32),
        ("n_general_blocks", C.c_int32), ("n_boundary_cells", C.c_int32),
        ("has_temporal_storage", C.c_int32), ("has_post_collision", C.c_int32), ("n_xrun_blocks", C.c_int32),
        ("device_bytes", C.c_int64),
    ]


_lib = None


def load() -> C.CDLL:
    """Load libludwig_hip.so; raises if it has not been built (run `python __graft_entry__.py` / build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
    sig = {
        "ludwig_abi_version": (C.c_int, []),
        "ludwig_last_error": (C.c_char_p, []),
        "ludwig_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "ludwig_level_create": (C.c_int, [C.POINTER(LevelHost), i32, C.POINTER(vp)]),
        "ludwig_level_destroy": (None, [vp]),
        "ludwig_level_set_stream": (C.c_int, [vp, vp]),
        "ludwig_level_add_post_collision_readers": (C.c_int, [vp, vp, i64]),
        "ludwig_level_set_order": (C.c_int, [vp, i32, vp, i64]),
        "ludwig_level_upload": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "ludwig_level_download": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "ludwig_level_field_ptr": (C.c_int, [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "ludwig_init_equilibrium": (C.c_int, [vp]),
        "ludwig_step": (C.c_int, [vp, vp, i64, f32, f32, f32, C.POINTER(StepFlags)]),
        "ludwig_stream_collide": (C.c_int, [vp, vp, i64, f32, f32, f32, C.POINTER(StepFlags), i32]),
        "ludwig_bouzidi_correction": (C.c_int, [vp, i64, f32]),
        "ludwig_save_old": (C.c_int, [vp, i64]),
        "ludwig_execute_timestep_batch": (C.c_int, [C.POINTER(vp), i32, i64, i32, f32, C.POINTER(StepFlags)]),
        "ludwig_execute_timestep_batch_observed": (C.c_int, [C.POINTER(vp), i32, i64, i32, f32, C.POINTER(StepFlags),
                                                             C.POINTER(BatchObserver), i32]),
        "ludwig_sync": (C.c_int, [vp]),
        "ludwig_halo_pack": (C.c_int, [vp, i32, vp, i64, vp, vp]),
        "ludwig_halo_unpack": (C.c_int, [vp, i32, vp, i64, vp, vp]),
        "ludwig_map_surface_stresses": (C.c_int, [vp, i32, i32, vp, vp, C.POINTER(SurfaceParams), vp, vp, vp, vp]),
        "ludwig_level_info": (C.c_int, [vp, C.POINTER(LevelInfo)]),
        "ludwig_level_rho_min": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "ludwig_level_block_order": (C.c_int, [vp, vp]),
        "ludwig_stream_create": (C.c_int, [i32, i32, C.POINTER(vp)]),
        "ludwig_stream_destroy": (C.c_int, [i32, vp]),
        "ludwig_level_field_layout": (C.c_int, [vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "ludwig_level_set_rho_store": (C.c_int, [vp, i32]),
        "ludwig_record_step_rule": (C.c_int, [vp, i32, i32, i32, i32, i32, i32]),
        "ludwig_level_record_steps": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "ludwig_comm_unique_id": (C.c_int, [vp]),
        "ludwig_comm_create": (C.c_int, [vp, i32, i32, i32, C.POINTER(vp)]),
        "ludwig_comm_destroy": (None, [vp]),
        "ludwig_comm_allreduce_f32": (C.c_int, [vp, vp, i32, i32]),
        "ludwig_halo_plan_create": (C.c_int, [vp, vp, C.POINTER(HaloPlanDesc), C.POINTER(vp)]),
        "ludwig_halo_plan_destroy": (None, [vp]),
        "ludwig_halo_exchange": (C.c_int, [vp, i32, vp, vp]),
        "ludwig_halo_wait": (C.c_int, [vp]),
        "ludwig_halo_plan_pack": (C.c_int, [vp, i32, i32, vp]),
        "ludwig_halo_plan_unpack": (C.c_int, [vp, i32, i32, vp]),
        "ludwig_halo_plan_buffers": (C.c_int, [vp, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i64)]),
        "ludwig_halo_plan_timing": (C.c_int, [vp, i32]),
        "ludwig_halo_plan_in_stream": (C.c_int, [vp, i32]),
        "ludwig_halo_plan_exchange_ms": (C.c_int, [vp, vp, i32, C.POINTER(C.c_int32)]),
        "ludwig_step_distributed": (C.c_int, [vp, vp, vp, i64, f32, f32, f32, C.POINTER(StepFlags)]),
        "ludwig_level_stats_reset": (C.c_int, [vp]),
        "ludwig_level_stats_accumulate": (C.c_int, [vp, i64]),
        "ludwig_level_monitor": (C.c_int, [vp, i64, vp, vp, vp, vp]),
        "ludwig_level_stats_download": (C.c_int, [vp, i32, vp, C.c_size_t, C.POINTER(C.c_int64)]),
        "ludwig_level_gradient_fields_compute": (C.c_int, [vp, i32, f32]),
        "ludwig_level_gradient_fields_download": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "ludwig_level_subgrid_fields_compute": (C.c_int, [vp, i32]),
        "ludwig_level_subgrid_fields_download": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "ludwig_level_subgrid_stats_reset": (C.c_int, [vp]),
        "ludwig_level_subgrid_stats_accumulate": (C.c_int, [vp, i64]),
        "ludwig_level_subgrid_stats_download": (C.c_int, [vp, i32, vp, C.c_size_t, C.POINTER(C.c_int64)]),
        "ludwig_probes_create": (C.c_int, [C.POINTER(vp), i32, i32, vp, vp, vp, vp, i32, C.POINTER(vp)]),
        "ludwig_probes_destroy": (None, [vp]),
        "ludwig_probes_sample": (C.c_int, [vp, i32, i64]),
        "ludwig_probes_download": (C.c_int, [vp, vp, vp, i32, C.POINTER(C.c_int32)]),
        "ludwig_execute_timestep_batch_probes": (C.c_int, [C.POINTER(vp), i32, i64, i32, f32, C.POINTER(StepFlags), vp, i64, i32]),
        "ludwig_surface_stats_create": (C.c_int, [vp, i32, vp, vp, vp, vp, C.POINTER(SurfaceParams), C.POINTER(vp)]),
        "ludwig_surface_stats_destroy": (None, [vp]),
        "ludwig_surface_stats_reset": (C.c_int, [vp]),
        "ludwig_surface_stats_accumulate": (C.c_int, [vp, i64]),
        "ludwig_surface_stats_download": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_int64)]),
        "ludwig_execute_timestep_batch_sampled": (C.c_int, [C.POINTER(vp), i32, i64, i32, f32, C.POINTER(StepFlags), C.POINTER(BatchSamplers)]),
        "ludwig_slices_create": (C.c_int, [C.POINTER(vp), i32, i32, vp, vp, vp, vp, vp, vp, i32, C.POINTER(vp)]),
        "ludwig_slices_destroy": (None, [vp]),
        "ludwig_slices_sample": (C.c_int, [vp, i64]),
        "ludwig_slices_download": (C.c_int, [vp, vp, C.c_size_t]),
        "ludwig_streamlines_create": (C.c_int, [vp, i32, i32, vp, vp, f32, f32, i32, C.POINTER(vp)]),
        "ludwig_streamlines_destroy": (None, [vp]),
        "ludwig_streamlines_trace": (C.c_int, [vp, i64]),
        "ludwig_streamlines_download": (C.c_int, [vp, vp, vp, vp, C.c_size_t]),
        "ludwig_render_create": (C.c_int, [vp, i32, i64, C.POINTER(vp)]),
        "ludwig_render_destroy": (None, [vp]),
        "ludwig_render_image": (C.c_int, [vp, i64, i32, vp, vp, i32, i32, i32, vp, i32, vp]),
        "ludwig_render_download": (C.c_int, [vp, vp, vp, vp, C.c_size_t]),
        "ludwig_tracers_create": (C.c_int, [vp, i32, i32, vp, i32, i32, f32, C.POINTER(vp)]),
        "ludwig_tracers_destroy": (None, [vp]),
        "ludwig_tracers_advance": (C.c_int, [vp, i64]),
        "ludwig_tracers_snapshot": (C.c_int, [vp, i64]),
        "ludwig_tracers_download": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_int64)]),
        "ludwig_level_isosurface_extract": (C.c_int, [vp, i32, i32, f32, f32, vp, vp, vp, i64, C.POINTER(C.c_int64)]),
        "ludwig_level_isosurface_download": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t]),
        "ludwig_level_wall_census": (C.c_int, [vp, i64, C.POINTER(WallCensus)]),
        "ludwig_wall_surface_create": (C.c_int, [vp, i32, vp, vp, vp, C.POINTER(SurfaceParams), C.POINTER(vp)]),
        "ludwig_wall_surface_destroy": (None, [vp]),
        "ludwig_wall_surface_compute": (C.c_int, [vp, i64]),
        "ludwig_wall_surface_download": (C.c_int, [vp, vp, C.c_size_t]),
        "ludwig_force_series_create": (C.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, C.POINTER(SurfaceParams), i32, C.POINTER(vp)]),
        "ludwig_force_series_destroy": (None, [vp]),
        "ludwig_force_series_sample": (C.c_int, [vp, i64, i64]),
        "ludwig_force_series_download": (C.c_int, [vp, vp, vp, vp, i32, C.POINTER(C.c_int32)]),
        "ludwig_execute_timestep_batch_loads": (C.c_int, [C.POINTER(vp), i32, i64, i32, f32, C.POINTER(StepFlags), C.POINTER(BatchSamplers),
                                                          vp, i64, i32]),
        "ludwig_flux_planes_create": (C.c_int, [C.POINTER(vp), i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(vp)]),
        "ludwig_flux_planes_destroy": (None, [vp]),
        "ludwig_flux_planes_sample": (C.c_int, [vp, i64]),
        "ludwig_flux_planes_download": (C.c_int, [vp, vp, vp, vp, i32, C.POINTER(C.c_int32)]),
        "ludwig_modes_create": (C.c_int, [C.POINTER(vp), i32, i32, i32, vp, C.POINTER(vp)]),
        "ludwig_modes_destroy": (None, [vp]),
        "ludwig_modes_reset": (C.c_int, [vp]),
        "ludwig_modes_accumulate": (C.c_int, [vp, i32, i64, i32]),
        "ludwig_modes_download": (C.c_int, [vp, i32, i32, vp, C.c_size_t, C.POINTER(C.c_int32)]),
        "ludwig_execute_timestep_batch_tracers": (C.c_int, [C.POINTER(vp), i32, i64, i32, f32, C.POINTER(StepFlags), C.POINTER(BatchSamplers),
                                                            vp, i64, i32, vp, i64, i32]),
        "ludwig_flow_source_create": (C.c_int, [i32, i32, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
        "ludwig_flow_source_from_levels": (C.c_int, [C.POINTER(vp), i32, i64, C.POINTER(vp)]),
        "ludwig_flow_source_destroy": (None, [vp]),
        "ludwig_level_init_from_source": (C.c_int, [vp, vp, vp, f32, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)   # AttributeError if the .so does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    if lib.ludwig_abi_version() != 1:
        raise RuntimeError("libludwig_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().ludwig_last_error()
        raise LudwigError(rc, msg.decode("utf-8", "replace") if msg else "")


class Handle:
    """An object of the library behind a ctypes handle `_h`, made by the subclass's constructor (which also sets `_lib`): `handle`
    raises once it is closed, close() destroys it once, and a failing __del__ stays silent."""
    _destroy = ""       # the library's destroy function
    _closed = ""        # what `handle` raises after close()
    _h = None

    @property
    def handle(self):
        if not self._h:                        # None, or a NULL c_void_p
            raise RuntimeError(self._closed)
        return self._h

    def close(self) -> None:
        if self._h:
            getattr(self._lib, self._destroy)(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ModeSet(Handle):
    """ludwig_modes_*: running sums of rho and u per cell times the rows of a weight table W [n_rows, n_columns] (Float64), over every
    level of `levels` (DeviceLevel). start_step / interval: the coarse steps a batch samples, and what row_of() counts rows from."""
    _destroy, _closed = "ludwig_modes_destroy", "mode set closed"

    def __init__(self, levels, W, start_step: int = 1, interval: int = 1):
        import numpy as np
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2:
            raise ValueError(f"modes: the weight table must be [n_rows, n_columns], got shape {W.shape}")
        if int(interval) < 1:
            raise ValueError(f"modes: interval {interval} < 1")
        self._lib = load()
        self.levels = list(levels)
        self.W = W
        self.n_rows, self.n_columns = int(W.shape[0]), int(W.shape[1])
        self.start_step, self.interval = int(start_step), int(interval)
        arr = (C.c_void_p * len(self.levels))(*[(lv.handle if lv is not None else None) for lv in self.levels])
        h = C.c_void_p()
        check(self._lib.ludwig_modes_create(arr, len(self.levels), self.n_columns, self.n_rows, W.ctypes.data, C.byref(h)))
        self._h = h

    def row_of(self, t_coarse: int) -> int:
        return ((int(t_coarse) - self.start_step) // self.interval) % self.n_rows

    def reset(self) -> None:
        check(self._lib.ludwig_modes_reset(self.handle))

    def accumulate(self, level_index: int, t_sub: int, row: int) -> None:
        """one sample of a level after its sub-step t_sub with table row `row` (queued on the level's stream)"""
        check(self._lib.ludwig_modes_accumulate(self.handle, int(level_index), int(t_sub), int(row)))

    def download(self, level_index: int, column: int):
        """(Float64 sums [8,8,8,n_blocks,4] of one column in the reference layout: rho, ux, uy, uz; samples); ghost blocks are 0"""
        import numpy as np
        a = np.empty((8, 8, 8, self.levels[level_index].n_blocks, 4), dtype=np.float64, order="F")
        n = C.c_int32(0)
        check(self._lib.ludwig_modes_download(self.handle, int(level_index), int(column), a.ctypes.data if a.size else None, a.nbytes,
                                              C.byref(n)))
        return a, int(n.value)


def device_count() -> int:
    n = C.c_int(0)
    rc = load().ludwig_device_count(C.byref(n))
    return n.value if rc == 0 else 0
