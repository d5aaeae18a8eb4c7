"""Flux planes: integrals of mass, momentum, pressure and kinetic-energy flux over axis-aligned planes and boxes at every sampled
coarse step, reduced on the device inside the batches (no reference counterpart).

Semantics ("Flux planes"; include/ludwig_hip.h states the same, and host_record below restates the kernels bit for
bit):
  * Planes. A flux plane (preprocess.FluxPlane) is a slice plane plus direction = +1 or -1: name, normal axis n, position, optional
    bounds, optional spacing h, in the STL frame after stl_scale. A box (preprocess.FluxBox) is six such planes <name>_xmin .. _zmax
    with outward directions.
  * Points are CELL-CENTRED, so that the midpoint rule covers the bounds (slices put points on the bounds): along each in-plane axis
    max(1, floor((hi - lo) / h)) points at lo + (i + 0.5) h, float64, point index i + n_a j. Defaults as for slices: bounds = the
    whole domain, h = dx of the finest level; at most SLICE_MAX_POINTS per plane; a plane outside the domain is refused when planned.
  * Sampling. Level, corners, weights, replaced corners and validity of every point come from slices.plan_points unchanged (the
    probes' rule). Invalid points - outside the domain, held by no level, obstacle base cell - take no part. The sample of a valid
    point is rho, ux, uy, uz by probes.trilinear in float32, read from the level's newest state after the coarse step
    (statistics.t_sub_after: vel_temp after an even sub-step, vel after an odd one).
  * Integrands per valid point, float32, in exactly this operand order: un = u[n] (along the +axis; the direction is applied later),
    m = rho * un, q = (ux*ux + uy*uy) + uz*uz, and the eight rows ROWS = rho, un, m, m*ux, m*uy, m*uz, rho*q, m*q.
  * Reduction. For every (plane, level) pair: the valid points of the plane on that level in point order, every row widened to
    float64 and summed by forces.tree_sum_f64 (adjacent pairs halved, +0.0 appended where a length is odd), and an int64 count. A
    plane's record is the float64 left-to-right sum of its per-level records from the coarsest level to the finest, skipping levels
    that hold none of its points; counts add as integers; no valid point: +0.0 and 0. The per-level split is deliberate: every level
    reduces its own points on its own stream, so no level waits for another.
  * The area element h^2, the direction and all physical scales are applied here, in float64 (plane_quantities, box_quantities).
  * Sampled coarse steps: start_step + k interval. Records wait in a device ring of `capacity` samples until they are downloaded.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Sequence, Tuple

import numpy as np

from . import forces as forces_mod
from ._lib import Handle
from .force_series import Series as _Series, segment_end       # noqa: F401  (one ring rule for every in-batch series)
from .preprocess import SLICE_MAX_POINTS, FluxBox, FluxPlane
from .probes import gather, trilinear
from .slices import _extent, plan_points
from .statistics import is_sample_step, t_sub_after

F32 = np.float32
ROWS = ("rho", "un", "m", "m_ux", "m_uy", "m_uz", "rho_q", "m_q")
N_ROWS = len(ROWS)


@dataclass
class FluxPlan:
    spec: FluxPlane
    axes: Tuple[int, int]           # in-plane axes a < b
    spacing: float                  # h
    dims: Tuple[int, int]           # points along a, b
    points: np.ndarray              # [n, 3] float64, STL frame
    domain: np.ndarray              # [n, 3] float64, domain frame
    valid: np.ndarray               # [n] bool
    level: np.ndarray               # [n] int32 (0 where invalid)
    blocks: np.ndarray              # [n, 8] int32, reference block index of every corner (0 where invalid)
    cells: np.ndarray               # [n, 8] int32, x + 8 y + 64 z
    weights: np.ndarray             # [n, 3] float32
    replaced: np.ndarray            # [n, 8] bool

    @property
    def n(self) -> int:
        return self.points.shape[0]

    def lists(self) -> List[Tuple[int, np.ndarray]]:
        """(level index, point indices in point order) of every level that holds valid points, coarsest first"""
        return [(int(li), np.flatnonzero(self.valid & (self.level == li))) for li in np.unique(self.level[self.valid])]


def flux_axis_points(lo: float, hi: float, h: float) -> int:
    """cells along one in-plane axis: max(1, floor((hi - lo) / h))"""
    return max(1, int(math.floor((hi - lo) / h)))


def flux_grid(spec: FluxPlane, grids: Sequence, offset=(0.0, 0.0, 0.0)):
    """(in-plane axes, spacing, dims, points [n, 3] float64 in the STL frame) of a flux plane; ValueError for a plane wholly outside
    the domain or with more than SLICE_MAX_POINTS points"""
    off = np.asarray(offset, dtype=np.float64).reshape(3)
    lo, hi = -off, _extent(grids) - off                      # the domain in the STL frame
    nrm = int(spec.normal)
    axes = tuple(a for a in range(3) if a != nrm)
    h = float(spec.spacing) if spec.spacing is not None else float(grids[-1].dx)
    bounds = spec.bounds if spec.bounds is not None else tuple((float(lo[a]), float(hi[a])) for a in axes)
    where = f"flux plane {spec.name!r}"
    if not lo[nrm] <= spec.position <= hi[nrm]:
        raise ValueError(f"{where}: position {spec.position} lies outside the domain [{lo[nrm]}, {hi[nrm]}] along {'xyz'[nrm]}")
    for (b0, b1), a in zip(bounds, axes):
        if b1 < lo[a] or b0 > hi[a]:
            raise ValueError(f"{where}: bounds [{b0}, {b1}] along {'xyz'[a]} miss the domain [{lo[a]}, {hi[a]}]")
    dims = tuple(flux_axis_points(b0, b1, h) for b0, b1 in bounds)
    if dims[0] * dims[1] > SLICE_MAX_POINTS:
        raise ValueError(f"{where}: {dims[0]} x {dims[1]} points, more than {SLICE_MAX_POINTS} per plane")
    ca = bounds[0][0] + (np.arange(dims[0], dtype=np.float64) + 0.5) * h
    cb = bounds[1][0] + (np.arange(dims[1], dtype=np.float64) + 0.5) * h
    pts = np.empty((dims[0] * dims[1], 3), dtype=np.float64)
    pts[:, axes[0]] = np.tile(ca, dims[1])                   # i fastest
    pts[:, axes[1]] = np.repeat(cb, dims[0])
    pts[:, nrm] = float(spec.position)
    return axes, h, dims, pts


def plan_flux_plane(spec: FluxPlane, grids: Sequence, offset=(0.0, 0.0, 0.0)) -> FluxPlan:
    """the plan of one plane over `grids` (host BlockLevels, level 1 first); offset = params.mesh_offset"""
    axes, h, dims, pts = flux_grid(spec, grids, offset)
    dom, valid, level, blocks, cells, weights, replaced = plan_points(pts, grids, offset)
    return FluxPlan(spec, axes, h, dims, pts, dom, valid, level, blocks, cells, weights, replaced)


# ---- the numpy restatement of k_flux_chunks / k_flux_combine (kernels.hpp stencil_sample, flux_contributions, tree_leaf, tree_combine)
# and of the download's sum over levels ----
def contributions(plan: FluxPlan, idx: np.ndarray, rho: np.ndarray, vel: np.ndarray) -> np.ndarray:
    """[len(idx), 8] float32: the rows of points idx of one level from its fields in the reference layout"""
    s = trilinear(gather(plan, idx, rho, vel), plan.weights[idx][:, None, :])      # [m, 4]: rho, ux, uy, uz
    r, ux, uy, uz = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    un = s[:, 1 + int(plan.spec.normal)]
    m = r * un
    q = (ux * ux + uy * uy) + uz * uz
    return np.stack([r, un, m, m * ux, m * uy, m * uz, r * q, m * q], axis=1).astype(F32)


def list_record(contrib: np.ndarray) -> np.ndarray:
    """float64 [8]: one (plane, level) record of float32 contributions [n, 8]"""
    c = np.asarray(contrib, dtype=F32).astype(np.float64).reshape(-1, N_ROWS)
    return np.array([forces_mod.tree_sum_f64(c[:, k]) for k in range(N_ROWS)], dtype=np.float64)


def host_record(plan: FluxPlan, fields: Callable[[int], Tuple[np.ndarray, np.ndarray]]) -> Tuple[np.ndarray, int]:
    """(sums [8] float64, count) of a plane; fields(level index) -> (rho, newest velocity buffer) of that level"""
    sums, count = np.zeros(N_ROWS, dtype=np.float64), 0
    for k, (li, idx) in enumerate(plan.lists()):
        rho, vel = fields(li)
        rec = list_record(contributions(plan, idx, rho, vel))
        sums = rec if k == 0 else sums + rec
        count += int(idx.size)
    return sums, count


def host_sample(stepper, plans: Sequence[FluxPlan], t_coarse: int) -> Tuple[np.ndarray, np.ndarray]:
    """(sums [n_planes, 8] float64, counts [n_planes] int64) after coarse step t_coarse from a stepper's downloaded fields (a stepper
    without flux_planes_setup, e.g. the CPU oracle)"""
    cache: Dict[int, Tuple] = {}

    def fields(li):
        if li not in cache:
            cache[li] = (stepper.field(li, "rho"), stepper.field(li, "vel_temp" if t_sub_after(li, t_coarse) % 2 == 0 else "vel"))
        return cache[li]
    sums = np.zeros((len(plans), N_ROWS), dtype=np.float64)
    counts = np.zeros(len(plans), dtype=np.int64)
    for k, p in enumerate(plans):
        sums[k], counts[k] = host_record(p, fields)
    return sums, counts


class Series(_Series):
    """the host copy of a flux series: per sample [n_planes, 8] float64 sums and [n_planes] int64 counts"""

    def __init__(self, n_planes: int):
        super().__init__((int(n_planes), N_ROWS), (int(n_planes),))


# ---- the device set (ludwig_flux_planes_*) ----
class DeviceFluxPlanes(Handle):
    """one device set over every plane of `plans` on device levels (DeviceLevel, or None for a level no point is on); the plans'
    blocks are the levels' own (reference-order) block indices"""
    _destroy, _closed = "ludwig_flux_planes_destroy", "flux plane set closed"

    def __init__(self, plans: Sequence[FluxPlan], levels: Sequence, capacity: int = 64, start_step: int = 1, interval: int = 1):
        from . import _lib
        if int(interval) < 1:
            raise ValueError(f"flux planes: interval {interval} < 1")
        if int(capacity) < 1:
            raise ValueError(f"flux planes: capacity {capacity} < 1")
        self._lib = _lib.load()
        self.n_planes, self.capacity = len(plans), int(capacity)
        self.start_step, self.interval = int(start_step), int(interval)      # the coarse steps a batch samples
        arr = (C.c_void_p * len(levels))(*[(lv.handle if lv is not None else None) for lv in levels])

        def cat(name, dt, tail):
            parts = [np.asarray(getattr(p, name)).reshape((-1,) + tail) for p in plans]
            return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0,) + tail), dtype=dt)
        start = np.ascontiguousarray(np.cumsum([0] + [p.n for p in plans]), dtype=np.int32)
        normal = np.ascontiguousarray([int(p.spec.normal) for p in plans], dtype=np.int32)
        li, bl, ce = cat("level", np.int32, ()), cat("blocks", np.int32, (8,)), cat("cells", np.int32, (8,))
        w, va = cat("weights", np.float32, (3,)), cat("valid", np.uint8, ())
        h = C.c_void_p()
        _lib.check(self._lib.ludwig_flux_planes_create(arr, len(levels), self.n_planes, start.ctypes.data, normal.ctypes.data,
                                                       li.ctypes.data, bl.ctypes.data, ce.ctypes.data, w.ctypes.data, va.ctypes.data,
                                                       self.capacity, C.byref(h)))
        self._h = h

    def is_sample_step(self, t: int) -> bool:
        return is_sample_step(t, self.start_step, self.interval)

    def sample(self, t_coarse: int) -> None:
        """between batches: one ring slot of the state after coarse step t_coarse"""
        from . import _lib
        _lib.check(self._lib.ludwig_flux_planes_sample(self.handle, int(t_coarse)))

    def download(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(coarse steps [n] int64, sums [n, n_planes, 8] float64, counts [n, n_planes] int64) taken since the last download; empties
        the ring"""
        from . import _lib
        sums = np.empty((self.capacity, self.n_planes, N_ROWS), dtype=np.float64)
        counts = np.empty((self.capacity, self.n_planes), dtype=np.int64)
        steps = np.empty(self.capacity, dtype=np.int64)
        n = C.c_int32(0)
        _lib.check(self._lib.ludwig_flux_planes_download(self.handle, sums.ctypes.data, counts.ctypes.data, steps.ctypes.data,
                                                         self.capacity, C.byref(n)))
        return steps[: n.value].copy(), sums[: n.value].copy(), counts[: n.value].copy()


# ---- physical quantities (float64) ----
@dataclass
class PlaneFlux:
    mass_flow: float                # [kg/s], signed by direction
    volume_flow: float              # [m^3/s], signed by direction
    momentum: Tuple[float, float, float]    # [N], signed by direction
    mean_pressure: float            # [Pa], gauge; 0 without a valid point
    pressure_force: float           # [N], mean gauge pressure x valid area, along the +axis
    kinetic_energy_flux: float      # [W], signed by direction
    area: float                     # [m^2] of the valid points
    count: int


def plane_quantities(plan: FluxPlan, sums, count: int, params) -> PlaneFlux:
    """a record in physical units. With A = h^2, d = direction, rho0 = rho_physical, c = velocity_scale:
    mass flow = d rho0 c A sum(m); volume flow = d c A sum(un); momentum flux_j = d rho0 c^2 A sum(m u_j);
    pressure p = (rho - 1) / 3 in lattice units, scaled by rho0 c^2 as forces.stress_from_cells does: pressure force =
    rho0 c^2 A (sum(rho) - count) / 3, mean pressure = that over count A; kinetic-energy flux = d rho0 c^3 A sum(m q) / 2"""
    s = [float(v) for v in sums]
    A, d = float(plan.spacing) ** 2, float(plan.spec.direction)
    rho0, c = float(params.rho_physical), float(params.velocity_scale)
    ps = rho0 * c * c
    pf = ps * A * ((s[0] - float(count)) / 3.0)
    area = float(count) * A
    return PlaneFlux(d * rho0 * c * A * s[2], d * c * A * s[1], tuple(d * ps * A * s[3 + j] for j in range(3)),
                     pf / area if count > 0 else 0.0, pf, d * 0.5 * rho0 * c ** 3 * A * s[7], area, int(count))


@dataclass
class BoxFlux:
    mass_imbalance: float           # [kg/s]: the sum of the six outward mass flows
    force: Tuple[float, float, float]       # [N] on the body inside
    Cd: float
    Cl: float


def box_quantities(faces: Sequence[Tuple[FluxPlan, PlaneFlux]], params) -> BoxFlux:
    """the control-volume balance over a box's six faces (outward directions): mass imbalance = sum of the outward mass flows;
    F_j = - sum_faces [momentum flux_j + p n_j A], n = direction e_axis - the steady balance without the viscous, subgrid and unsteady
    terms; Cd = F_x / F_ref, Cl = F_z / F_ref with forces.finish_forces' F_ref = rho0 U^2 / 2 x reference_area (no symmetry doubling)"""
    F = [0.0, 0.0, 0.0]
    dm = 0.0
    for plan, q in faces:
        dm += q.mass_flow
        for j in range(3):
            F[j] -= q.momentum[j]
        F[int(plan.spec.normal)] -= float(plan.spec.direction) * q.pressure_force
    F_ref = 0.5 * params.rho_physical * params.u_physical ** 2 * params.reference_area
    cd, cl = (F[0] / F_ref, F[2] / F_ref) if F_ref > 1e-10 else (0.0, 0.0)
    return BoxFlux(dm, (F[0], F[1], F[2]), cd, cl)


# ---- result files ----
FLUXES_CSV_HEADER = ("Step,Time_phys_s,Plane,MassFlow_kg_s,VolumeFlow_m3_s,MomentumFlux_x_N,MomentumFlux_y_N,MomentumFlux_z_N,"
                     "MeanGaugePressure_Pa,PressureForce_N,KineticEnergyFlux_W,ValidArea_m2,ValidPoints")
BOXES_CSV_COMMENT = ("# control-volume force F_j = -sum over the six faces of [momentum flux_j + p n_j A] with outward normals: "
                     "the steady balance without the viscous, subgrid and unsteady terms; Cd, Cl normalised as forces.csv's, "
                     "no symmetry doubling")
BOXES_CSV_HEADER = "Step,Time_phys_s,Box,MassImbalance_kg_s,Fx_N,Fy_N,Fz_N,Cd,Cl"


def fluxes_csv_row(step: int, time_phys: float, name: str, q: PlaneFlux) -> str:
    return "%d,%.10e,%s,%.10e,%.10e,%.10e,%.10e,%.10e,%.10e,%.10e,%.10e,%.10e,%d" % (
        step, time_phys, name, q.mass_flow, q.volume_flow, q.momentum[0], q.momentum[1], q.momentum[2], q.mean_pressure,
        q.pressure_force, q.kinetic_energy_flux, q.area, q.count)


def boxes_csv_row(step: int, time_phys: float, name: str, b: BoxFlux) -> str:
    return "%d,%.10e,%s,%.10e,%.10e,%.10e,%.10e,%.10e,%.10e" % (step, time_phys, name, b.mass_imbalance, b.force[0], b.force[1],
                                                                b.force[2], b.Cd, b.Cl)


def box_faces(boxes: Sequence[FluxBox], plans: Sequence[FluxPlan]) -> List[Tuple[str, List[int]]]:
    """(box name, indices into `plans` of its six faces) of every box"""
    return [(b.name, [k for k, p in enumerate(plans) if p.spec.box == b.name]) for b in boxes]


def csv_rows(plans: Sequence[FluxPlan], boxes: Sequence[FluxBox], steps, sums, counts, params) -> Tuple[List[str], List[str], list]:
    """(fluxes.csv rows, flux_boxes.csv rows, [(step, box name, BoxFlux)]) of downloaded samples"""
    faces = box_faces(boxes, plans)
    plane_rows, box_rows, box_values = [], [], []
    for i in range(len(steps)):
        step, time_phys = int(steps[i]), float(steps[i]) * params.time_scale
        q = [plane_quantities(p, sums[i][k], int(counts[i][k]), params) for k, p in enumerate(plans)]
        plane_rows += [fluxes_csv_row(step, time_phys, p.spec.name, q[k]) for k, p in enumerate(plans)]
        for name, idx in faces:
            b = box_quantities([(plans[k], q[k]) for k in idx], params)
            box_rows.append(boxes_csv_row(step, time_phys, name, b))
            box_values.append((step, name, b))
    return plane_rows, box_rows, box_values
