"""One maker and one sampler per observer kind, shared by tests/test_gpu_replaced_buffers.py and tests/test_gpu_record_state.py.

makers(): the sets that are objects of their own (probes, surface statistics, ...). level_makers(): the readers that live on the level
itself or elsewhere (statistics, monitor, gradient fields, iso-surfaces, the surface-stress map, images, a warm-start source, halo packs).
Every entry is (make, sample): make() returns an object with close(), sample(object) a list of arrays. All of them are written for the
32^3 periodic box of 64 blocks (points, seeds, planes and the camera lie inside it)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import _inprocess_world as iw
import _surface_common as sc
from open_ludwig_amd import _lib, flux_planes as fp, force_series as fs, forces, preprocess as pp, probes as pm, render as rd
from open_ludwig_amd import slices as sl, streamlines as st, surface_stats as ss, tracers as tr, wall_diagnostics as wd, warm_start as ws

F32 = np.float32


def surface_plan(n_blocks, n=600, seed=3):
    """a hand-made plan: more triangles than one chunk of 512 (the force series reduces in two stages), some without a cell"""
    rng = np.random.default_rng(seed)
    found = rng.random(n) > 0.1
    blocks = np.where(found, rng.integers(0, n_blocks, n), -1).astype(np.int32)
    cells = np.where(found, rng.integers(0, 512, n), 0).astype(np.int32)
    normals = rng.standard_normal((n, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    plan = ss.SurfacePlan(found, blocks, cells, rng.uniform(0.1, 0.9, n).astype(F32), normals.astype(F32))
    return plan, rng.uniform(0.5, 1.5, n).astype(F32), rng.uniform(-4.0, 4.0, (3, n)).astype(F32)


POINTS = [[3.3, 4.2, 5.1], [30.5, 9.25, 17.75], [20.0, 8.0, 8.0], [15.9, 16.1, 24.0]]
SEEDS = np.array([[5.2, 7.3, 11.6], [3.25, 20.125, 2.9], [16.0, 16.0, 16.0]], dtype=F32)
T = 2                                                       # the state the samples read: after coarse step 2


def makers(grids, dev, t=T):
    """t: the coarse step whose state the samples read (a level's newest state after t steps)"""
    g = grids[0]
    plan, area, arm = surface_plan(g.n_blocks)
    sparams = sc.tunnel_params((16.0, 16.0, 16.0), 5.0)
    pplan = pm.plan_probes(POINTS, grids)
    fplans = [fp.plan_flux_plane(pp.FluxPlane("x", 0, 12.0, None, 1.0), grids),
              fp.plan_flux_plane(pp.FluxPlane("z", 2, 20.0, ((4.0, 27.0), (4.0, 27.0)), 1.0), grids)]
    splans = [sl.plan_slice(pp.SlicePlane("z", 2, 16.05, ((0.2, 30.8), (0.3, 30.7)), 0.37, pp.SLICE_FIELDS), grids)]
    W = np.array([[1.0, 0.5], [0.25, -1.0]])

    def sampled(S, *calls):
        for name, args in calls:
            getattr(S, name)(*args)
        out = S.download(0, 1) if isinstance(S, _lib.ModeSet) else S.download()
        return [np.asarray(x) for x in (out if isinstance(out, (tuple, list)) else (out,))]

    return {
        "probes": (lambda: pm.DeviceProbes(pplan, [dev], 8, 1, 1), lambda S: sampled(S, ("sample", (0, t)))),
        "surface_stats": (lambda: ss.DeviceSurfaceStats(plan, dev, 0, g.tau, sparams), lambda S: sampled(S, ("accumulate", (t,)))),
        "force_series": (lambda: fs.DeviceForceSeries(plan, area, arm, dev, 0, g.tau, sparams), lambda S: sampled(S, ("sample", (t, t)))),
        "flux_planes": (lambda: fp.DeviceFluxPlanes(fplans, [dev], 4), lambda S: sampled(S, ("sample", (t,)))),
        "modes": (lambda: _lib.ModeSet([dev], W), lambda S: sampled(S, ("accumulate", (0, t, 0)))),
        "wall_surface": (lambda: wd.DeviceWallSurface(plan, dev, sparams), lambda S: sampled(S, ("compute", (t,)))),
        "slices": (lambda: sl.DeviceSlices(splans, [dev], grids), lambda S: sampled(S, ("sample", (t,)))),
        "streamlines": (lambda: st.DeviceStreamlines([dev], SEEDS, np.ones(len(SEEDS), F32), 0.5, 1.0e-6, 40),
                        lambda S: sampled(S, ("trace", (t,)))),
        "tracers": (lambda: tr.DeviceTracers([dev], SEEDS, 2, 1, 1, 1), lambda S: sampled(S, ("advance", (t,)), ("advance", (t,)), ("snapshot", (t,)))),
    }


def batch_set(kind, grids, dev, start_step):
    """the set of `kind` for an observed batch that starts at coarse step start_step and samples every step: the one of makers(), but a
    mode set gets a window of four rows that begins there (a batch must not run past its window)"""
    if kind == "modes":
        return _lib.ModeSet([dev], np.array([[1.0, 0.5], [0.25, -1.0], [-0.5, 2.0], [1.5, 0.125]]), start_step=start_step)
    return makers(grids, dev)[kind][0]()


KINDS = ("probes", "surface_stats", "force_series", "flux_planes", "modes", "wall_surface", "slices", "streamlines", "tracers")


# ---- the readers that are no set of their own ----
class Nothing:
    """what make() returns where the reader needs no object"""

    def close(self):
        pass


def newest_vel(t):
    """the velocity buffer a level index 0 wrote in coarse step t"""
    return "vel_temp" if t % 2 == 0 else "vel"


# a closed tetrahedron-like patch of four triangles inside the box (centres and unit normals are all the device map reads)
_MESH_CENTERS = np.array([[10.3, 11.2, 12.1], [21.7, 9.4, 15.2], [16.2, 22.6, 7.9], [5.5, 27.1, 25.3]], dtype=F32)
_MESH_NORMALS = np.array([[1.0, 0.0, 0.0], [0.0, 0.6, 0.8], [-0.6, 0.0, 0.8], [0.0, -1.0, 0.0]], dtype=F32)
MESH = SimpleNamespace(centers=_MESH_CENTERS, normals=_MESH_NORMALS)

CAMERA = {"type": "perspective", "position": [-19.0, -13.0, 41.0], "look_at": [16.0, 16.0, 16.0], "up": [0.0, 0.0, 1.0], "fov": 50.0}
IMAGE_SIZE = (16, 12)                                       # 64 x 48 at most
RENDER_FIELDS = ("density", "velocity_magnitude", "q_criterion", "vorticity_magnitude")


def iso_values(state):
    """(density, speed) values that cut the flow `state` (a dict with rho and vel of the newest state) about in half"""
    speed = np.linalg.norm(state["vel"].astype(np.float64), axis=-1)
    return float(np.median(state["rho"])), float(np.median(speed))


def render_ranges(state):
    speed = np.linalg.norm(state["vel"].astype(np.float64), axis=-1)
    return {"density": (float(state["rho"].min()), float(state["rho"].max())), "velocity_magnitude": (float(speed.min()), float(speed.max())),
            "q_criterion": (-1.0e-4, 1.0e-4), "vorticity_magnitude": (0.0, 0.02)}


def self_plan_lists(n_blocks, seed=11, n=257):
    """(send, receive) lists of a self-rank halo plan, per group: an odd count of distinct element offsets all over the field"""
    rng = np.random.default_rng(seed)
    one = lambda: {g: np.sort(rng.choice(512 * n_blocks * iw.GROUP_COMPONENTS[g], n, replace=False)).astype(np.int64) for g in ("f", "vel", "rho")}
    return one(), one()


def self_plan(dev, send, recv):
    """a halo plan of `dev` whose only peer is rank 0 itself, without a communicator"""
    rc, h = iw.create_plan(dev, [0], {k: [v] for k, v in send.items()}, {k: [v] for k, v in recv.items()})
    _lib.check(rc)
    return iw.PlanHandle(h, dev)


def level_makers(grids, dev, t, state, target=None):
    """state: the flow the readers are expected to see (rho and the newest vel), which iso values and colour ranges are chosen from, so
    that no output is empty or constant. target: a second DeviceLevel of the same grid that init_from_source fills (warm_start)."""
    g = grids[0]
    lib = _lib.load()
    vn = newest_vel(t)
    rho_iso, speed_iso = iso_values(state)
    ranges = render_ranges(state)
    sparams = sc.tunnel_params((0.0, 0.0, 0.0), 1.0)
    send, recv = self_plan_lists(g.n_blocks)
    nothing = Nothing

    def stats(_):
        dev.stats_reset()
        dev.stats_accumulate(t)
        return [dev.stats_download(s)[0] for s in ("rho", "vel", "vel2")]

    def monitor(_):
        counts, cells = np.zeros(2, np.int64), np.zeros(16, np.int64)
        extremes, sums = np.zeros(3, F32), np.zeros(2, np.float64)
        _lib.check(lib.ludwig_level_monitor(dev.handle, int(t), counts.ctypes.data, cells.ctypes.data, extremes.ctypes.data, sums.ctypes.data))
        return [counts, cells, extremes, sums]

    def census(_):
        rec = _lib.WallCensus()
        _lib.check(lib.ludwig_level_wall_census(dev.handle, int(t), C.byref(rec)))
        return [np.frombuffer(bytes(rec), dtype=np.uint8).copy()]

    def subgrid_stats(_):
        dev.subgrid_stats_reset()
        dev.subgrid_stats_accumulate(t)
        return [dev.subgrid_stats_download(s)[0] for s in ("nu", "nunu", "eps")]

    def iso(field, value):
        def sample(_):
            n, pos, att, keys = dev.isosurface(field, value, vn)
            assert n > 0, f"the {field} surface at {value} is empty"
            return [np.array([n], np.int64), pos, att, keys]
        return sample

    def image(R):
        out = []
        table = rd.bake_table("coolwarm", 0.05)
        cam, persp = rd.Camera.build(CAMERA, *IMAGE_SIZE).arrays()
        for field in RENDER_FIELDS:
            lo, hi = ranges[field]
            R.image(t, field, np.ones(1, F32), camera=cam, perspective=persp, width=IMAGE_SIZE[0], height=IMAGE_SIZE[1], step=0.5, lo=lo, hi=hi,
                    max_samples=4096, table=table)
            out += list(R.download())
        return out

    def warm(_):
        src = ws.DeviceFlowSource.from_levels([dev], t)
        try:
            counts = target.init_from_source(src, (1.0, 1.0, 1.0, 0.0, 0.0, 0.0), 1.0, (1.0, 0.0, 0.0, 0.0))
            return [counts] + [target.download(n) for n in ("f", "f_temp", "vel", "vel_temp", "rho")]
        finally:
            src.close()

    def packed(P):
        out = []
        for group, field in (("f", "f_temp" if t % 2 == 0 else "f"), ("vel", vn), ("rho", "rho")):
            _lib.check(P.pack(group, field))
            out.append(P.read_send(group))
        return out

    def gathered(_):
        import torch
        out = []
        for group, field in (("f", "f_temp" if t % 2 == 0 else "f"), ("vel", vn)):
            idx = torch.as_tensor(send[group], device="cuda:0")
            buf = torch.empty(idx.numel(), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            _lib.check(lib.ludwig_halo_pack(dev.handle, _lib.FIELD_NAMES[field], C.c_void_p(idx.data_ptr()), idx.numel(), C.c_void_p(buf.data_ptr()),
                                            None))
            dev.synchronize()
            out.append(buf.cpu().numpy().view(np.uint32))
        return out

    return {
        "rho_min": (nothing, lambda _: [np.array([dev.rho_min()], F32)]),
        "stats": (nothing, stats),
        "monitor": (nothing, monitor),
        "wall_census": (nothing, census),
        "gradient_vel": (nothing, lambda _: list(dev.gradient_fields("vel", 1.0))),
        "gradient_vel_temp": (nothing, lambda _: list(dev.gradient_fields("vel_temp", 1.0))),
        "subgrid_fields": (nothing, lambda _: list(dev.subgrid_fields(vn))),
        "subgrid_stats": (nothing, subgrid_stats),
        "iso_density": (nothing, iso("density", rho_iso)),
        "iso_speed": (nothing, iso("velocity_magnitude", speed_iso)),
        "surface_stress_map": (nothing, lambda _: list(forces.map_surface_stresses_device(MESH, dev, 1.0, g.tau, sparams, 5, vn))),
        "render": (lambda: rd.DeviceRender([dev], IMAGE_SIZE[0] * IMAGE_SIZE[1]), image),
        "warm_start": (nothing, warm),
        "halo_plan_pack": (lambda: self_plan(dev, send, recv), packed),
        "halo_pack": (nothing, gathered),
    }


LEVEL_KINDS = ("rho_min", "stats", "monitor", "wall_census", "gradient_vel", "gradient_vel_temp", "subgrid_fields", "subgrid_stats",
               "iso_density", "iso_speed", "surface_stress_map", "render", "warm_start", "halo_plan_pack", "halo_pack")
# a plain level has no near-wall cell, so its census is the empty record whatever the flow is
CONSTANT_ON_A_PLAIN_LEVEL = ("wall_census",)
# making the set is itself a ruler: a halo plan bans the record step on its level
BANNING_KINDS = ("halo_plan_pack",)
