"""Cost of the wall diagnostics on the device - a census of every level (ludwig_level_wall_census), one compute and one download of
the wall-surface set (ludwig_wall_surface_*) - in ms, next to ludwig_level_monitor (the comparable 17 B per cell pass) timed on the same
levels in the same process, and the coarse step with the feature off.

Cases: the 256^3 periodic box with a wall model (one level; the cells of the lowest layer of blocks are given a wall distance of 0.5 to
8 cells, so 1 024 of its 32 768 blocks are near-wall) and the 3-level ball1m sphere (Bouzidi, wall model, temporal interpolation; the
surface set is the ball's 20 480 triangles on the finest level).
Per case:
  step_ms              one coarse step alone (mean over a batch), no observer made
  census_ms            a census of every level, back to back (rho already stored, a uniform velocity uploaded so that the model runs): 21 B per cell of a near-wall block, the flag test
                       alone elsewhere; per level one 1.6-KB upload, one launch, one 1.6-KB download and one synchronisation
  monitor_ms           a monitor record of every level, back to back
  census_over_monitor  the ratio of the two
  surface_compute_ms, surface_download_ms   (ball1m) one compute, queued and synchronised; one download of 7 floats per triangle
Host clock around work that ends in a device synchronise; the medians of a few repetitions.
usage: wall_cost.py [--out FILE]  (default: print only)"""
import dataclasses

import numpy as np

from _cost_common import add_row, box_case, golden_case, parse_args, timed, write_rows


def measure(name, grids, params, u, mesh=None, phys=None, n_steps=20, n_samples=20, reps=5):
    from open_ludwig_amd import adapt, execute_timestep_batch, statistics, surface_stats, wall_diagnostics as wd
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    sync = dev[0].synchronize
    t = [1]

    def steps(n):
        execute_timestep_batch(dev, t[0], n, np.float32(u), params)
        t[0] += n

    def census_all(tc):
        return [wd.census(d, statistics.t_sub_after(lvl, tc)) for lvl, d in enumerate(dev)]

    def monitor_all(tc):
        return [d.monitor(statistics.t_sub_after(lvl, tc)) for lvl, d in enumerate(dev)]

    steps(4)                                                       # warm-up: code objects, level streams
    step_ms = timed(lambda: steps(n_steps), sync, reps) / n_steps  # before any observer exists: the feature off
    for d, g in zip(dev, grids):                                   # from rest every near-wall cell would skip the model: a moving state
        v = np.zeros((8, 8, 8, g.n_blocks, 3), dtype=np.float32, order="F")
        v[..., 0], v[..., 1] = 0.04, 0.01
        d.upload("vel", v)
        d.upload("vel_temp", v)
    recs = census_all(t[0] - 1)                                    # warm-up: the census record, the monitor's slab, rho stored
    monitor_all(t[0] - 1)
    census_ms = timed(lambda: [census_all(t[0] - 1) for _ in range(n_samples)], sync, reps) / n_samples
    monitor_ms = timed(lambda: [monitor_all(t[0] - 1) for _ in range(n_samples)], sync, reps) / n_samples
    per_level = [timed(lambda d=d, lvl=lvl: [wd.census(d, statistics.t_sub_after(lvl, t[0] - 1)) for _ in range(n_samples)], sync, reps) / n_samples
                 for lvl, d in enumerate(dev)]
    res = {"case": name, "levels": len(grids), "blocks": [g.n_blocks for g in grids], "near_cells": [r.near_cells for r in recs],
           "evaluated_cells": [r.evaluated for r in recs],
           "step_ms": round(step_ms, 4), "census_ms": round(census_ms, 4), "census_ms_per_level": [round(v, 4) for v in per_level],
           "monitor_ms": round(monitor_ms, 4), "census_over_monitor": round(census_ms / monitor_ms, 3)}
    if mesh is not None:
        fin = len(grids) - 1
        plan = surface_stats.plan_surface(mesh, grids[fin], phys)
        S = wd.DeviceWallSurface(plan, dev[fin], phys)
        t_sub = statistics.t_sub_after(fin, t[0] - 1)
        S.compute(t_sub)
        S.download()
        res["triangles"] = plan.n
        res["surface_compute_ms"] = round(timed(lambda: [S.compute(t_sub) for _ in range(n_samples)], sync, reps) / n_samples, 4)
        res["surface_download_ms"] = round(timed(lambda: [S.download() for _ in range(n_samples)], sync, reps) / n_samples, 4)
        S.close()
    for d in dev:
        d.close()
    return res


def walled_box():
    """the 256^3 box with a wall model: the lowest layer of blocks lies 0.5 to 8 cells above a wall"""
    name, grids, params, u = box_case()
    g = grids[0]
    low = np.flatnonzero(np.asarray(g.map_z) == 1)
    for k in range(8):
        g.wall_dist[:, :, k, low] = np.float32(k + 0.5)
    return name + ", wall model, 1024 near-wall blocks", grids, dataclasses.replace(params, wall_model_active=True), 0.03


def main():
    args = parse_args("wall_cost.py")
    rows = []
    add_row(rows, measure(*walled_box()))
    name, cfg, grids, mesh, phys, params = golden_case()
    add_row(rows, measure(name, grids, params, cfg.u_lattice, mesh, phys))
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
