"""Cost of integrating flux planes inside the batches (the LUDWIG_OBSERVE_FLUXES entry of ludwig_execute_timestep_batch_observed:
k_flux_chunks / k_flux_combine on every level's own stream right after its last sub-step, no join) in ms per coarse step, against the
yardstick a user has without it: the same set sampled by ludwig_flux_planes_sample between batches of one.

Set: one box around the body (its bounding box grown by a quarter of its size on every side, clipped one coarse cell inside the domain)
at the finest level's spacing plus one wake plane over the full cross-section one body length behind it, interval 1, on ball1m
(3 levels) and on the wing at surface resolution 200 (--cases). The wake plane has the finest spacing too, doubled until it fits the point cap. One box, one copy of the
levels, the configurations alternating (off, in-batch, cut, batch1, and again), as tracers_cost.py does:
  off_ms        batches of --steps coarse steps, no set
  in_batch_ms   the same batches with the set sampled inside them at interval 1 (the ring drained after each batch)
  cut_ms        batches of ONE coarse step, ludwig_flux_planes_sample after each
  batch1_ms     batches of one coarse step with no set: what cutting alone costs
--step-only: the ball1m coarse step alone, one JSON line (for alternating processes of two checkouts: the feature off against its parent).
--trace: in-batch batches only, nothing timed (for a kernel trace of its own).
Host clock around work that ends in a device synchronise; the medians of 5 repetitions, every repetition kept beside them.
usage: flux_planes_cost.py [--out FILE] [--cases ball1m,wing] [--steps 40] [--step-only] [--trace]  (default: print only)"""
import numpy as np

from _cost_common import add_row, golden_case, parse_args, timed, write_rows
from streamlines_cost import ball_step_ms


def flux_set(grids, mesh, phys):
    """the planes of the measured set: the six faces of the box around the body, then the wake plane"""
    from open_ludwig_amd import flux_planes as fp, preprocess as pp
    lo, hi = np.asarray(mesh.min_bounds, dtype=np.float64), np.asarray(mesh.max_bounds, dtype=np.float64)
    grow = 0.25 * (hi - lo)
    # clipped one coarse cell inside the domain (a half model touches the symmetry plane: that face then cuts the body)
    off, dx1 = np.asarray(phys.mesh_offset, dtype=np.float64), float(grids[0].dx)
    dom_hi = np.array([grids[0].grid_dim_x, grids[0].grid_dim_y, grids[0].grid_dim_z], dtype=np.float64) * 8 * dx1 - off
    box_lo, box_hi = np.maximum(lo - grow, -off + dx1), np.minimum(hi + grow, dom_hi - dx1)
    box = pp.FluxBox("body", tuple((float(a), float(b)) for a, b in zip(box_lo, box_hi)))
    plans = [fp.plan_flux_plane(f, grids, phys.mesh_offset) for f in pp.flux_box_faces(box)]
    h = float(grids[-1].dx)
    while True:
        try:
            plans.append(fp.plan_flux_plane(pp.FluxPlane("wake", 0, float(hi[0] + (hi[0] - lo[0])), None, h), grids, phys.mesh_offset))
            return plans, h
        except ValueError as e:
            if "more than" not in str(e):
                raise
            h *= 2.0


def measure(key, n_steps, reps=5, trace=False):
    from open_ludwig_amd import adapt, execute_timestep_batch, flux_planes as fp
    name, cfg, grids, mesh, phys, params = golden_case(key)
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    u = np.float32(cfg.u_lattice)
    plans, wake_h = flux_set(grids, mesh, phys)
    s = fp.DeviceFluxPlanes(plans, dev, n_steps, 1, 1)
    sync = dev[0].synchronize
    t = [1]

    def batches(size, fluxes=None, between=None):
        def run():
            for _ in range(n_steps // size):
                execute_timestep_batch(dev, t[0], size, u, params, fluxes=fluxes)
                t[0] += size
                if between is not None:
                    between(t[0] - 1)
            if fluxes is not None or between is not None:
                s.download()
        return run
    configs = {"off_ms": batches(n_steps), "in_batch_ms": batches(n_steps, fluxes=s), "cut_ms": batches(1, between=s.sample),
               "batch1_ms": batches(1)}
    if trace:
        for _ in range(3):
            configs["in_batch_ms"]()
        s.close()
        for d in dev:
            d.close()
        return {"case": name, "traced_steps": 3 * n_steps}
    for run in configs.values():                                            # warm-up: streams, events, first launches
        run()
    got = {k: [] for k in configs}
    for _ in range(reps):                                                   # alternating, one repetition of each per round
        for k, run in configs.items():
            got[k].append(timed(run, sync, 1) / n_steps)
    s.close()
    for d in dev:
        d.close()
    lists = [idx.size for p in plans for _, idx in p.lists()]
    row = {"case": name, "cells": sum(512 * g.n_blocks for g in grids), "levels": len(grids), "planes": len(plans),
           "points": int(sum(p.n for p in plans)), "valid_points": int(sum(p.valid.sum() for p in plans)), "lists": len(lists),
           "chunks": int(sum(-(-n // 512) for n in lists)), "wake_spacing_over_finest_dx": wake_h / float(grids[-1].dx),
           "steps_per_batch": n_steps}
    for k, v in got.items():
        row[k] = round(float(np.median(v)), 4)
        row[k.replace("_ms", "_all_ms")] = [round(x, 4) for x in v]
    row["in_batch_extra_ms"] = round(row["in_batch_ms"] - row["off_ms"], 4)
    row["cut_extra_ms"] = round(row["cut_ms"] - row["off_ms"], 4)
    return row


def main():
    args = parse_args("flux_planes_cost.py", ("--step-only", {"action": "store_true"}), ("--trace", {"action": "store_true"}),
                      ("--cases", {"default": "ball1m,wing"}), ("--steps", {"type": int, "default": 40}))
    rows = []
    if args.step_only:
        name, ms = ball_step_ms()
        add_row(rows, {"case": name, "step_ms": round(ms, 4)})
    else:
        for key in [k for k in args.cases.split(",") if k]:
            add_row(rows, measure(key, args.steps, trace=args.trace))
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
