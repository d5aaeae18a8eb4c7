"""Cost of filling a level from a flow source (ludwig_level_init_from_source: k_init_from_source) beside ludwig_init_equilibrium of the
same level in the same process, in ms on the device, and the store bandwidth it reaches.

Set-ups: the 256^3 periodic box (the bench workload) and ball1m on 3 levels, each after 4 coarse steps from rest; the source is the
hierarchy's own flow (ludwig_flow_source_from_levels) under the identity map, so every fluid cell is found.
  init_from_source_ms   the call without counts between two HIP events on the level's stream (the null stream); the median of
                        `--reps` after one warm-up. With counts it adds one 8-byte-per-counter download and a synchronisation.
  init_equilibrium_ms   ludwig_init_equilibrium of the same level, the same way: two or three fills of constants (no rho, no vel)
  bytes_per_cell        what the pass stores: 27 + 27 populations, 3 + 3 velocities and rho = 244 B, 368 B with the saved state
  store_TBps            bytes_per_cell x cells / init_from_source_ms
  source_ms             ludwig_flow_source_from_levels of the whole hierarchy (host clock; allocation, copies, synchronisation)
--step-only: the ball1m coarse step alone, one JSON line (for alternating processes of two checkouts: the keys off against the parent).
usage: warm_start_cost.py [--out FILE] [--cases box,ball1m] [--reps 7] [--step-only]  (default: print only)"""
import time

import numpy as np

from _cost_common import HipEvent, add_row, box_case, golden_case, parse_args, timed, write_rows


def event_ms(fn, reps):
    e0, e1 = HipEvent(), HipEvent()
    fn()
    out = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        out.append(e0.elapsed_ms(e1))
    return float(np.median(out)), [round(min(out), 4), round(max(out), 4)]


def measure(key, reps):
    from open_ludwig_amd import adapt, execute_timestep_batch, warm_start as ws
    if key == "box":
        name, grids, params, u = box_case()
    else:
        name, cfg, grids, _, _, params = golden_case(key)
        u = float(cfg.u_lattice)
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    execute_timestep_batch(dev, 1, 4, np.float32(u), params)
    t0 = time.perf_counter()
    src = ws.DeviceFlowSource.from_levels(dev, 4)
    source_ms = (time.perf_counter() - t0) * 1e3
    rows = []
    for li, (g, d) in enumerate(zip(grids, dev)):
        m = np.array([2.0 ** -li] * 3 + [0.0] * 3, np.float32)
        counts = d.init_from_source(src, m, 1.0, (1.0, 0.0, 0.0, 0.0))
        warm_ms, warm_span = event_ms(lambda: d.init_from_source(src, m, 1.0, (1.0, 0.0, 0.0, 0.0), counts=False), reps)
        eq_ms, eq_span = event_ms(d.init_equilibrium, reps)
        cells = 512 * g.n_blocks
        per_cell = 368 if d.has_temporal_storage else 244
        rows.append({"case": name, "level": g.level_id, "cells": cells, "source_levels": len(grids), "found": int(counts[0]),
                     "init_from_source_ms": round(warm_ms, 4), "init_from_source_ms_min_max": warm_span,
                     "init_equilibrium_ms": round(eq_ms, 4), "init_equilibrium_ms_min_max": eq_span, "bytes_per_cell": per_cell,
                     "store_TBps": round(per_cell * cells / (warm_ms * 1e-3) / 1e12, 3), "source_ms": round(source_ms, 3)})
    src.close()
    for d in dev:
        d.close()
    return rows


def ball_step_ms(n_steps=20, reps=5):
    from open_ludwig_amd import adapt, execute_timestep_batch
    name, cfg, grids, _, _, params = golden_case()
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    execute_timestep_batch(dev, 1, 4, np.float32(cfg.u_lattice), params)
    ms = timed(lambda: execute_timestep_batch(dev, 5, n_steps, np.float32(cfg.u_lattice), params), dev[0].synchronize, reps) / n_steps
    for d in dev:
        d.close()
    return name, ms


def main():
    args = parse_args("warm_start_cost.py", ("--cases", {"default": "box,ball1m"}), ("--reps", {"type": int, "default": 7}),
                      ("--step-only", {"action": "store_true"}))
    rows = []
    if args.step_only:
        name, ms = ball_step_ms()
        add_row(rows, {"case": name, "step_ms": round(ms, 4)})
    else:
        for key in [k for k in args.cases.split(",") if k]:
            for row in measure(key, args.reps):
                add_row(rows, row)
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
