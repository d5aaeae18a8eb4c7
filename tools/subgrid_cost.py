"""Cost of the subgrid observer on the device - k_subgrid<FIELDS> (ludwig_level_subgrid_fields_compute) and k_subgrid<SUMS>
(ludwig_level_subgrid_stats_accumulate) - in ms and GB/s per call, next to their yardsticks timed in the same process:
k_velocity_gradient_fields (the same staging, 38 B per cell) and k_accumulate_stats (the same Float64 read-modify-write, 176 B per cell).

Cases: the 256^3 periodic box (one level, the bench workload) and every level of the 3-level ball1m sphere.
Per level, each a call alone, back to back on the level's stream (no download):
  fields_ms, fields_GBps       FIELDS_BYTES x owned cells / fields_ms
  sums_ms, sums_GBps           SUMS_BYTES x owned cells / sums_ms
  gradient_ms, gradient_GBps   GRADIENT_BYTES per cell
  stats_ms, stats_GBps         STATS_BYTES per cell
Per case: step_ms, one coarse step (mean over a batch) taken before any observer exists: the feature off.
FIELDS_BYTES = 12 (own velocity) + 9 (the six face layers: 6 x 64 cells x 12 B / 512) + 1 (obstacle) + 8 (written) = 30;
SUMS_BYTES = 12 + 9 + 1 + 24 (sums read) + 24 (sums written) = 70.
Host clock around work that ends in a device synchronise; the medians of a few repetitions.
usage: subgrid_cost.py [--out FILE] [--step-only]  (default: print only; --step-only: the coarse step of ball1m alone, for comparing
two builds of the library through LUDWIG_HIP_LIB, a process each)"""
import numpy as np

from _cost_common import add_row, box_case, golden_case, parse_args, timed, write_rows

FIELDS_BYTES = 12 + 9 + 1 + 8
SUMS_BYTES = 12 + 9 + 1 + 24 + 24
GRADIENT_BYTES = 12 + 9 + 1 + 16
STATS_BYTES = 16 + 80 + 80


def measure(name, grids, params, u, n_steps=20, n_calls=20, reps=5, step_only=False):
    from open_ludwig_amd import _lib, adapt, execute_timestep_batch
    lib = _lib.load()
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    sync = dev[0].synchronize
    execute_timestep_batch(dev, 1, 4, np.float32(u), params)            # warm-up: code objects, level streams, a flow
    step_ms = timed(lambda: execute_timestep_batch(dev, 5, n_steps, np.float32(u), params), sync, reps) / n_steps
    res = {"case": name, "step_ms": round(step_ms, 4)}
    if not step_only:
        levels = []
        for g, d in zip(grids, dev):
            scale = float(np.float32(1.0 / g.dx))
            d.stats_reset()
            d.subgrid_stats_reset()
            calls = {"fields": (FIELDS_BYTES, lambda: lib.ludwig_level_subgrid_fields_compute(d.handle, _lib.VEL)),
                     "sums": (SUMS_BYTES, lambda: lib.ludwig_level_subgrid_stats_accumulate(d.handle, 1)),
                     "gradient": (GRADIENT_BYTES, lambda: lib.ludwig_level_gradient_fields_compute(d.handle, _lib.VEL, scale)),
                     "stats": (STATS_BYTES, lambda: lib.ludwig_level_stats_accumulate(d.handle, 1))}
            cells = 512 * g.n_blocks
            row = {"level": g.level_id, "blocks": g.n_blocks, "cells": cells}
            for key, (nbytes, call) in calls.items():
                def many():
                    for _ in range(n_calls):
                        _lib.check(call())
                many()                                                   # allocation, first launch
                ms = timed(many, sync, reps) / n_calls
                row[key + "_ms"] = round(ms, 4)
                row[key + "_GBps"] = round(nbytes * cells / (ms * 1e-3) / 1e9, 1)
            levels.append(row)
        res["levels"] = levels
        for key in ("fields", "sums", "gradient", "stats"):
            res[key + "_all_levels_ms"] = round(sum(l[key + "_ms"] for l in levels), 4)
    for d in dev:
        d.close()
    return res


def main():
    args = parse_args("subgrid_cost.py", ("--step-only", {"action": "store_true"}))
    rows = []
    if not args.step_only:
        add_row(rows, measure(*box_case()))
    name, cfg, grids, _, _, params = golden_case()
    add_row(rows, measure(name, grids, params, cfg.u_lattice, step_only=args.step_only))
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
