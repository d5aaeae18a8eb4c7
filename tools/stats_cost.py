"""Cost of one time-averaged statistics sample (ludwig_level_stats_accumulate) on the device, in ms and GB/s.

Cases: the 256^3 periodic box (one level, the bench workload) and the 3-level ball1m sphere (Bouzidi, wall model, temporal interpolation).
Per case:
  step_ms          one coarse step alone (mean over a batch)
  sample_ms        k_accumulate_stats alone, back to back (rho already stored): 176 B per owned cell
  sample_replay_ms one sample right after a step whose rho store was elided: the kernel plus the rho replay
  step_and_sample  a coarse step plus a sample of every level, per coarse step, sampling every `interval` steps
GB/s = 176 B x owned cells / sample_ms. Host clock around work that ends in a device synchronise; the medians of a few repetitions.
usage: stats_cost.py [--out FILE]  (default: print only)"""
import time

import numpy as np

from _cost_common import add_row, box_case, golden_case, parse_args, timed, write_rows

BYTES_PER_CELL = 4 + 12 + 2 * 80


def measure(name, grids, params, u, n_steps=20, n_samples=20, reps=5, interval=10):
    from open_ludwig_amd import adapt, execute_timestep_batch, statistics
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
        d.stats_reset()
    sync = dev[0].synchronize
    t = [1]

    def steps(n):
        execute_timestep_batch(dev, t[0], n, np.float32(u), params)
        t[0] += n

    def sample_all(tc):
        for lvl, d in enumerate(dev):
            d.stats_accumulate(statistics.t_sub_after(lvl, tc))

    steps(4)                                                       # warm-up: code objects, level streams
    sample_all(t[0] - 1)
    step_ms = timed(lambda: steps(n_steps), sync, reps) / n_steps
    sample_ms = timed(lambda: [sample_all(t[0] - 1) for _ in range(n_samples)], sync, reps) / n_samples
    replay = []
    for _ in range(reps):
        for d in dev:
            d.set_rho_store(False)                                 # the default policy: the next step may elide its rho store
        steps(1)
        sync()
        t0 = time.perf_counter()
        sample_all(t[0] - 1)
        sync()
        replay.append((time.perf_counter() - t0) * 1e3)

    def run_sampled():
        for _ in range(n_steps // interval):
            steps(interval)
            sample_all(t[0] - 1)
    both_ms = timed(run_sampled, sync, reps) / (n_steps // interval * interval)
    cells = sum(512 * g.n_blocks for g in grids)
    res = {"case": name, "levels": len(grids), "blocks": [g.n_blocks for g in grids], "cells": cells,
           "step_ms": round(step_ms, 4), "sample_ms": round(sample_ms, 4),
           "sample_GBps": round(BYTES_PER_CELL * cells / (sample_ms * 1e-3) / 1e9, 1),
           "sample_replay_ms": round(float(np.median(replay)), 4),
           "interval": interval, "step_and_sample_ms_per_step": round(both_ms, 4),
           "overhead_per_step_pct": round(100.0 * (both_ms / step_ms - 1.0), 2)}
    for d in dev:
        d.close()
    return res


def main():
    args = parse_args("stats_cost.py")
    rows = []
    add_row(rows, measure(*box_case()))
    name, cfg, grids, _, _, params = golden_case()
    add_row(rows, measure(name, grids, params, cfg.u_lattice))
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
