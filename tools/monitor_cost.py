"""Cost of one flow-monitor record per level (ludwig_level_monitor) on the device, in ms and TB/s, next to the yardstick
k_accumulate_stats timed in the same process.

Cases: the 256^3 periodic box (one level, the bench workload) and the 3-level ball1m sphere (Bouzidi, wall model, temporal interpolation).
Per case:
  step_ms            one coarse step alone (mean over a batch)
  stats_sample_ms    k_accumulate_stats of every level, back to back, no host synchronisation in between: 176 B per owned cell
  monitor_ms         a record of every level, back to back (rho already stored): 17 B per owned cell, and per level two or three
                     launches, one 80-byte download and one synchronisation - the host clock sees all of it
  monitor_replay_ms  the same right after a step whose rho store was elided: plus the rho replay
  run_case_added_ms_per_step  monitor_replay_ms / diag_freq of the shipped ball1m case: what advanced.flow_monitor adds to run_case
TB/s = bytes per cell x owned cells / time. Host clock around work that ends in a device synchronise; the medians of a few repetitions.
usage: monitor_cost.py [--out FILE]  (default: print only)"""
import os
import time

import numpy as np

from _cost_common import GOLDEN, add_row, box_case, golden_case, parse_args, timed, write_rows

STATS_BYTES_PER_CELL = 4 + 12 + 2 * 80
MONITOR_BYTES_PER_CELL = 4 + 12 + 1


def measure(name, grids, params, u, diag_freq, n_steps=20, n_samples=20, reps=5):
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

    def monitor_all(tc):
        return [d.monitor(statistics.t_sub_after(lvl, tc)) for lvl, d in enumerate(dev)]

    steps(4)                                                       # warm-up: code objects, level streams, the monitor's slab
    sample_all(t[0] - 1)
    recs = monitor_all(t[0] - 1)
    step_ms = timed(lambda: steps(n_steps), sync, reps) / n_steps
    sample_ms = timed(lambda: [sample_all(t[0] - 1) for _ in range(n_samples)], sync, reps) / n_samples
    monitor_ms = timed(lambda: [monitor_all(t[0] - 1) for _ in range(n_samples)], sync, reps) / n_samples
    per_level = [timed(lambda d=d, lvl=lvl: [d.monitor(statistics.t_sub_after(lvl, t[0] - 1)) for _ in range(n_samples)], sync, reps) / n_samples
                 for lvl, d in enumerate(dev)]
    replay = []
    for _ in range(reps):
        for d in dev:
            d.set_rho_store(False)                                 # the default policy: the next step may elide its rho store
        steps(1)
        sync()
        t0 = time.perf_counter()
        monitor_all(t[0] - 1)
        replay.append((time.perf_counter() - t0) * 1e3)
    replay_ms = float(np.median(replay))
    cells = sum(512 * g.n_blocks for g in grids)
    stats_tbps = STATS_BYTES_PER_CELL * cells / (sample_ms * 1e-3) / 1e12
    monitor_tbps = MONITOR_BYTES_PER_CELL * cells / (monitor_ms * 1e-3) / 1e12
    res = {"case": name, "levels": len(grids), "blocks": [g.n_blocks for g in grids], "cells": cells, "fluid_cells": [r.n_fluid for r in recs],
           "step_ms": round(step_ms, 4),
           "stats_sample_ms": round(sample_ms, 4), "stats_sample_TBps": round(stats_tbps, 3),
           "monitor_ms": round(monitor_ms, 4), "monitor_TBps": round(monitor_tbps, 3),
           "monitor_ms_per_level": [round(v, 4) for v in per_level],
           "monitor_TBps_per_level": [round(MONITOR_BYTES_PER_CELL * 512 * g.n_blocks / (v * 1e-3) / 1e12, 3) for g, v in zip(grids, per_level)],
           "monitor_over_stats_bandwidth": round(monitor_tbps / stats_tbps, 3),
           "monitor_replay_ms": round(replay_ms, 4),
           "diag_freq": int(diag_freq), "run_case_added_ms_per_step": round(replay_ms / diag_freq, 6),
           "run_case_added_pct_of_step": round(100.0 * replay_ms / diag_freq / step_ms, 4)}
    for d in dev:
        d.close()
    return res


def main():
    args = parse_args("monitor_cost.py")
    from open_ludwig_amd import preprocess as pp
    shipped = pp.load_case_configuration(os.path.join(GOLDEN, "ball1m_config.yaml"))
    rows = []
    add_row(rows, measure(*box_case(), shipped.diag_freq))
    name, cfg, grids, _, _, params = golden_case()
    add_row(rows, measure(name, grids, params, cfg.u_lattice, shipped.diag_freq))
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
