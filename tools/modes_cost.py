"""Cost of accumulating Fourier modes on the device (ludwig_modes_*, the LUDWIG_OBSERVE_MODES entry of
ludwig_execute_timestep_batch_observed: k_accumulate_modes on every level's own stream right after its last sub-step, no join).

(a) the kernel: one sample of every level, back to back (rho already stored), for M = 3 and M = 7 table columns on the 256^3 periodic
    box and on ball1m, and in the same process k_accumulate_stats by the method of stats_cost.py. Bytes per cell and sample: 16 + 64 M
    (modes), 176 (statistics); GB/s = bytes x cells / ms.
(b) the ball1m coarse step with the observer (M = 7: three frequencies) inside batches of --steps coarse steps at interval 1 and at
    interval 10, against the same batches without it. One copy of the levels, the configurations alternating (off, every 1, every 10,
    and again), as probe_cost.py does.
--step-only: the ball1m coarse step alone, one JSON line (for alternating processes of two checkouts: the feature off against its parent).
Host clock around work that ends in a device synchronise; the medians of 5 repetitions, every repetition kept beside them.
usage: modes_cost.py [--out FILE] [--steps 40] [--step-only]  (default: print only)"""
import numpy as np

from _cost_common import add_row, box_case, golden_case, parse_args, timed, write_rows
from streamlines_cost import ball_step_ms

STATS_BYTES_PER_CELL = 4 + 12 + 2 * 80
N_ROWS = 4096


def modes_bytes_per_cell(m):
    return 16 + 64 * m


def kernel_row(name, grids, params, u, n_samples=20, reps=5):
    from open_ludwig_amd import _lib, adapt, execute_timestep_batch, statistics
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
        d.stats_reset()
        d.set_rho_store(True)
    sync = dev[0].synchronize
    execute_timestep_batch(dev, 1, 4, np.float32(u), params)      # warm-up: code objects, level streams; the state after step 4
    cells = sum(512 * g.n_blocks for g in grids)
    row = {"case": name, "levels": len(grids), "blocks": [g.n_blocks for g in grids], "cells": cells}

    def stats_all():
        for lvl, d in enumerate(dev):
            d.stats_accumulate(statistics.t_sub_after(lvl, 4))
    stats_all()
    got = {"stats": [timed(lambda: [stats_all() for _ in range(n_samples)], sync, 1) / n_samples for _ in range(reps)]}
    for m in (3, 7):
        S = _lib.ModeSet(dev, np.random.default_rng(m).uniform(-1.0, 1.0, (N_ROWS, m)))
        taken = [0]

        def modes_all():
            for lvl in range(len(dev)):
                S.accumulate(lvl, statistics.t_sub_after(lvl, 4), taken[0])
            taken[0] += 1
        modes_all()
        got[f"modes_M{m}"] = [timed(lambda: [modes_all() for _ in range(n_samples)], sync, 1) / n_samples for _ in range(reps)]
        S.close()
    for k, v in got.items():
        ms = float(np.median(v))
        per_cell = STATS_BYTES_PER_CELL if k == "stats" else modes_bytes_per_cell(int(k.split("M")[1]))
        row[f"{k}_sample_ms"] = round(ms, 4)
        row[f"{k}_sample_all_ms"] = [round(x, 4) for x in v]
        row[f"{k}_bytes_per_cell"] = per_cell
        row[f"{k}_GBps"] = round(per_cell * cells / (ms * 1e-3) / 1e9, 1)
    for d in dev:
        d.close()
    return row


def observer_row(n_steps, reps=5, m=7):
    from open_ludwig_amd import _lib, adapt, execute_timestep_batch
    name, cfg, grids, _, _, params = golden_case("ball1m")
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    u = np.float32(cfg.u_lattice)
    S = _lib.ModeSet(dev, np.random.default_rng(m).uniform(-1.0, 1.0, (N_ROWS, m)))
    sync = dev[0].synchronize
    t, taken = [1], [0]

    def batches(interval=None):
        def run():
            if interval is None:
                execute_timestep_batch(dev, t[0], n_steps, u, params)
            else:
                k = -(-n_steps // interval)
                if taken[0] + k > N_ROWS:
                    S.reset()
                    taken[0] = 0
                # the schedule whose next row is the set's count: the batch's first step is sampled with that row
                S.start_step, S.interval = t[0] - taken[0] * interval, interval
                execute_timestep_batch(dev, t[0], n_steps, u, params, modes=S)
                taken[0] += k
            t[0] += n_steps
        return run
    configs = {"off_ms": batches(), "every_1_ms": batches(1), "every_10_ms": batches(10)}
    for run in configs.values():                                            # warm-up: streams, events, first launches
        run()
    got = {k: [] for k in configs}
    for _ in range(reps):                                                   # alternating, one repetition of each per round
        for k, run in configs.items():
            got[k].append(timed(run, sync, 1) / n_steps)
    S.close()
    for d in dev:
        d.close()
    row = {"case": name, "cells": sum(512 * g.n_blocks for g in grids), "levels": len(grids), "columns": m, "steps_per_batch": n_steps}
    for k, v in got.items():
        row[k] = round(float(np.median(v)), 4)
        row[k.replace("_ms", "_all_ms")] = [round(x, 4) for x in v]
    row["every_1_extra_ms"] = round(row["every_1_ms"] - row["off_ms"], 4)
    row["every_10_extra_ms"] = round(row["every_10_ms"] - row["off_ms"], 4)
    return row


def main():
    args = parse_args("modes_cost.py", ("--step-only", {"action": "store_true"}), ("--steps", {"type": int, "default": 40}))
    rows = []
    if args.step_only:
        name, ms = ball_step_ms()
        add_row(rows, {"case": name, "step_ms": round(ms, 4)})
    else:
        add_row(rows, kernel_row(*box_case()))
        name, cfg, grids, _, _, params = golden_case("ball1m")
        add_row(rows, kernel_row(name, grids, params, cfg.u_lattice))
        add_row(rows, observer_row(args.steps))
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
