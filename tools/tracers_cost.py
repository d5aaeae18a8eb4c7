"""Cost of advecting tracers inside the batches (ludwig_execute_timestep_batch_tracers: k_tracers_advance behind every coarse step, a
join of the level streams around it) in ms per coarse step, against the yardstick a user has without it: the same set advanced by
ludwig_tracers_advance between batches of one.

Set: 1 024 seeds (the streamline tool's 32 x 32 rake two coarse cells upstream of the finest level's box) x 64 generations, released
every advance, interval 1, on ball1m (3 levels) and on the wing at surface resolution 200 (--cases). One box, one copy of the levels, the
configurations alternating (off, in-batch, cut, and again), as probe_cost.py does:
  off_ms        batches of --steps coarse steps, no set
  in_batch_ms   the same batches with the set advanced inside them at interval 1
  cut_ms        batches of ONE coarse step, ludwig_tracers_advance after each
  batch1_ms     batches of one coarse step with no set: what cutting alone costs
  snapshot_ms, download_ms   one snapshot launch; its records to the host
--step-only: the ball1m coarse step alone, one JSON line (for alternating processes of two checkouts: the feature off against its parent).
Host clock around work that ends in a device synchronise; the medians of 5 repetitions.
usage: tracers_cost.py [--out FILE] [--cases ball1m,wing] [--steps 40] [--step-only]  (default: print only)"""
import numpy as np

from _cost_common import add_row, golden_case, parse_args, timed, write_rows
from streamlines_cost import ball_step_ms, rake

GENERATIONS = 64


def measure(key, n_steps, reps=5):
    from open_ludwig_amd import adapt, execute_timestep_batch, tracers as tr
    name, cfg, grids, _, _, params = golden_case(key)
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    u = np.float32(cfg.u_lattice)
    seeds = rake(grids)
    s = tr.DeviceTracers(dev, seeds, GENERATIONS, 1, 1, 1)
    sync = dev[0].synchronize
    t = [1]

    def batches(size, tracers=None, between=None):
        def run():
            for _ in range(n_steps // size):
                execute_timestep_batch(dev, t[0], size, u, params, tracers=tracers)
                t[0] += size
                if between is not None:
                    between(t[0] - 1)
        return run
    configs = {"off_ms": batches(n_steps), "in_batch_ms": batches(n_steps, tracers=s), "cut_ms": batches(1, between=s.advance),
               "batch1_ms": batches(1)}
    for run in configs.values():                                            # warm-up: streams, events, first launches; fills the ring
        run()
    for _ in range(max(0, GENERATIONS - 2 * n_steps)):
        s.advance(t[0] - 1)
    got = {k: [] for k in configs}
    for _ in range(reps):                                                   # alternating, one repetition of each per round
        for k, run in configs.items():
            got[k].append(timed(run, sync, 1) / n_steps)
    snap_ms = timed(lambda: s.snapshot(t[0] - 1), sync, reps)
    both_ms = timed(lambda: (s.snapshot(t[0] - 1), s.download()), sync, reps)
    rec, k_adv = s.download()
    s.close()
    for d in dev:
        d.close()
    row = {"case": name, "cells": sum(512 * g.n_blocks for g in grids), "levels": len(grids), "seeds": int(len(seeds)),
           "generations": GENERATIONS, "slots": int(rec.shape[0]), "steps_per_batch": n_steps, "advances": k_adv,
           "alive": int((rec[:, 7] == 0).sum()), "outside": int((rec[:, 7] == 1).sum()), "obstacle": int((rec[:, 7] == 2).sum())}
    for k, v in got.items():
        row[k] = round(float(np.median(v)), 4)
        row[k.replace("_ms", "_all_ms")] = [round(x, 4) for x in v]
    row["in_batch_extra_ms"] = round(row["in_batch_ms"] - row["off_ms"], 4)
    row["cut_extra_ms"] = round(row["cut_ms"] - row["off_ms"], 4)
    row["snapshot_ms"], row["download_ms"] = round(snap_ms, 3), round(both_ms - snap_ms, 3)
    return row


def main():
    args = parse_args("tracers_cost.py", ("--step-only", {"action": "store_true"}), ("--cases", {"default": "ball1m,wing"}),
                      ("--steps", {"type": int, "default": 40}))
    rows = []
    if args.step_only:
        name, ms = ball_step_ms()
        add_row(rows, {"case": name, "step_ms": round(ms, 4)})
    else:
        for key in [k for k in args.cases.split(",") if k]:
            add_row(rows, measure(key, args.steps))
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
