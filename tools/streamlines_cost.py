"""Cost of a streamline trace (ludwig_streamlines_trace: k_streamlines, one launch over all levels) and of its download on the device,
in ms, and of a run_case batch that ends with one streamline group against the same batch with a flow file and with no output.

Rake: 1 024 seeds (32 x 32) in the plane two coarse cells upstream of the finest level's box, spanning it in y and z, forward,
step 0.5, max_steps 2000, on ball1m (3 levels) and on the wing at surface resolution 200 (--cases). The levels' velocity buffers hold an
uploaded uniform field u = (0.05, 0.004, 0.002), rho = 1: a trace is a latency chain whose length is the number of steps, not a function
of the values, and the start-up field of a few coarse steps is at rest where the lines would run.
  lines, vertices    the count of each; ended_by: lines per end code
  trace_ms           the launch alone, to the device synchronise
  download_ms        counts, codes and the first max(count) records of every line to the host
  ns_per_step        trace_ms over the longest line's steps: the latency of one step (two samples) of the chain
run_case (ball1m): one batch of 8 steps with nothing at its end, with a flow file, and with one streamline group (trace, download, file).
--step-only: the ball1m coarse step alone, one JSON line (for alternating processes of two checkouts: the feature off against its parent).
Host clock around work that ends in a device synchronise; the medians of 5 repetitions.
usage: streamlines_cost.py [--out FILE] [--cases ball1m,wing] [--step-only]  (default: print only)"""
import copy
import os
import shutil
import tempfile
import time

import numpy as np

from _cost_common import BALL, GOLDEN, add_row, golden_case, parse_args, timed, write_rows

U = (0.05, 0.004, 0.002)
N_SIDE, MAX_STEPS, STEP, MIN_SPEED = 32, 2000, 0.5, 1.0e-6


def rake(grids):
    """N_SIDE x N_SIDE positions (cell units of level 1) in the plane two coarse cells upstream of the finest level's box"""
    fin = grids[-1]
    c = np.asarray(fin.active_block_coords).reshape(-1, 3)
    s = 8.0 / 2 ** (len(grids) - 1)
    lo, hi = (c.min(axis=0) - 1) * s, c.max(axis=0) * s
    y = np.linspace(lo[1] + 0.25, hi[1] - 0.25, N_SIDE)
    z = np.linspace(lo[2] + 0.25, hi[2] - 0.25, N_SIDE)
    yy, zz = np.meshgrid(y, z, indexing="ij")
    return np.stack([np.full(yy.size, max(lo[0] - 2.0, 1.0)), yy.reshape(-1), zz.reshape(-1)], axis=1).astype(np.float32)


def measure_rake(key, reps=5):
    from open_ludwig_amd import adapt, streamlines as sl
    name, cfg, grids, _, _, params = golden_case(key)
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d, g in zip(dev, grids):
        d.init_equilibrium()
        v = np.empty((8, 8, 8, g.n_blocks, 3), np.float32, order="F")
        v[...] = np.asarray(U, dtype=np.float32)
        d.upload("vel", v)
        d.upload("vel_temp", v)
        del v
    seeds = rake(grids)
    s = sl.DeviceStreamlines(dev, seeds, np.ones(len(seeds), np.float32), STEP, MIN_SPEED, MAX_STEPS)
    s.trace(1)
    counts, codes, _ = s.download()                                         # first launch, and the figures of the row
    sync = dev[0].synchronize
    trace_ms = timed(lambda: s.trace(1), sync, reps)
    both_ms = timed(lambda: (s.trace(1), s.download()), sync, reps)
    s.close()
    for d in dev:
        d.close()
    return {"case": name, "cells": sum(512 * g.n_blocks for g in grids), "levels": len(grids), "lines": int(len(seeds)),
            "max_steps": MAX_STEPS, "vertices": int(counts.sum()), "longest": int(counts.max()),
            "ended_by": {nm: int((codes == k).sum()) for k, nm in enumerate(("max_steps", "outside", "obstacle", "slow"))},
            "trace_ms": round(trace_ms, 3), "download_ms": round(both_ms - trace_ms, 3),
            "ns_per_step": round(trace_ms * 1e6 / max(int(counts.max()) - 1, 1), 1)}


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


def run_case_output_step(reps=5):
    """one run_case batch of 8 steps: nothing at its end, a flow file at its end, one streamline group at its end (ball1m, 3 levels)"""
    from open_ludwig_amd import case, preprocess as pp
    base = pp.load_case_configuration(os.path.join(GOLDEN, "ball1m_config.yaml"), BALL)
    base.diag_freq, base.output_freq = 8, 1000
    flow = copy.copy(base)
    flow.output_freq = 8
    setup = pp.setup_multilevel_domain(base, os.path.join(GOLDEN, "ball1m.stl"))
    grids, _, phys, _ = setup
    # the rake of measure_rake as a seed group, in the STL frame
    pts = rake(grids).astype(np.float64) * grids[0].dx - np.asarray(phys.mesh_offset, dtype=np.float64)
    over = copy.deepcopy(BALL)
    over["advanced"] = {"streamlines": {"enabled": True, "start_step": 8, "interval": 8, "step": STEP, "max_steps": MAX_STEPS,
                                        "min_speed": MIN_SPEED, "direction": "forward",
                                        "seeds": [{"name": "rake", "points": pts.tolist()}]}}
    lines = pp.load_case_configuration(os.path.join(GOLDEN, "ball1m_config.yaml"), over)
    lines.diag_freq, lines.output_freq = 8, 1000
    res, sizes, log = {}, {}, []
    for label, c in (("plain", base), ("flow", flow), ("lines", lines)) * 2:       # the first round is the warm-up
        times = []
        for _ in range(reps if label != "flow" else 3):
            d = tempfile.mkdtemp()
            t0 = time.perf_counter()
            case.run_case(c, case.HipStepper, steps=8, setup=setup, out_dir=d, log=log.append)
            times.append((time.perf_counter() - t0) * 1e3)
            sizes[label] = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.startswith(("flow_", "stream_")))
            shutil.rmtree(d)
        res[label] = float(np.median(times))
    return {"case": "run_case ball1m, 8 steps, output at step 8", "cells": sum(512 * gr.n_blocks for gr in grids), "lines": len(pts),
            "sample": next((l for l in reversed(log) if l.startswith("streamlines")), ""),
            "plain_ms": round(res["plain"], 1), "flow_file_ms": round(res["flow"], 1), "streamlines_ms": round(res["lines"], 1),
            "flow_file_extra_ms": round(res["flow"] - res["plain"], 1), "streamlines_extra_ms": round(res["lines"] - res["plain"], 1),
            "flow_file_bytes": sizes["flow"], "streamlines_bytes": sizes["lines"]}


def main():
    args = parse_args("streamlines_cost.py", ("--step-only", {"action": "store_true"}), ("--cases", {"default": "ball1m,wing"}),
                      ("--no-run-case", {"action": "store_true"}))
    rows = []
    if args.step_only:
        name, ms = ball_step_ms()
        add_row(rows, {"case": name, "step_ms": round(ms, 4)})
    else:
        for key in [k for k in args.cases.split(",") if k]:
            add_row(rows, measure_rake(key))
        if not args.no_run_case:
            add_row(rows, run_case_output_step())
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
