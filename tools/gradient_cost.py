"""Cost of the velocity-gradient fields (ludwig_level_gradient_fields_compute, k_velocity_gradient_fields) on the device, in ms and GB/s,
and of an output step of run_case with the Vorticity / QCriterion arrays on and off.

Cases: the 256^3 periodic box (one level, the bench workload) and every level of the 3-level ball1m sphere.
Per level:
  compute_ms     one compute alone, back to back on the level's stream (no download)
  compute_GBps   BYTES_PER_CELL x owned cells / compute_ms
  download_ms    both downloads to the host (reference layout), for comparison
Per case: step_ms, one coarse step (mean over a batch).
run_case (ball1m): one batch of 8 steps ending in an output step (flow + surface VTU, forces), fields off and on; the difference is
what the two arrays cost an output step, device pass, downloads and file included.
BYTES_PER_CELL = 12 (own velocity) + 9 (the six face layers: 6 x 64 cells x 12 B / 512) + 1 (obstacle) + 16 (written) = 38.
Host clock around work that ends in a device synchronise; the medians of a few repetitions.
usage: gradient_cost.py [--out FILE]  (default: print only)"""
import copy
import os
import shutil
import tempfile
import time

import numpy as np

from _cost_common import BALL, GOLDEN, add_row, box_case, golden_case, parse_args, timed, write_rows

BYTES_PER_CELL = 12 + 9 + 1 + 16


def measure(name, grids, params, u, n_steps=20, n_computes=20, reps=5):
    from open_ludwig_amd import _lib, adapt, execute_timestep_batch
    lib = _lib.load()
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    sync = dev[0].synchronize
    execute_timestep_batch(dev, 1, 4, np.float32(u), params)            # warm-up: code objects, level streams, a flow
    step_ms = timed(lambda: execute_timestep_batch(dev, 5, n_steps, np.float32(u), params), sync, reps) / n_steps
    levels = []
    for g, d in zip(grids, dev):
        scale = float(np.float32(1.0 / g.dx))

        def compute():
            for _ in range(n_computes):
                _lib.check(lib.ludwig_level_gradient_fields_compute(d.handle, _lib.VEL, scale))
        compute()                                                        # allocation, first launch
        ms = timed(compute, sync, reps) / n_computes
        dl = timed(lambda: d.gradient_fields("vel", scale), sync, reps)
        cells = 512 * g.n_blocks
        levels.append({"level": g.level_id, "blocks": g.n_blocks, "cells": cells, "compute_ms": round(ms, 4),
                       "compute_GBps": round(BYTES_PER_CELL * cells / (ms * 1e-3) / 1e9, 1),
                       "compute_and_download_ms": round(dl, 3)})
    for d in dev:
        d.close()
    return {"case": name, "levels": levels, "step_ms": round(step_ms, 4),
            "compute_all_levels_ms": round(sum(l["compute_ms"] for l in levels), 4)}


def run_case_output_step(reps=3):
    """one run_case batch of 8 steps with an output step at its end, Vorticity / QCriterion off and on (ball1m, 3 levels)"""
    from open_ludwig_amd import case, preprocess as pp
    cfg = pp.load_case_configuration(os.path.join(GOLDEN, "ball1m_config.yaml"), BALL)
    cfg.diag_freq = cfg.output_freq = 8
    on = copy.copy(cfg)
    on.output_fields = cfg.output_fields + ("Vorticity", "QCriterion")
    setup = pp.setup_multilevel_domain(cfg, os.path.join(GOLDEN, "ball1m.stl"))
    res = {}
    for label, c in (("off", cfg), ("on", on), ("off", cfg), ("on", on)):       # the first pair is the warm-up
        times = []
        for _ in range(reps):
            d = tempfile.mkdtemp()
            t0 = time.perf_counter()
            case.run_case(c, case.HipStepper, steps=8, setup=setup, out_dir=d)
            times.append((time.perf_counter() - t0) * 1e3)
            shutil.rmtree(d)
        res[label] = float(np.median(times))
    return {"case": "run_case ball1m, 8 steps, output at step 8", "cells": sum(512 * gr.n_blocks for gr in setup[0]),
            "fields_off_ms": round(res["off"], 1), "fields_on_ms": round(res["on"], 1), "output_step_extra_ms": round(res["on"] - res["off"], 1)}


def main():
    args = parse_args("gradient_cost.py")
    rows = []
    add_row(rows, measure(*box_case()))
    name, cfg, grids, _, _, params = golden_case()
    add_row(rows, measure(name, grids, params, cfg.u_lattice))
    add_row(rows, run_case_output_step())
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
