"""Cost of the iso-surface extraction (ludwig_level_isosurface_extract: k_iso_count, the host scan, k_iso_emit) on the device, in ms,
beside ludwig_level_gradient_fields_compute on the same levels in the same process, and of a run_case output step with one Q surface
against the same step with a flow file.

Cases: the 256^3 periodic box (one level, the bench workload; the scalar is uploaded through rho: a small sphere that crosses few blocks,
diagonal waves that cross most) and every level of the 3-level ball1m sphere after a few coarse steps (Q at its 99.9th percentile: few
blocks; |u| at its median: most).
Per surface:
  triangles          the count
  count_ms           the count pass alone: the call with max_triangles = 0, which is refused after the counts reached the host
  extract_ms         count + scan + emit (no download)
  count_vs_gradient  count_ms over gradient_ms of the level (reported, not gated: the count pass moves about 7 B per cell, the gradient 38)
  download_ms        the three arrays to the host
Per level: gradient_ms, one ludwig_level_gradient_fields_compute alone, back to back.
run_case (ball1m): one batch of 8 steps with nothing at its end, with a flow file, and with one Q surface (extraction, download, weld, file).
--step-only: the ball1m coarse step alone, one JSON line (for alternating processes of two checkouts: the feature off against its parent).
Host clock around work that ends in a device synchronise; the medians of a few repetitions.
usage: isosurface_cost.py [--out FILE] [--step-only]  (default: print only)"""
import copy
import os
import shutil
import tempfile
import time

import numpy as np

from _cost_common import BALL, GOLDEN, add_row, box_case, golden_case, parse_args, timed, write_rows


def surface_rows(d, g, surfaces, gradient_ms, reps=5):
    rows = []
    scale = np.float32(1.0 / g.dx)
    for label, field, value in surfaces:
        n = d.isosurface(field, value, "vel", scale, download=False)[0]           # allocation, first launch
        count_ms = timed(lambda: d.isosurface(field, value, "vel", scale, max_triangles=0), d.synchronize, reps)
        extract_ms = timed(lambda: d.isosurface(field, value, "vel", scale, download=False), d.synchronize, reps)
        download_ms = timed(lambda: d.isosurface(field, value, "vel", scale), d.synchronize, 3) - extract_ms
        rows.append({"surface": label, "field": field, "value": float(value), "triangles": n, "count_ms": round(count_ms, 4),
                     "extract_ms": round(extract_ms, 4), "count_vs_gradient": round(count_ms / gradient_ms, 2),
                     "download_ms": round(download_ms, 3)})
    return rows


def gradient_ms(d, g, n_computes=20, reps=5):
    from open_ludwig_amd import _lib
    lib = _lib.load()
    scale = float(np.float32(1.0 / g.dx))

    def compute():
        for _ in range(n_computes):
            _lib.check(lib.ludwig_level_gradient_fields_compute(d.handle, _lib.VEL, scale))
    compute()
    return timed(compute, d.synchronize, reps) / n_computes


def measure_box():
    from open_ludwig_amd import adapt, cases
    name, grids, params, u = box_case()
    g = grids[0]
    d = adapt(g, 0, upload_state=False)
    d.init_equilibrium()
    gx, gy, gz = (np.asarray(c, dtype=np.float32) - 1 for c in cases.global_cell_coords(g))
    few = np.asfortranarray(-np.sqrt((gx - 127.3) ** 2 + (gy - 128.1) ** 2 + (gz - 126.6) ** 2))
    rows = []
    grad = gradient_ms(d, g)
    d.upload("rho", few)
    rows += surface_rows(d, g, [("sphere r = 6: few blocks", "density", -6.0)], grad)
    most = np.asfortranarray(np.sin((2 * np.pi / 24) * (gx + gy + gz)).astype(np.float32))
    d.upload("rho", most)
    rows += surface_rows(d, g, [("diagonal waves, period 24: most blocks", "density", 0.05)], grad)
    d.close()
    return {"case": name, "levels": [{"level": 1, "blocks": g.n_blocks, "cells": 512 * g.n_blocks, "gradient_ms": round(grad, 4),
                                      "surfaces": rows}]}


def ball_step_ms(n_steps=20, reps=5):
    from open_ludwig_amd import adapt, execute_timestep_batch
    name, cfg, grids, _, _, params = golden_case()
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    execute_timestep_batch(dev, 1, 4, np.float32(cfg.u_lattice), params)
    ms = timed(lambda: execute_timestep_batch(dev, 5, n_steps, np.float32(cfg.u_lattice), params), dev[0].synchronize, reps) / n_steps
    return name, cfg, grids, params, dev, ms


def measure_ball():
    from open_ludwig_amd import isosurface as iso
    name, cfg, grids, params, dev, step_ms = ball_step_ms()
    skips = iso.skip_flags(grids)
    levels = []
    for li, (g, d) in enumerate(zip(grids, dev)):
        grad = gradient_ms(d, g)
        vel = d.download("vel")
        _, q = d.gradient_fields("vel", np.float32(1.0 / g.dx))
        fluid = ~g.obstacle
        speed = iso.scalar_host("velocity_magnitude", None, vel, None, None)
        surfaces = [("Q at its 99.9th percentile: few blocks", "q_criterion", np.float32(np.percentile(q[fluid], 99.9))),
                    ("|u| at its median: most blocks", "velocity_magnitude", np.float32(np.median(speed[fluid])))]
        levels.append({"level": g.level_id, "blocks": g.n_blocks, "cells": 512 * g.n_blocks, "exported_blocks": int((skips[li] == 0).sum()),
                       "gradient_ms": round(grad, 4), "surfaces": surface_rows(d, g, surfaces, grad)})
    for d in dev:
        d.close()
    return {"case": name, "step_ms": round(step_ms, 4), "levels": levels}


def run_case_output_step(reps=3):
    """one run_case batch of 8 steps: nothing at its end, a flow file at its end, one Q surface at its end (ball1m, 3 levels)"""
    from open_ludwig_amd import case, preprocess as pp
    base = pp.load_case_configuration(os.path.join(GOLDEN, "ball1m_config.yaml"), BALL)
    base.diag_freq, base.output_freq = 8, 1000
    flow = copy.copy(base)
    flow.output_freq = 8
    flow.output_fields = base.output_fields + ("QCriterion",)
    # the surface's value: the 99th percentile of Q on the finest level after those 8 steps
    from open_ludwig_amd.solver_control import ramp_velocity
    _, _, grids, _, _, sp = golden_case()
    st = case.HipStepper(grids)
    st.batch(1, 8, ramp_velocity(8, base.ramp_steps, base.u_lattice), sp)
    fin = len(grids) - 1
    q = st.gradient_fields(fin, "vel", np.float32(1.0 / grids[fin].dx))[1]
    value = float(np.percentile(q[~grids[fin].obstacle], 99))
    st.close()
    over = copy.deepcopy(BALL)
    over["advanced"] = {"isosurfaces": {"enabled": True, "start_step": 8, "interval": 8,
                                        "surfaces": [{"name": "q", "field": "q_criterion", "value": value}]}}
    surf = pp.load_case_configuration(os.path.join(GOLDEN, "ball1m_config.yaml"), over)
    surf.diag_freq, surf.output_freq = 8, 1000
    setup = pp.setup_multilevel_domain(base, os.path.join(GOLDEN, "ball1m.stl"))
    res, sizes = {}, {}
    for label, c in (("plain", base), ("flow", flow), ("surface", surf)) * 2:      # the first round is the warm-up
        times = []
        for _ in range(reps):
            d = tempfile.mkdtemp()
            t0 = time.perf_counter()
            case.run_case(c, case.HipStepper, steps=8, setup=setup, out_dir=d)
            times.append((time.perf_counter() - t0) * 1e3)
            sizes[label] = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.startswith(("flow_", "iso_")))
            shutil.rmtree(d)
        res[label] = float(np.median(times))
    return {"case": "run_case ball1m, 8 steps, output at step 8", "cells": sum(512 * gr.n_blocks for gr in setup[0]), "q_value": value,
            "plain_ms": round(res["plain"], 1), "flow_file_ms": round(res["flow"], 1), "q_surface_ms": round(res["surface"], 1),
            "flow_file_extra_ms": round(res["flow"] - res["plain"], 1), "q_surface_extra_ms": round(res["surface"] - res["plain"], 1),
            "flow_file_bytes": sizes["flow"], "q_surface_bytes": sizes["surface"]}


def main():
    args = parse_args("isosurface_cost.py", ("--step-only", {"action": "store_true"}))
    rows = []
    if args.step_only:
        name, _, _, _, dev, ms = ball_step_ms()
        for d in dev:
            d.close()
        add_row(rows, {"case": name, "step_ms": round(ms, 4)})
    else:
        add_row(rows, measure_box())
        add_row(rows, measure_ball())
        add_row(rows, run_case_output_step())
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
