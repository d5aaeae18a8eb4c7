"""Cost of one 1920 x 1080 volume image (ludwig_render_image: the scalar kernels of the field and k_render, one launch over all levels)
of each field, in ms on the device, beside the coarse-step time of the same levels.

Set-ups: ball1m on 3 levels and the 256^3 periodic box (the bench workload), each after 4 coarse steps from rest. Camera: perspective,
40 degrees, towards the domain's centre along (0.55, 0.45, -0.7) from 0.95 of its diagonal away, so that the domain about fills the
frame. The medium is thin (opacity 0.002 on `coolwarm`), so no ray ends as OPAQUE: every ray that meets the box marches through all of it or into the
body, the dearest image of the set-up at this step length (0.5) and size.
  image_ms           ludwig_render_image between two HIP events on the levels' stream (the null stream): for |u|, Q and |omega| this
                     includes the gradient fields and the scalar kernel of every level; the median of `--reps` after one warm-up
  download_ms        ludwig_render_download (host clock; 24 bytes per pixel)
  samples, ns_per_sample   the image's samples and image_ms over them
  rays               per end code
  step_ms            one coarse step of the same levels, HIP events around a batch of 10
usage: render_cost.py [--out FILE] [--cases ball1m,box] [--reps 5]  (default: print only)"""
import time

import numpy as np

from _cost_common import HipEvent, add_row, box_case, golden_case, parse_args, write_rows

WIDTH, HEIGHT = 1920, 1080
RANGES = {"density": (0.99, 1.01), "velocity_magnitude": (0.0, 0.1), "q_criterion": (-1.0e-4, 1.0e-4), "vorticity_magnitude": (0.0, 0.05)}


def camera(grids):
    from open_ludwig_amd import render as rd
    size = 8.0 * np.array(grids[0].block_pointer.shape, dtype=np.float64)
    d = np.array([0.55, 0.45, -0.7])
    d /= np.linalg.norm(d)
    centre = size / 2.0
    spec = {"type": "perspective", "position": (centre - 0.95 * np.linalg.norm(size) * d).tolist(), "look_at": centre.tolist(),
            "up": [0.0, 0.0, 1.0], "fov": 40.0}
    return rd.Camera.build(spec, WIDTH, HEIGHT).arrays()


def measure(key, reps):
    from open_ludwig_amd import adapt, execute_timestep_batch, render as rd
    if key == "box":
        name, grids, params, u = box_case()
    else:
        name, cfg, grids, _, _, params = golden_case(key)
        u = float(cfg.u_lattice)
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    execute_timestep_batch(dev, 1, 4, np.float32(u), params)
    e0, e1 = HipEvent(), HipEvent()
    e0.record()
    execute_timestep_batch(dev, 5, 10, np.float32(u), params)
    e1.record()
    step_ms = e0.elapsed_ms(e1) / 10.0
    t_coarse = 14
    r = rd.DeviceRender(dev, WIDTH * HEIGHT)
    cam, persp = camera(grids)
    scales, table = rd.level_scales(grids), rd.bake_table("coolwarm", 0.002)
    rows = []
    for field, (lo, hi) in RANGES.items():
        image = lambda: r.image(t_coarse, field, scales, cam, persp, WIDTH, HEIGHT, 0.5, lo, hi, 4096, table)
        image()
        _, codes, samples = r.download()                                    # the warm-up, and the figures of the row
        ms, down = [], []
        for _ in range(reps):
            e0.record()
            image()
            e1.record()
            ms.append(e0.elapsed_ms(e1))
            t0 = time.perf_counter()
            r.download()
            down.append((time.perf_counter() - t0) * 1e3)
        total = int(samples.astype(np.int64).sum())
        rows.append({"case": name, "cells": sum(512 * g.n_blocks for g in grids), "levels": len(grids), "field": field,
                     "width": WIDTH, "height": HEIGHT, "step": 0.5, "image_ms": round(float(np.median(ms)), 3),
                     "image_ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "download_ms": round(float(np.median(down)), 3),
                     "samples": total, "longest_ray": int(samples.max()), "ns_per_sample": round(float(np.median(ms)) * 1e6 / max(total, 1), 4),
                     "rays": {nm: int((codes == k).sum()) for k, nm in enumerate(rd.CODE_NAMES)}, "step_ms": round(step_ms, 3)})
    r.close()
    for d in dev:
        d.close()
    return rows


def main():
    args = parse_args("render_cost.py", ("--cases", {"default": "ball1m,box"}), ("--reps", {"type": int, "default": 5}))
    rows = []
    for key in [k for k in args.cases.split(",") if k]:
        for row in measure(key, args.reps):
            add_row(rows, row)
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
