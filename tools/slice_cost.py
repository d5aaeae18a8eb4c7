"""Cost of slices (ludwig_slices_*) per coarse step, on the device, of writing one slice file, and of a run_case output step.

Cases: the 3-level ball1m sphere (Re 266k set-up) with one y-normal plane through the sphere's centre of 1024 x 512 points (x -1.0 ..
4.0, z -1.25 .. 1.25 in the STL frame, h = 5 / 1023), and the wing at surface resolution 200 (3 levels) with one y-normal plane
across the middle of the domain, 1024 points along its longer in-plane axis; all five fields. One copy of the levels is stepped on in three
configurations, in alternation:
  off          no sampling
  slices_1     the plane sampled and downloaded after every coarse step (batches of 1, as run_case cuts them at interval 1)
  slices_10    sampled after every 10th coarse step (batches of 10)
`off` runs in batches of 10. Every measurement is 40 coarse steps on the host clock around synchronised batches; medians of `--reps`
alternating rounds, in ms per coarse step, and the overhead against `off`. Also: the plan's host time, the sample + download time
alone, and the time to write one VTI file (zlib on the host).
run_case (ball1m, 8 coarse steps, one batch, forces and diagnostics on): wall time with no output, with one flow-file output step
(flow_%06d.vtu + surface_%06d.vtu at step 8), and with one slice output step (the plane above at step 8); the differences against no
output are the cost of each output step.
usage: slice_cost.py [--out FILE] [--reps N] [--cases ball1m,wing] [--run-case 0|1]"""
import os
import tempfile
import time

import numpy as np

from _cost_common import BALL, GOLDEN, add_row, golden_case, parse_args, write_rows

STEPS = 40


def plane_of(key, grids, phys):
    from open_ludwig_amd import preprocess as pp
    if key == "ball1m":
        return pp.SlicePlane("wake", 1, 0.0, ((-1.0, 4.0), (-1.25, 1.25)), 5.0 / 1023, pp.SLICE_FIELDS)
    l1 = grids[0]
    ext = np.array([l1.grid_dim_x, l1.grid_dim_y, l1.grid_dim_z], dtype=np.float64) * 8 * float(l1.dx)
    off = np.asarray(phys.mesh_offset, dtype=np.float64)
    return pp.SlicePlane("mid", 1, float(ext[1] / 2 - off[1]), None, float(max(ext[0], ext[2]) / 1023), pp.SLICE_FIELDS)


def run_case_cost(reps):
    """(seconds without output, with one flow-file output step, with one slice output step), medians of reps runs of ball1m"""
    from open_ludwig_amd import case, preprocess as pp
    g = GOLDEN
    plane = {"name": "wake", "normal": "y", "position": 0.0, "bounds": [[-1.0, 4.0], [-1.25, 1.25]], "spacing": 5.0 / 1023,
             "fields": ["density", "velocity", "velocity_magnitude", "vorticity", "q_criterion"]}
    runs = {"none": (10**6, False), "flow": (8, False), "slice": (10**6, True)}
    out = {k: [] for k in runs}
    for _ in range(reps):
        for k, (freq, on) in runs.items():
            over = {"basic": {**BALL["basic"], "simulation": {"steps": 8, "output_freq": freq}},
                    "advanced": {"diagnostics": {"freq": 8}, "gpu": {"async_depth": 8},
                                 "slices": {"enabled": on, "start_step": 8, "interval": 1000, "planes": [plane]}}}
            cfg = pp.load_case_configuration(os.path.join(g, "ball1m_config.yaml"), over)
            setup = pp.setup_multilevel_domain(cfg, os.path.join(g, "ball1m.stl"))
            with tempfile.TemporaryDirectory() as d:
                t1 = time.perf_counter()
                case.run_case(cfg, case.HipStepper, setup=setup, out_dir=d)
                out[k].append(time.perf_counter() - t1)
    return {k: round(float(np.median(v)), 3) for k, v in out.items()}


def measure(key, reps):
    from open_ludwig_amd import case, slices as sl
    name, cfg, grids, _, phys, params = golden_case(key)
    spec = plane_of(key, grids, phys)
    t0 = time.perf_counter()
    plan = sl.plan_slice(spec, grids, phys.mesh_offset)
    plan_s = time.perf_counter() - t0
    st = case.HipStepper(grids)
    st.slices_setup([plan])
    t_next = [1]
    u = np.float32(cfg.u_lattice)

    def run(key):
        per = 1 if key == "slices_1" else 10
        t = t_next[0]
        st.dev[0].synchronize()
        t1 = time.perf_counter()
        for _ in range(STEPS // per):
            st.batch(t, per, u, params)
            if key != "off":
                st.slices_sample(t + per - 1)
            t += per
        st.dev[0].synchronize()
        t_next[0] = t
        return (time.perf_counter() - t1) * 1e3 / STEPS

    keys = ("off", "slices_1", "slices_10")
    for k in keys:
        run(k)                                             # warm-up
    times = {k: [] for k in keys}
    for _ in range(reps):
        for k in keys:
            times[k].append(run(k))
    med = {k: float(np.median(v)) for k, v in times.items()}
    samp = []
    for _ in range(20):
        st.dev[0].synchronize()
        t1 = time.perf_counter()
        vals = st.slices_sample(t_next[0] - 1)
        samp.append((time.perf_counter() - t1) * 1e3)
    with tempfile.TemporaryDirectory() as d:
        w = sl.SliceWriter(d, [plan], phys.time_scale)
        t1 = time.perf_counter()
        w.write(t_next[0] - 1, vals)
        write_ms = (time.perf_counter() - t1) * 1e3
        size = os.path.getsize(os.path.join(d, sl.slice_file_name(spec.name, t_next[0] - 1)))
    st.close()
    res = {"case": name, "blocks": [g.n_blocks for g in grids], "plane": list(plan.dims),
           "points": plan.n, "valid": int(plan.valid.sum()), "points_per_level": [int((plan.valid & (plan.level == l)).sum()) for l in range(len(grids))],
           "plan_host_s": round(plan_s, 3), "reps": reps, "ms_per_coarse_step": {k: round(v, 4) for k, v in med.items()},
           "overhead_vs_off_pct": {k: round(100.0 * (v / med["off"] - 1.0), 2) for k, v in med.items() if k != "off"},
           "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
           "sample_and_download_ms": round(float(np.median(samp)), 3), "write_vti_ms": round(write_ms, 1), "vti_bytes": size}
    return res


def main():
    args = parse_args("slice_cost.py", ("--reps", dict(type=int, default=7)), ("--cases", dict(default="ball1m,wing")),
                      ("--run-case", dict(type=int, default=1)))
    rows = []
    for key in args.cases.split(","):
        add_row(rows, measure(key, args.reps))
    if args.run_case:
        t = run_case_cost(3)
        add_row(rows, {"case": "ball1m run_case, 8 coarse steps", "wall_s": t,
                       "flow_output_step_s": round(t["flow"] - t["none"], 3), "slice_output_step_s": round(t["slice"] - t["none"], 3)})
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
