"""Cost of the force series (ludwig_execute_timestep_batch_loads with a force-series set) per coarse step, on the device.

Cases: the 3-level ball1m sphere (Re 266k set-up, 20 480 triangles) and the wing at surface resolution 200 (3 levels, 63 196
triangles), each with its own STL's triangles on the finest level. Per case, ONE copy of the levels stepped on in four
configurations, in alternation:
  off          no set (the finest level elides its rho store where it can)
  rho_store    no set, but the finest level stores rho after every step (what creating a set switches on)
  series_1     a force series sampled every coarse step
  series_10    a force series sampled every 10th coarse step
  run_case_1   series_1 with run_case's host work after every batch on top: the drained records go through force_series.Series
               (append, take_new), forces.finish_forces and force_series.csv_row, and the rows are written to a file
Every measurement is BATCHES batches of 8 coarse steps (run_case's async_depth), each ending in the library's own synchronisation and,
with a set, in the drain of its ring (as HipStepper.batch does), bracketed by two HIP events on the levels' stream (the null stream;
the events see the host time between the synchronised batches too, as a run does). The medians of `--reps` alternating rounds, in ms
per coarse step, and the overhead of each against `off`.
--step-only: the coarse step of the first case alone, nothing of the feature made (the key off), host clock around synchronised
batches of 8; --root DIR takes the package and its library from another checkout of the project (the parent commit, built there), so
that two builds can be compared, a process each, in alternation.
usage: force_series_cost.py [--out FILE] [--reps N] [--cases ball1m,wing] [--step-only [--root DIR]]"""
import sys

import numpy as np

from _cost_common import HipEvent, add_row, golden_case, parse_args, timed, write_rows

if "--root" in sys.argv:                                    # ahead of the first import of the package
    sys.path.insert(0, sys.argv[sys.argv.index("--root") + 1])

BATCH, BATCHES = 8, 8


def measure(name, grids, mesh, phys, params, u, reps):
    import os
    from open_ludwig_amd import adapt, execute_timestep_batch, force_series as fs, forces, surface_stats as ss
    # ONE copy of the levels for every configuration: separate copies differ by a few % on their own (allocation placement)
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    fin = len(grids) - 1
    plan = ss.plan_surface(mesh, grids[fin], phys)
    sets = {"off": [None, False], "rho_store": [None, True],
            "series_1": [fs.from_mesh(mesh, plan, dev[fin], fin, grids[fin].tau, phys, 1, 1, BATCH), True],
            "series_10": [fs.from_mesh(mesh, plan, dev[fin], fin, grids[fin].tau, phys, 1, 10, BATCH), True],
            "run_case_1": [fs.from_mesh(mesh, plan, dev[fin], fin, grids[fin].tau, phys, 1, 1, BATCH), True]}
    series, sink = fs.Series(), open(os.devnull, "w")
    taken = {k: 0 for k, (F, _) in sets.items() if F is not None}
    t_next = [1]
    ev0, ev1 = HipEvent(), HipEvent()

    def run(key):
        F, store = sets[key]
        dev[fin].set_rho_store(store)                       # off: the finest level may elide its rho store again
        t = t_next[0]
        dev[0].synchronize()
        ev0.record()
        for _ in range(BATCHES):
            execute_timestep_batch(dev, t, BATCH, np.float32(u), params, forces=F)
            if F is not None:
                got = F.download()
                taken[key] += got[0].size
                if key == "run_case_1":
                    series.append(*got)
                    for step, sums, cov in zip(*series.take_new()):
                        fr = forces.finish_forces(sums, int(cov), phys, False)
                        sink.write(fs.csv_row(int(step), float(step) * phys.time_scale, fr, u) + "\n")
            t += BATCH
        ev1.record()
        t_next[0] = t
        return ev0.elapsed_ms(ev1) / (BATCHES * BATCH)

    for key in sets:                                        # warm-up: code objects, level streams
        run(key)
    times = {key: [] for key in sets}
    for _ in range(reps):
        for key in sets:
            times[key].append(run(key))
    med = {key: float(np.median(v)) for key, v in times.items()}
    res = {"case": name, "levels": len(grids), "blocks": [g.n_blocks for g in grids], "triangles": plan.n,
           "triangles_found": int(plan.found.sum()), "reps": reps, "records_taken": taken,
           "ms_per_coarse_step": {k: round(v, 4) for k, v in med.items()},
           "overhead_vs_off_pct": {k: round(100.0 * (v / med["off"] - 1.0), 2) for k, v in med.items() if k != "off"},
           "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}}
    sink.close()
    for F, _ in sets.values():
        if F is not None:
            F.close()
    for d in dev:
        d.close()
    return res


def step_only(name, grids, params, u, reps):
    import open_ludwig_amd
    from open_ludwig_amd import adapt, build, execute_timestep_batch
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    t = [1]

    def steps():
        for _ in range(BATCHES):
            execute_timestep_batch(dev, t[0], BATCH, np.float32(u), params)
            t[0] += BATCH
    steps()                                                 # warm-up: code objects, level streams
    ms = [timed(steps, dev[0].synchronize, 1) / (BATCH * BATCHES) for _ in range(reps)]
    for d in dev:
        d.close()
    return {"case": name, "package": open_ludwig_amd.__file__, "sources": build.source_digest(), "reps": reps,
            "step_ms": round(float(np.median(ms)), 4), "spread_ms": [round(min(ms), 4), round(max(ms), 4)]}


def main():
    args = parse_args("force_series_cost.py", ("--reps", dict(type=int, default=9)), ("--cases", dict(default="ball1m,wing")),
                      ("--step-only", dict(action="store_true")), ("--root", dict(default=None)))
    rows = []
    if args.step_only:
        name, cfg, grids, mesh, phys, params = golden_case(args.cases.split(",")[0])
        add_row(rows, step_only(name, grids, params, cfg.u_lattice, args.reps))
        write_rows(rows, args.out)
        return
    for key in args.cases.split(","):
        name, cfg, grids, mesh, phys, params = golden_case(key)
        add_row(rows, measure(name, grids, mesh, phys, params, cfg.u_lattice, args.reps))
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
