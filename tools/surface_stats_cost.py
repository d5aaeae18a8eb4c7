"""Cost of surface statistics (ludwig_execute_timestep_batch_sampled with a surface set) per coarse step, on the device.

Cases: the 3-level ball1m sphere (Re 266k set-up) and the wing at surface resolution 200 (3 levels), each with its own STL's
triangles on the finest level. Per case, one copy of the levels stepped on in four configurations, in alternation:
  off          no surface set (the finest level elides its rho store where it can)
  rho_store    no surface set, but the finest level stores rho after every step (what creating a set switches on)
  surface_1    a surface set sampled every coarse step
  surface_10   a surface set sampled every 10th coarse step
Every measurement is BATCHES batches of 8 coarse steps (run_case's async_depth), each ending in the library's own synchronisation,
bracketed by two HIP events on the levels' stream (the null stream; the events see the host time between the synchronised batches
too, as a run does). The medians of `--reps` alternating rounds, in ms per coarse step, and the overhead of each against `off`.
usage: surface_stats_cost.py [--out FILE] [--reps N] [--cases ball1m,wing]"""
import numpy as np

from _cost_common import HipEvent, add_row, golden_case, parse_args, write_rows

BATCH, BATCHES = 8, 8


def measure(name, grids, mesh, phys, params, u, reps):
    from open_ludwig_amd import adapt, execute_timestep_batch, surface_stats as ss
    # ONE copy of the levels for every configuration: separate copies differ by a few % on their own (allocation placement)
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    fin = len(grids) - 1
    plan = ss.plan_surface(mesh, grids[fin], phys)
    sets = {"off": [None, False], "rho_store": [None, True],
            "surface_1": [ss.DeviceSurfaceStats(plan, dev[fin], fin, grids[fin].tau, phys, 1, 1), True],
            "surface_10": [ss.DeviceSurfaceStats(plan, dev[fin], fin, grids[fin].tau, phys, 1, 10), True]}
    t_next = [1]
    ev0, ev1 = HipEvent(), HipEvent()

    def run(key):
        S, store = sets[key]
        dev[fin].set_rho_store(store)                       # off: the finest level may elide its rho store again
        t = t_next[0]
        dev[0].synchronize()
        ev0.record()
        for _ in range(BATCHES):
            execute_timestep_batch(dev, t, BATCH, np.float32(u), params, surface=S)
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
    n_samples = {k: S.download()[1] for k, (S, _) in sets.items() if S is not None}
    res = {"case": name, "levels": len(grids), "blocks": [g.n_blocks for g in grids], "triangles": plan.n,
           "triangles_found": int(plan.found.sum()), "reps": reps, "samples_taken": n_samples,
           "ms_per_coarse_step": {k: round(v, 4) for k, v in med.items()},
           "overhead_vs_off_pct": {k: round(100.0 * (v / med["off"] - 1.0), 2) for k, v in med.items() if k != "off"},
           "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}}
    for S, _ in sets.values():
        if S is not None:
            S.close()
    for d in dev:
        d.close()
    return res


def main():
    args = parse_args("surface_stats_cost.py", ("--reps", dict(type=int, default=9)), ("--cases", dict(default="ball1m,wing")))
    rows = []
    for key in args.cases.split(","):
        name, cfg, grids, mesh, phys, params = golden_case(key)
        add_row(rows, measure(name, grids, mesh, phys, params, cfg.u_lattice, args.reps))
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
