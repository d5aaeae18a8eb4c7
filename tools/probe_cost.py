"""Cost of probes (ludwig_execute_timestep_batch_probes) per coarse step, on the device.

Cases: the 3-level ball1m sphere (Re 266k set-up; 64 probes: 48 in the wake, 16 next to the wall) and the 256^3 periodic box (one
level, the bench workload; 64 probes). Per case, one copy of the levels stepped on in four configurations, in alternation:
  off          no probe set (the finest level elides its rho store where it can)
  rho_store    no probe set, but every level stores rho after every step (what creating a probe set switches on)
  probes_1     a probe set sampled every coarse step
  probes_10    a probe set sampled every 10th coarse step
Every measurement is BATCHES batches of 8 coarse steps (run_case's async_depth), each ending in the library's own synchronisation,
with the ring drained after every batch as HipStepper does, bracketed by two HIP events on the levels' stream (the null stream; the events
see the host time between the synchronised batches too, as a run does). The medians of `--reps` alternating rounds, in ms per coarse step,
and the overhead of each against `off`; drain_ms_per_coarse_step is the host clock around the ring downloads alone (inside the
bracket).
usage: probe_cost.py [--out FILE] [--reps N]"""
import time

import numpy as np

from _cost_common import HipEvent, add_row, box_case, golden_case, parse_args, write_rows

BATCH, BATCHES = 8, 8


def ball1m_points():
    """48 wake points (x 0.6 .. 2.0 behind the sphere of radius 0.5, a 4 x 4 x 3 lattice) and 16 on a ring 0.1 (2.5 finest cells) off the wall"""
    pts = [[x, y, z] for x in (0.6, 1.0, 1.5, 2.0) for y in (-0.3, -0.1, 0.1, 0.3) for z in (-0.2, 0.0, 0.2)]
    r = 0.6
    pts += [[r * np.cos(a), r * np.sin(a) * 0.8, r * np.sin(a) * 0.6] for a in np.linspace(0, 2 * np.pi, 16, endpoint=False)]
    return np.array(pts)


def measure(name, grids, params, u, plan, reps):
    from open_ludwig_amd import adapt, execute_timestep_batch, probes as pm
    # ONE copy of the levels for every configuration: separate copies differ by a few % on their own (allocation placement)
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    sets = {"off": [None, False], "rho_store": [None, True], "probes_1": [pm.DeviceProbes(plan, dev, BATCH, 1, 1), True],
            "probes_10": [pm.DeviceProbes(plan, dev, BATCH, 1, 10), True]}
    t_next = [1]

    ev0, ev1 = HipEvent(), HipEvent()

    def run(key):
        """(device ms per coarse step, host ms per coarse step spent draining the ring)"""
        P, store = sets[key]
        for d in dev:
            d.set_rho_store(store)                          # off: the finest level may elide its rho store again
        t = t_next[0]
        dev[0].synchronize()
        drain = 0.0
        ev0.record()
        for _ in range(BATCHES):
            execute_timestep_batch(dev, t, BATCH, np.float32(u), params, probes=P)
            if P is not None:
                t1 = time.perf_counter()
                P.download()
                drain += time.perf_counter() - t1
            t += BATCH
        ev1.record()
        t_next[0] = t
        return ev0.elapsed_ms(ev1) / (BATCHES * BATCH), drain * 1e3 / (BATCHES * BATCH)

    for key in sets:                                        # warm-up: code objects, level streams
        run(key)
    times = {key: [] for key in sets}
    drains = {key: [] for key in sets if sets[key][0] is not None}
    for _ in range(reps):
        for key in sets:
            ms, dr = run(key)
            times[key].append(ms)
            if key in drains:
                drains[key].append(dr)
    med = {key: float(np.median(v)) for key, v in times.items()}
    res = {"case": name, "levels": len(grids), "blocks": [g.n_blocks for g in grids], "probes": plan.n,
           "probes_per_level": [int((plan.level == l).sum()) for l in range(len(grids))], "reps": reps,
           "ms_per_coarse_step": {k: round(v, 4) for k, v in med.items()},
           "overhead_vs_off_pct": {k: round(100.0 * (v / med["off"] - 1.0), 2) for k, v in med.items() if k != "off"},
           "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
           "drain_ms_per_coarse_step": {k: round(float(np.median(v)), 4) for k, v in drains.items()}}
    for P, _ in sets.values():
        if P is not None:
            P.close()
    for d in dev:
        d.close()
    return res


def main():
    args = parse_args("probe_cost.py", ("--reps", dict(type=int, default=9)))
    from open_ludwig_amd import probes as pm
    rows = []
    name, cfg, grids, _, phys, params = golden_case()
    plan = pm.plan_probes(ball1m_points(), grids, phys.mesh_offset)
    add_row(rows, measure(name, grids, params, cfg.u_lattice, plan, args.reps))
    name, grids, params, u = box_case()
    rng = np.random.default_rng(5)
    plan = pm.plan_probes(rng.uniform(8.0, 248.0, (64, 3)), grids)
    add_row(rows, measure(name, grids, params, u, plan, args.reps))
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
