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
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

BATCH, BATCHES = 8, 8


def ball1m_points():
    """48 wake points (x 0.6 .. 2.0 behind the sphere of radius 0.5, a 4 x 4 x 3 lattice) and 16 on a ring 0.1 (2.5 finest cells) off the wall"""
    pts = [[x, y, z] for x in (0.6, 1.0, 1.5, 2.0) for y in (-0.3, -0.1, 0.1, 0.3) for z in (-0.2, 0.0, 0.2)]
    r = 0.6
    pts += [[r * np.cos(a), r * np.sin(a) * 0.8, r * np.sin(a) * 0.6] for a in np.linspace(0, 2 * np.pi, 16, endpoint=False)]
    return np.array(pts)


class _HipEvent:
    """a hipEvent_t of the HIP runtime libludwig_hip.so runs on, recorded on the null stream (the levels' stream here)"""

    def __init__(self):
        import ctypes as C
        from open_ludwig_amd import _lib
        _lib.load()
        path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)   # the runtime the library loaded
        self.C, self.hip = C, C.CDLL(path)
        self.ev = C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.ev)) == 0

    def record(self):
        assert self.hip.hipEventRecord(self.ev, None) == 0

    def elapsed_ms(self, end) -> float:
        assert self.hip.hipEventSynchronize(end.ev) == 0
        ms = self.C.c_float()
        assert self.hip.hipEventElapsedTime(self.C.byref(ms), self.ev, end.ev) == 0
        return float(ms.value)


def measure(name, grids, params, u, plan, reps):
    from open_ludwig_amd import adapt, execute_timestep_batch, probes as pm
    # ONE copy of the levels for every configuration: separate copies differ by a few % on their own (allocation placement)
    dev = [adapt(g, 0, upload_state=False) for g in grids]
    for d in dev:
        d.init_equilibrium()
    sets = {"off": [None, False], "rho_store": [None, True], "probes_1": [pm.DeviceProbes(plan, dev, BATCH, 1, 1), True],
            "probes_10": [pm.DeviceProbes(plan, dev, BATCH, 1, 10), True]}
    t_next = [1]

    ev0, ev1 = _HipEvent(), _HipEvent()

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
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    from open_ludwig_amd import _lib, cases, preprocess as pp, probes as pm
    if _lib.device_count() < 1:
        raise SystemExit("probe_cost.py needs a GPU")
    rows = []
    g = os.path.join(ROOT, "tests", "golden")
    cfg = pp.load_case_configuration(os.path.join(g, "ball1m_config.yaml"), {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}}})
    grids, _, phys, _ = pp.setup_multilevel_domain(cfg, os.path.join(g, "ball1m.stl"))
    plan = pm.plan_probes(ball1m_points(), grids, phys.mesh_offset)
    rows.append(measure("ball1m sphere, 3 levels (Re 266k setup)", grids, pp.solver_params(cfg, phys), cfg.u_lattice, plan, args.reps))
    print(json.dumps(rows[-1]), flush=True)
    grids, params = cases.periodic_box((32, 32, 32), init=False)
    rng = np.random.default_rng(5)
    plan = pm.plan_probes(rng.uniform(8.0, 248.0, (64, 3)), grids)
    rows.append(measure("periodic 256^3", grids, params, 0.0, plan, args.reps))
    print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
