"""Does grid sequencing pay on ball1m? The case at half its surface resolution from rest, then at its own resolution twice: from rest
(cold) and warm-started from the half-resolution run's last state (advanced.state_files / advanced.initial_condition, warm_start.py).

  coarse   surface_resolution // 2, ramp_steps / 2 and steps / 2 coarse steps (its time step is twice as long: the same physical time),
           one state file after the last step
  cold     the case as shipped, `--steps` coarse steps from rest
  warm     the case as shipped from the coarse run's state, first_step = ramp_steps + 1 (the inlet at full speed from the first batch),
           up to the same last step number

Both fine runs write forces_series.csv every `--interval` steps; every `--keep`th row of the two goes side by side (Step, U_inlet, Cd
and Cl of the cold run, Cd and Cl of the warm run, empty before its first step) to profiles/warm_start_ball1m_cd_side_by_side.csv, and
profiles/warm_start_ball1m_summary.txt gets one line, from all rows:
the mean and rms of the COLD run's Cd over its last third, and for each run the number of coarse steps taken on the fine grid after which
its Cd stays within that mean +- rms up to the end of the run (both measured against the cold run's band; no threshold is set here).
Evidence, not a test. usage: run_sequenced.py [--steps N (default: the case's own)] [--interval 10] [--keep 10] [--out-prefix profiles/warm_start_ball1m]"""
import argparse
import copy
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run(over, case_dir, name, log):
    from open_ludwig_amd import case, preprocess as pp
    cfg = pp.load_case_configuration(os.path.join(GOLDEN, "ball1m_config.yaml"), over)
    cfg.case_dir = case_dir
    setup = pp.setup_multilevel_domain(cfg, os.path.join(GOLDEN, "ball1m.stl"))
    out = os.path.join(case_dir, name)
    t0 = time.time()
    case.run_case(cfg, case.HipStepper, setup=setup, out_dir=out, log=log)
    cells = sum(512 * g.n_blocks for g in setup[0])
    print(f"{name}: surface_resolution {cfg.surface_resolution}, {cells} cells, {cfg.steps} steps in {time.time() - t0:.1f} s", flush=True)
    return cfg, out


def settled_after(steps, cd, lo, hi):
    """the first step from which cd stays in [lo, hi] up to the end; None if the last row is outside"""
    outside = np.flatnonzero((cd < lo) | (cd > hi))
    if outside.size == 0:
        return int(steps[0])
    return int(steps[outside[-1] + 1]) if outside[-1] + 1 < len(steps) else None


U_INLET, CD, CL = 2, 11, 12                               # Step,Time_s,U_inlet,Fx_N,...,Cd,Cl,Cs,Cmy


def side_by_side(path, cold, warm, keep):
    """every keep-th row of the cold series with the warm run's row of the same step beside it"""
    by_step = {int(r[0]): r for r in warm}
    with open(path, "w") as fh:
        fh.write("Step,U_inlet,Cd_cold,Cl_cold,Cd_warm,Cl_warm\n")
        for r in cold[::keep]:
            w = by_step.get(int(r[0]))
            fh.write("%d,%.6f,%.6f,%.6f,%s\n" % (r[0], r[U_INLET], r[CD], r[CL], "%.6f,%.6f" % (w[CD], w[CL]) if w is not None else ","))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=None, help="coarse steps of the fine runs (default: the case's own)")
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--out-prefix", default=os.path.join(ROOT, "profiles", "warm_start_ball1m"))
    args = ap.parse_args()
    from open_ludwig_amd import _lib, preprocess as pp
    if _lib.device_count() < 1:
        raise SystemExit("run_sequenced.py needs a GPU")
    base = pp.load_case_configuration(os.path.join(GOLDEN, "ball1m_config.yaml"))
    ramp, res = int(base.ramp_steps), int(base.surface_resolution)
    if args.steps is None:
        args.steps = int(base.steps)
    series = {"enabled": True, "start_step": 1, "interval": args.interval}
    quiet = {"basic": {"simulation": {"output_freq": 10 ** 9}}, "advanced": {"diagnostics": {"freq": 1000}, "forces": {"series": series}}}
    work = tempfile.mkdtemp(prefix="sequenced_")
    lines = []
    try:
        coarse = copy.deepcopy(quiet)
        coarse["basic"].update(surface_resolution=res // 2)
        coarse["basic"]["simulation"].update(steps=args.steps // 2, ramp_steps=ramp // 2)
        coarse["advanced"]["state_files"] = {"enabled": True, "interval": 0}
        run(coarse, work, "coarse", lines.append)
        cold = copy.deepcopy(quiet)
        cold["basic"]["simulation"].update(steps=args.steps)
        _, cold_out = run(cold, work, "cold", lines.append)
        warm = copy.deepcopy(quiet)
        warm["basic"]["simulation"].update(steps=args.steps - ramp)
        warm["advanced"]["initial_condition"] = {"state": os.path.join("coarse", "state_%06d.npz" % (args.steps // 2)), "first_step": ramp + 1}
        _, warm_out = run(warm, work, "warm", lines.append)
        for l in lines:
            if l.startswith("initial condition"):
                print(l)
        rows = {}
        for name, out in (("cold", cold_out), ("warm", warm_out)):
            rows[name] = np.loadtxt(os.path.join(out, "forces_series.csv"), delimiter=",", skiprows=1)
        side_by_side(f"{args.out_prefix}_cd_side_by_side.csv", rows["cold"], rows["warm"], args.keep)
        cd = CD
        late = rows["cold"][rows["cold"][:, 0] > args.steps - args.steps // 3, cd]
        mean, rms = float(late.mean()), float(np.sqrt(np.mean((late - late.mean()) ** 2)))
        cold_at = settled_after(rows["cold"][:, 0], rows["cold"][:, cd], mean - rms, mean + rms)
        warm_at = settled_after(rows["warm"][:, 0], rows["warm"][:, cd], mean - rms, mean + rms)
        text = (f"ball1m, surface_resolution {res} against {res // 2} -> {res}, {args.steps} steps, Cd every {args.interval} steps: cold run's Cd "
                f"over steps {args.steps - args.steps // 3 + 1}..{args.steps}: mean {mean:.6f} rms {rms:.6f}; Cd stays within mean +- rms after "
                f"{cold_at if cold_at is not None else 'never (not by the last row)'} fine coarse steps cold and after "
                f"{warm_at - ramp if warm_at is not None else 'never (not by the last row)'} fine coarse steps warm "
                f"(warm run: steps {ramp + 1}..{args.steps}, after {args.steps // 2} coarse-grid steps of twice the time step)")
        print(text)
        with open(f"{args.out_prefix}_summary.txt", "w") as fh:
            fh.write(text + "\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
