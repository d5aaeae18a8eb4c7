"""What the *_cost.py tools share: the timer, the HIP event bracket, the cases and the command line / result writer."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

GOLDEN = os.path.join(ROOT, "tests", "golden")
BALL = {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}}}
# key -> (name in the results, config, STL, overrides)
CASES = {"ball1m": ("ball1m sphere, 3 levels (Re 266k setup)", "ball1m", "ball1m.stl", BALL),
         "wing": ("wing5deg, surface resolution 200, 3 levels", "wing5deg", "wing5deg_model.stl",
                  {"basic": {"surface_resolution": 200, "num_levels": 3}})}


def timed(fn, sync, reps):
    """median host ms of fn() between two sync() calls"""
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


class HipEvent:
    """a hipEvent_t of the HIP runtime libludwig_hip.so runs on, recorded on the null stream (the levels' stream in the tools)"""

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


def box_case():
    """the 256^3 periodic box (one level, the bench workload): (name, grids, solver params, inlet speed)"""
    from open_ludwig_amd import cases
    grids, params = cases.periodic_box((32, 32, 32), init=False)
    return "periodic 256^3", grids, params, 0.0


def golden_case(key="ball1m"):
    """a case of CASES set up from tests/golden: (name, cfg, grids, mesh, physical parameters, solver params)"""
    from open_ludwig_amd import preprocess as pp
    name, cfg_name, stl, over = CASES[key]
    cfg = pp.load_case_configuration(os.path.join(GOLDEN, cfg_name + "_config.yaml"), over)
    grids, mesh, phys, _ = pp.setup_multilevel_domain(cfg, os.path.join(GOLDEN, stl))
    return name, cfg, grids, mesh, phys, pp.solver_params(cfg, phys)


def parse_args(tool, *extra):
    """--out FILE and the tool's own (flag, keywords) arguments; ends the program where there is no GPU"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    for flag, kw in extra:
        ap.add_argument(flag, **kw)
    args = ap.parse_args()
    from open_ludwig_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit(f"{tool} needs a GPU")
    return args


def add_row(rows, row):
    """a result: printed as one JSON line at once, kept for write_rows"""
    rows.append(row)
    print(json.dumps(row), flush=True)


def write_rows(rows, out):
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)
