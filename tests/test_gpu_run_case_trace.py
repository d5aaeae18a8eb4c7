"""run_case pinned call by call on the device: a HipStepper that logs every public method run_case calls drives the cube on two levels
with every output switched on, then a second run warm-started from the first run's state file, and both call traces and file lists are
compared with tests/golden/run_case_trace_gpu.json. The fixture is recorded data only; `python tests/test_gpu_run_case_trace.py` on a
device rewrites it from the code as it stands (done once, before run_case was broken into phases). The trace holds names, scalar
arguments and the shapes of arrays - nothing the kernels compute - so it does not follow the numerics; what the files hold is pinned by
each output's own test_gpu_*.py."""
import copy
import json
import os
import sys
import tempfile

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from open_ludwig_amd import case, preprocess as pp

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(G, "run_case_trace_gpu.json")
SEEDS = [{"name": "rake", "line": {"from": [-4.0, -1.5, -0.2], "to": [-4.0, 1.5, 0.3], "count": 5}},
         {"name": "pts", "points": [[-2.0, 0.3, 0.1], [0.0, 0.0, 0.0], [1.0e3, 0.0, 0.0]]}]
CAMERA = {"type": "perspective", "position": [-6.0, -5.0, 4.0], "look_at": [0.0, 0.0, 0.0], "up": [0, 0, 1], "fov": 40}
CUBE = {"basic": {"num_levels": 2, "surface_resolution": 14,
                  "simulation": {"steps": 12, "output_freq": 8, "ramp_steps": 4,
                                 "output_fields": {"vorticity": True, "q_criterion": True, "eddy_viscosity": True}}},
        "advanced": {"diagnostics": {"freq": 4}, "gpu": {"async_depth": 5},
                     "probes": {"enabled": True, "start_step": 2, "interval": 3, "points": [[-2.0, 0.3, 0.1], [2.0, 0.0, 0.4]]},
                     "statistics": {"enabled": True, "start_step": 3, "interval": 4, "subgrid": True},
                     "surface_statistics": {"enabled": True, "start_step": 3, "interval": 4},
                     "forces": {"series": {"enabled": True, "start_step": 2, "interval": 1}},
                     "slices": {"enabled": True, "start_step": 2, "interval": 3, "planes": [{"name": "mid", "normal": "y", "position": 0.0}]},
                     "isosurfaces": {"enabled": True, "start_step": 4, "interval": 4,
                                     "surfaces": [{"name": "q", "field": "q_criterion", "value": 2e-6},
                                                  {"name": "front", "field": "density", "value": 1.000001}]},
                     "streamlines": {"enabled": True, "start_step": 2, "interval": 5, "step": 0.5, "max_steps": 60, "min_speed": 1e-7,
                                     "direction": "both", "seeds": SEEDS},
                     "render": {"enabled": True, "start_step": 3, "interval": 6, "width": 24, "height": 16, "views": [
                         {"name": "v", "field": "velocity_magnitude", "range": [0.0, 0.02], "colormap": "heat", "opacity": 0.05,
                          "camera": CAMERA}]},
                     "tracers": {"enabled": True, "start_step": 2, "interval": 2, "release_every": 2, "generations": 2, "output_interval": 4,
                                 "seeds": SEEDS},
                     "flux_planes": {"enabled": True, "start_step": 1, "interval": 7,
                                     "planes": [{"name": "wake", "normal": "x", "position": 1.5, "direction": -1}],
                                     "boxes": [{"name": "cv", "bounds": [[-1.0, 1.2], [-0.9, 0.9], [-0.8, 0.8]]}]},
                     "fourier_modes": {"enabled": True, "start_step": 1, "interval": 2, "samples": 3, "strouhal": [0.2], "repeat": True},
                     "flow_monitor": {"enabled": True},
                     "wall_diagnostics": {"enabled": True},
                     "state_files": {"enabled": True, "interval": 6}}}
# the one scalar argument that follows the flow: the triangles a surface may still take after the levels before it
FLOW_DEPENDENT = {"isosurface": 7}


def _brief(x):
    """a scalar as it is, an array as its shape, a sequence item by item, anything else as its type's name"""
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, np.ndarray):
        return ["array", list(x.shape)]
    if isinstance(x, (list, tuple)):
        return [_brief(v) for v in x]
    return type(x).__name__


def _tracing(trace):
    """a HipStepper whose public methods log [name, arguments...]; a method that another one calls is not logged again"""
    class Tracing(case.HipStepper):
        _depth = 0

    def logged(name, inner):
        def call(self, *args, **kwargs):
            if self._depth == 0:
                brief = [_brief(a) for a in args]
                if name in FLOW_DEPENDENT and len(brief) > FLOW_DEPENDENT[name]:
                    brief[FLOW_DEPENDENT[name]] = "follows the flow"
                trace.append([name] + brief + [[k, _brief(v)] for k, v in sorted(kwargs.items())])
            self._depth += 1
            try:
                return inner(self, *args, **kwargs)
            finally:
                self._depth -= 1
        return call
    for name, member in vars(case.HipStepper).items():
        if callable(member) and not name.startswith("_"):
            setattr(Tracing, name, logged(name, member))
    return Tracing


def run_pair(root):
    """the 12-step run into root/first and the 6-step run warm-started from its state_000006.npz at first_step 7 into root/warm ->
    {"first": {"trace", "files"}, "warm": {...}}, and both runs' log lines"""
    stl = os.path.join(G, "cube1m.stl")
    warm = copy.deepcopy(CUBE)
    warm["basic"]["simulation"]["steps"] = 6
    warm["advanced"]["initial_condition"] = {"state": os.path.join("first", "state_000006.npz"), "first_step": 7}
    warm["advanced"]["statistics"]["start_step"] = 7                           # the sums are reset at start_step: it has to be run through
    got, logs, setup = {}, {}, None
    for name, over in (("first", CUBE), ("warm", warm)):
        cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), copy.deepcopy(over))
        cfg.case_dir = str(root)                                               # state paths are relative to the case folder
        setup = setup or pp.setup_multilevel_domain(cfg, stl)
        assert len(setup[0]) == 2
        trace, logs[name] = [], []
        case.run_case(cfg, _tracing(trace), setup=setup, out_dir=os.path.join(root, name), log=logs[name].append)
        got[name] = {"trace": trace, "files": sorted(os.listdir(os.path.join(root, name)))}
    return got, logs


def dump(data, fh):
    """the fixture's layout: one call per line"""
    runs = [f' "{name}": {{\n  "files": {json.dumps(d["files"])},\n  "trace": [\n' + ",\n".join("   " + json.dumps(c) for c in d["trace"])
            + "\n  ]\n }" for name, d in data.items()]
    fh.write("{\n" + ",\n".join(runs) + "\n}\n")


@pytest.mark.gpu
def test_device_call_traces_and_file_lists_are_the_recorded_ones(gpu, tmp_path):
    with open(FIXTURE) as fh:
        want = json.load(fh)
    got, _ = run_pair(str(tmp_path))
    got = json.loads(json.dumps(got))
    for name in ("first", "warm"):
        assert got[name]["trace"] == want[name]["trace"], name
        assert got[name]["files"] == want[name]["files"], name
    names = {c[0] for c in got["first"]["trace"]}
    assert {"probes_setup", "stats_sample", "subgrid_stats_sample", "surface_stats_setup", "force_series_new", "slices_sample", "isosurface",
            "streamlines", "render", "tracers_snapshot", "flux_planes_new", "modes_sums", "modes_reset", "monitor", "wall_census",
            "gradient_fields", "subgrid_fields", "close"} <= names
    assert got["warm"]["trace"][0][0] == "init_from" and got["warm"]["trace"][0][2] == 7
    assert "state_000006.npz" in got["first"]["files"] and "state_000012.npz" in got["warm"]["files"]


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        data, _ = run_pair(tmp)
    with open(FIXTURE, "w") as fh:
        dump(data, fh)
    print({name: (len(d["trace"]), len(d["files"])) for name, d in data.items()}, "->", FIXTURE)
