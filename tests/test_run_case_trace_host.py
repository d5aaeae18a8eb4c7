"""run_case pinned call by call without a device: the CPU oracle behind a stepper that logs batch, field and close drives the cube with
every output that has a host path switched on, at schedules that do not coincide, and the stepper-call trace, the log lines, the file
names and every CSV's text are compared with tests/golden/run_case_trace.json. The fixture is recorded data only;
`python tests/test_run_case_trace_host.py` rewrites it from the code as it stands (done once, before run_case was broken into phases:
whoever changes the order of run_case's calls or files on purpose records it again and reviews the diff).

What is logged, in order: ["batch", t_start, n, u_curr], ["field", level, name], ["close"]."""
import copy
import functools
import json
import os
import sys
import tempfile

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from open_ludwig_amd import case, preprocess as pp

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(G, "run_case_trace.json")
CFG, STL = os.path.join(G, "cube1m_config.yaml"), os.path.join(G, "cube1m.stl")
SEEDS = [{"name": "rake", "line": {"from": [-4.0, -1.5, -0.2], "to": [-4.0, 1.5, 0.3], "count": 5}},
         {"name": "pts", "points": [[-2.0, 0.3, 0.1], [0.0, 0.0, 0.0], [1.0e3, 0.0, 0.0]]}]
CAMERA = {"type": "perspective", "position": [-6.0, -5.0, 4.0], "look_at": [0.0, 0.0, 0.0], "up": [0, 0, 1], "fov": 40}
BASE = {"basic": {"num_levels": 1, "surface_resolution": 7, "simulation": {"steps": 12, "output_freq": 8, "ramp_steps": 4}},
        "advanced": {"boundary": {"method": "bounce_back"}, "high_re": {"wall_model": {"enabled": False}},
                     "numerics": {"c_wale": 0.0, "nu_sgs_background": 0.0}, "diagnostics": {"freq": 4}, "gpu": {"async_depth": 5},
                     "surface_statistics": {"enabled": True, "start_step": 3, "interval": 4},
                     "slices": {"enabled": True, "start_step": 2, "interval": 3, "planes": [{"name": "mid", "normal": "y", "position": 0.0}]},
                     "streamlines": {"enabled": True, "start_step": 2, "interval": 5, "step": 0.5, "max_steps": 60, "min_speed": 1e-7,
                                     "direction": "both", "seeds": SEEDS},
                     "tracers": {"enabled": True, "start_step": 2, "interval": 2, "release_every": 2, "generations": 2, "output_interval": 4,
                                 "seeds": SEEDS},
                     "flux_planes": {"enabled": True, "start_step": 1, "interval": 7,
                                     "planes": [{"name": "wake", "normal": "x", "position": 1.5, "direction": -1}],
                                     "boxes": [{"name": "cv", "bounds": [[-1.0, 1.2], [-0.9, 0.9], [-0.8, 0.8]]}]},
                     "isosurfaces": {"enabled": True, "start_step": 4, "interval": 4,
                                     "surfaces": [{"name": "front", "field": "density", "value": 1.000001},
                                                  {"name": "speed", "field": "velocity_magnitude", "value": 1e-4}]},
                     "state_files": {"enabled": True, "interval": 6},
                     "flow_monitor": {"enabled": True},
                     "render": {"enabled": True, "start_step": 3, "interval": 6, "width": 24, "height": 16, "views": [
                         {"name": "v", "field": "velocity_magnitude", "range": [0.0, 0.02], "colormap": "heat", "opacity": 0.05,
                          "camera": CAMERA}]}}}
CONFIGS = ("all_outputs", "no_tracers_depth_8")


def overrides(which, state_files=True):
    over = copy.deepcopy(BASE)
    if which == "no_tracers_depth_8":                                          # segments longer than one step occur
        del over["advanced"]["tracers"]
        over["advanced"]["gpu"]["async_depth"] = 8
    if not state_files:
        del over["advanced"]["state_files"]
    return over


@functools.lru_cache(maxsize=None)
def _setup(which):
    """the grids are stepped in place, but every OracleStepper starts them from the rest state"""
    return pp.setup_multilevel_domain(pp.load_case_configuration(CFG, overrides(which)), STL)


def _tracing(trace):
    from _steppers import OracleStepper

    class Tracing(OracleStepper):
        def batch(self, t_start, n, u_curr, params):
            trace.append(["batch", int(t_start), int(n), float(u_curr)])
            super().batch(t_start, n, u_curr, params)

        def field(self, level, name):
            trace.append(["field", int(level), str(name)])
            return super().field(level, name)

        def close(self):
            trace.append(["close"])
            super().close()
    return Tracing


def _csv_text(path):
    """a CSV's text; of convergence.csv only the columns that hold no wall-clock value (Walltime and MLUPS are left out)"""
    text = open(path).read()
    if os.path.basename(path) != "convergence.csv":
        return text
    return "".join(",".join(c for i, c in enumerate(l.split(",")) if i not in (1, 5)) + "\n" for l in text.splitlines())


@functools.lru_cache(maxsize=None)
def run(which, write_files=True, state_files=True):
    """one run -> {"trace", "log", "files", "csv"}; each distinct run is made once and shared by the tests"""
    from oracle import oracle
    oracle.set_num_threads(min(8, os.cpu_count() or 1))
    cfg = pp.load_case_configuration(CFG, overrides(which, state_files))
    trace, lines = [], []
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out")
        case.run_case(cfg, _tracing(trace), setup=_setup(which), out_dir=out, log=lines.append, write_files=write_files)
        files = sorted(os.listdir(out)) if os.path.isdir(out) else []
        csv = {name: _csv_text(os.path.join(out, name)) for name in files if name.endswith(".csv")}
    return {"trace": trace, "log": lines, "files": files, "csv": csv}


@pytest.mark.parametrize("which", CONFIGS)
def test_trace_log_files_and_csv_text_are_the_recorded_ones(which):
    with open(FIXTURE) as fh:
        want = json.load(fh)[which]
    got = json.loads(json.dumps(run(which)))
    assert got["trace"] == want["trace"]
    assert got["log"] == want["log"]
    assert got["files"] == want["files"]
    assert sorted(got["csv"]) == sorted(want["csv"])
    for name in want["csv"]:
        assert got["csv"][name] == want["csv"][name], name
    ends = [b[1] + b[2] - 1 for b in got["trace"] if b[0] == "batch"]
    assert ends == sorted(set(ends)) and ends[-1] == 12 and got["trace"][-1] == ["close"]
    if which == "no_tracers_depth_8":
        assert max(b[2] for b in got["trace"] if b[0] == "batch") > 1


def _only_in_first(a, b):
    """b must be a's calls in a's order with some left out -> the calls left out"""
    extra, j = [], 0
    for call in a:
        if j < len(b) and call == b[j]:
            j += 1
        else:
            extra.append(call)
    assert j == len(b), f"call {j} of the shorter trace, {b[j]}, is not in the longer one in this order"
    return extra


def test_write_files_false_writes_nothing_and_asks_the_stepper_the_same():
    """every rank of a distributed run makes the same stepper calls and one rank writes. Without state files the trace of a run that
    writes nothing IS the trace of the run that writes. A state file is written from fields downloaded for it, by the writing rank alone:
    there the two runs differ by exactly the two field reads (rho, newest velocity) of each state file and its log line - stated here,
    not hidden; the state steps 6 and 12 are cut by the tracers anyway, so the batches are the same."""
    writes, quiet = run("all_outputs", True, False), run("all_outputs", False, False)
    assert quiet["files"] == [] and writes["files"]
    assert quiet["trace"] == writes["trace"] and quiet["log"] == writes["log"]
    with_state, quiet_state = run("all_outputs", True, True), run("all_outputs", False, True)
    assert quiet_state["files"] == [] and quiet_state["trace"] == quiet["trace"] and quiet_state["log"] == quiet["log"]
    extra = _only_in_first(with_state["trace"], quiet_state["trace"])
    assert sorted(extra) == sorted([["field", 0, "rho"], ["field", 0, "vel_temp"]] * 2)
    assert _only_in_first(with_state["log"], quiet_state["log"]) == ["state file state_000006.npz written", "state file state_000012.npz written"]
    assert [f for f in with_state["files"] if f not in writes["files"]] == ["state_000006.npz", "state_000012.npz"]


class _Boom(Exception):
    pass


SETUPS = ("probes_setup", "slices_setup", "surface_stats_setup", "wall_diagnostics_setup", "force_series_setup", "modes_setup")


def _lifetime_config():
    over = {"basic": {"num_levels": 1, "surface_resolution": 7},
            "advanced": {"probes": {"enabled": True, "points": [[-2.0, 0.3, 0.1]]},
                         "slices": {"enabled": True, "planes": [{"name": "mid", "normal": "y", "position": 0.0}]},
                         "surface_statistics": {"enabled": True, "start_step": 1},
                         "wall_diagnostics": {"enabled": True},
                         "forces": {"enabled": True, "series": {"enabled": True}},
                         "fourier_modes": {"enabled": True, "samples": 4, "strouhal": [0.2]}}}
    return pp.load_case_configuration(CFG, over)


@functools.lru_cache(maxsize=None)
def _lifetime_setup():
    return pp.setup_multilevel_domain(_lifetime_config(), STL)


@pytest.mark.parametrize("failing", SETUPS + ("out_dir",))
def test_a_failure_after_the_stepper_exists_closes_it_once_and_propagates(failing, tmp_path):
    """a stepper whose set-up call raises, or an out_dir that cannot be created, ends the run with that very error and the stepper closed
    exactly once. Before run_case held the stepper under one try ... finally these calls sat under no try at all and the stepper was never
    closed: this is the one test here that fails on that earlier run_case."""
    closed, boom = [], _Boom(failing)

    def setup_call(name):
        def call(self, *args, **kwargs):
            if name == failing:
                raise boom
        return call

    class Failing:
        def __init__(self, grids):
            pass

        def close(self):
            closed.append(True)
    for name in SETUPS:
        setattr(Failing, name, setup_call(name))
    out_dir = None
    if failing == "out_dir":
        (tmp_path / "a_file").write_text("")
        out_dir = str(tmp_path / "a_file" / "out")
    with pytest.raises((_Boom, OSError)) as err:
        case.run_case(_lifetime_config(), Failing, steps=1, setup=_lifetime_setup(), out_dir=out_dir)
    assert (err.value is boom) if failing != "out_dir" else isinstance(err.value, NotADirectoryError)
    assert closed == [True]


if __name__ == "__main__":
    data = {which: run(which) for which in CONFIGS}
    with open(FIXTURE, "w") as fh:
        json.dump(data, fh, indent=1)
        fh.write("\n")
    for which, d in data.items():
        print(f"{which}: {len(d['trace'])} stepper calls, {len(d['log'])} log lines, {len(d['files'])} files -> {FIXTURE}")
