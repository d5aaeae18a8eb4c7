"""The host schedules of the two multi-GPU runners, pinned call by call without a device: DistributedLevelRunner.step,
MultiLevelRunner._step_level and MultiLevelRunner.step are driven with recording fakes (levels, exchangers, the two physics launches, the
library's ludwig_step_distributed), and every recorded call sequence is compared with tests/golden/partition_schedules.json. The fixture
is recorded data only; `python tests/test_partition_schedule_host.py` rewrites it from the code as it stands (done once, before the
schedules were single-sourced: whoever changes a schedule on purpose records it again and reviews the diff).

What is logged, in order: ("collide", level, part, t_sub, tw, parent), ("bouzidi", level, t_sub), ("post", level, [[group, field] ...]),
("join", level), ("in_stream", level, on), ("copy_to_old", level, t_sub), ("step_distributed", t)."""
import contextlib
import ctypes
import itertools
import json
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from open_ludwig_amd import _lib, partition, physics

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partition_schedules.json")
PARTS = {_lib.PART_ALL: "all", _lib.PART_BOUNDARY: "boundary", _lib.PART_INTERIOR: "interior"}


class FakeLevel:
    def __init__(self, log, name, has_post_collision=False, has_temporal_storage=False):
        self.log, self.name, self.handle = log, name, None
        self.has_post_collision, self.has_temporal_storage = has_post_collision, has_temporal_storage

    def copy_to_old(self, t_sub):
        self.log.append(["copy_to_old", self.name, int(t_sub)])


class FakePlan:
    def __init__(self, groups):
        self.groups = set(groups)

    def has(self, name):
        return name in self.groups


class _Recording:
    def post(self, fields):
        self.log.append(["post", self.name, [[g, f] for g, f in fields.items()]])

    def join(self):
        self.log.append(["join", self.name])

    def set_in_stream(self, on):
        self.log.append(["in_stream", self.name, bool(on)])
        self.in_stream = bool(on)


class FakeTorchHalo(_Recording):
    def __init__(self, log, name, groups):
        self.log, self.name, self.plan = log, name, FakePlan(groups)


class FakeNativeHalo(_Recording, partition.NativeHalo):
    """a NativeHalo to isinstance() only: its constructor, which talks to the library, never runs"""

    def __init__(self, log, name, groups, in_stream):
        self.log, self.name, self.plan, self.in_stream = log, name, FakePlan(groups), in_stream
        self._h = None


class FakeParams:
    q_min_threshold = 0.001

    def __init__(self, use_temporal_interp=False):
        self.use_temporal_interp = use_temporal_interp

    def to_c(self):
        return ctypes.c_int(0)


class FakeView:
    def __init__(self, n_owned, tau=0.6):
        self.n_owned = n_owned
        self.level = type("HostLevel", (), {"tau": tau})()


class FakeLib:
    """stands where a runner keeps the _lib module: the constants, check(), and a load() whose library logs ludwig_step_distributed"""
    PART_ALL, PART_BOUNDARY, PART_INTERIOR = _lib.PART_ALL, _lib.PART_BOUNDARY, _lib.PART_INTERIOR

    def __init__(self, log):
        self.log = log

    @staticmethod
    def check(rc):
        assert rc == 0

    def load(self):
        return self

    def ludwig_step_distributed(self, level, plan, parent, t, *rest):
        self.log.append(["step_distributed", int(t)])
        return 0


@contextlib.contextmanager
def recorded_physics(log):
    """physics.stream_collide / apply_bouzidi_correction replaced by recorders (the runners import them inside their methods), and
    _lib.load by a refusal: nothing under test may reach the library"""
    def stream_collide(level, parent, parent_tau, u_curr, params, timestep, temporal_weight=0.0, part=_lib.PART_ALL):
        log.append(["collide", level.name, PARTS[part], int(timestep), float(temporal_weight), parent.name if parent is not None else None])

    def apply_bouzidi_correction(level, timestep, q_min_threshold):
        log.append(["bouzidi", level.name, int(timestep)])

    def load():
        raise AssertionError("a host schedule loaded the library")

    saved = physics.stream_collide, physics.apply_bouzidi_correction, _lib.load
    physics.stream_collide, physics.apply_bouzidi_correction, _lib.load = stream_collide, apply_bouzidi_correction, load
    try:
        yield
    finally:
        physics.stream_collide, physics.apply_bouzidi_correction, _lib.load = saved


def _halo(kind, log, name, groups):
    if kind == "none":
        return None
    if kind == "torch":
        return FakeTorchHalo(log, name, groups)
    return FakeNativeHalo(log, name, groups, in_stream=(kind == "native_in_stream"))


def _groups(f_post, rho):
    return ["f", "vel"] + (["f_post"] if f_post else []) + (["rho"] if rho else [])


# ---- how the runners are constructed: the only part that follows the runners' attributes ----
def multi_level_runner(log, levels, halos, n_owned, level_overlap, params):
    r = object.__new__(partition.MultiLevelRunner)
    r.params = params
    r.levels, r.ex, r.level_overlap = levels, halos, level_overlap
    r.views = [FakeView(n) for n in n_owned]
    return r


def level_runner(log, level, halo, overlap, transport, params):
    r = object.__new__(partition.DistributedLevelRunner)
    r._lib, r.C, r.params = FakeLib(log), ctypes, params
    r.level, r.ex, r.overlap, r.transport = level, halo, overlap, transport
    r.view = FakeView(1)
    return r


# ---- the cases ----
def step_level_cases():
    """MultiLevelRunner._step_level: the full product; the plan's groups only where there is an exchanger"""
    out = {}
    for kind in ("none", "native", "native_in_stream", "torch"):
        plan_bits = [(False, False)] if kind == "none" else list(itertools.product((False, True), repeat=2))
        for i, stepping, children, hpc, (f_post, rho), overlap, t_sub in itertools.product(
                (0, 1), (False, True), (False, True), (False, True), plan_bits, (False, True), (4, 5)):
            log = []
            levels = [FakeLevel(log, "L0"), FakeLevel(log, "L1")]
            levels[i].has_post_collision = hpc
            halos = [FakeTorchHalo(log, "L0", _groups(False, False)), None]
            halos[i] = _halo(kind, log, f"L{i}", _groups(f_post, rho))
            r = multi_level_runner(log, levels, halos, [1 if (stepping or j != i) else 0 for j in range(2)], [overlap, overlap], FakeParams())
            parent = levels[0] if i else None
            with recorded_physics(log):
                r._step_level(i, t_sub, parent, np.float32(0.6), np.float32(0.5 if t_sub % 2 else 0.0), np.float32(0.0), children)
            name = f"i{i}-stepping{int(stepping)}-children{int(children)}-hpc{int(hpc)}-fpost{int(f_post)}-rho{int(rho)}-overlap{int(overlap)}-t{t_sub}-{kind}"
            out[name] = log
    return out


def nest_step_cases():
    """MultiLevelRunner.step: one coarse step of a three-level nest with temporal interpolation, every level held / the middle one not"""
    out = {}
    for held in ("all_levels", "middle_level_absent"):
        log = []
        levels = [FakeLevel(log, "L0", has_temporal_storage=True), FakeLevel(log, "L1", has_temporal_storage=True),
                  FakeLevel(log, "L2", has_post_collision=True)]
        halos = [FakeNativeHalo(log, "L0", _groups(False, True), False), FakeNativeHalo(log, "L1", _groups(False, True), True),
                 FakeTorchHalo(log, "L2", _groups(True, False))]
        n_owned = [3, 2, 5]
        if held == "middle_level_absent":
            levels[1], halos[1], n_owned[1] = None, None, 0
        r = multi_level_runner(log, levels, halos, n_owned, [True, False, True], FakeParams(use_temporal_interp=True))
        with recorded_physics(log):
            r.step(7, 0.03)
        out[held] = log
    return out


def level_runner_cases():
    """DistributedLevelRunner.step: overlap x transport x has_post_collision x plan has f_post x parity"""
    out = {}
    for overlap, transport, hpc, f_post, t in itertools.product((False, True), ("native", "torch"), (False, True), (False, True), (6, 7)):
        log = []
        level = FakeLevel(log, "L0", has_post_collision=hpc)
        halo = _halo(transport, log, "L0", _groups(f_post, False))
        r = level_runner(log, level, halo, overlap, transport, FakeParams())
        with recorded_physics(log):
            r.step(t, 0.03)
        out[f"overlap{int(overlap)}-{transport}-hpc{int(hpc)}-fpost{int(f_post)}-t{t}"] = log
    return out


CASES = {"MultiLevelRunner._step_level": step_level_cases, "MultiLevelRunner.step": nest_step_cases,
         "DistributedLevelRunner.step": level_runner_cases}


def record():
    """every case of every runner method, each sequence stored once: {"sequences": [...], "cases": {method: {case: index}}}"""
    sequences, index, cases = [], {}, {}
    for method, make in CASES.items():
        cases[method] = {}
        for name, log in make().items():
            key = json.dumps(log)
            if key not in index:
                index[key] = len(sequences)
                sequences.append(log)
            cases[method][name] = index[key]
    return {"sequences": sequences, "cases": cases}


def _check(method):
    with open(FIXTURE) as fh:
        want = json.load(fh)
    got = CASES[method]()
    assert sorted(got) == sorted(want["cases"][method]), "the set of cases differs from the recorded one"
    wrong = [name for name, log in got.items() if json.loads(json.dumps(log)) != want["sequences"][want["cases"][method][name]]]
    first = wrong[0] if wrong else None
    assert not wrong, (f"{len(wrong)} of {len(got)} schedules differ; first: {first}\n got  {got[first]}\n want "
                       f"{want['sequences'][want['cases'][method][first]]}")
    return len(got)


def test_multi_level_step_level_schedules_are_the_recorded_ones():
    assert _check("MultiLevelRunner._step_level") == 832


def test_multi_level_nest_step_is_the_recorded_one():
    assert _check("MultiLevelRunner.step") == 2


def test_distributed_level_runner_schedules_are_the_recorded_ones():
    assert _check("DistributedLevelRunner.step") == 32


if __name__ == "__main__":
    data = record()
    with open(FIXTURE, "w") as fh:
        fh.write("{\n \"sequences\": [\n" + ",\n".join("  " + json.dumps(s) for s in data["sequences"]) + "\n ],\n \"cases\": "
                 + json.dumps(data["cases"], indent=1).replace("\n", "\n ") + "\n}\n")
    print(f"{sum(len(c) for c in data['cases'].values())} cases, {len(data['sequences'])} distinct sequences -> {FIXTURE}")
