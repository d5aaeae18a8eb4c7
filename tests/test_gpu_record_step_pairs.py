"""The record step's outer-face pass behind the workgroup barrier, and the pull's cx = +-1 pairs (kernels.hpp k_step_records).

Bit for bit against the CPU oracle, NaN-aware (tests/_edge_states.py nan_aware_diff):

* run shapes where the face pass can go wrong, both starts, after 1, 2 and 3 steps: (1,2,3) - a lone block per run, one wave loads
  both faces and the ninth record in front of the barrier and evaluates them behind it; (3,1,2) - a run of three beside an idle
  wave, which still has to reach the barrier; (6,1,1) - a run of four and a run of two; (5,2,3).
* the box at rest, every population its weight and Pi = 0, with the stored velocity +0 and -0: the cx = -1 value is the cx = +1
  expression on negated operands, so a {t, -t} of zero, or a zero term added where it must be dropped, shows here. Lone blocks
  (1,2,1) and a run of two.
* one NaN or +Inf in one population of one cell (tests/_record_pairs_cases.py): c = (-1,-1,-1), its opposite and (0,-1,-1) - the
  cx = -1 and cx = +1 members of a pull row and the cx = 0 one between them - at x = 0 of a run's first block, x = 7 of its last and
  in a lone block. Two steps. Compared everywhere but the cells nonfinite_pull_cells names, one at most per case (for k = 0 and 26
  tests/test_gpu_record_step_packed.py test_nonfinite_cases_leave_out_one_cell_at_most shows that on the CPU, for k = 1
  tests/test_record_step_pairs_host.py).
* the f path of the same binary (LUDWIG_RECORD_STEP=0) on the perturbed start: equal bits in f, vel and rho after 3 steps.
"""
import numpy as np
import pytest

import _edge_states as es
import _record_pairs_cases as rp
from open_ludwig_amd import adapt, execute_timestep_batch
from oracle import oracle

F32 = np.float32
BOXES = [(1, 2, 3), (3, 1, 2), (6, 1, 1), (5, 2, 3)]
STEPS = (1, 2, 3)
INITS = ("taylor_green", "perturbed")


def box_id(b):
    return "x".join(map(str, b))


def oracle_states(grids, params, steps):
    """the oracle's newest f, vel and rho after each step count of `steps`, read-only"""
    out, t = {}, 0
    for n in steps:
        oracle.execute_timestep_batch(grids, t + 1, n - t, F32(0.0), params)
        t = n
        fn, vn = oracle.newest_buffers(0, n)
        out[n] = {"f": getattr(grids[0], fn).copy(), "vel": getattr(grids[0], vn).copy(), "rho": grids[0].rho.copy()}
        for a in out[n].values():
            a.setflags(write=False)
    return out


def make_rest(nb, zero):
    grids, params = rp.make(nb, "rest")
    for name in ("vel", "vel_temp"):
        getattr(grids[0], name)[...] = F32(zero)
    return grids, params


_reference = {}


def reference(key, build):
    if key not in _reference:
        grids, params = build()
        _reference[key] = oracle_states(grids, params, STEPS)
    return _reference[key]


def run_steps(grids, params, n, records=True):
    dev = adapt(grids[0], 0)
    try:
        execute_timestep_batch([dev], 1, n, F32(0.0), params)
        assert dev.record_steps() == (n if records else 0)
        fn, vn = oracle.newest_buffers(0, n)
        return {"f": dev.download(fn), "vel": dev.download(vn), "rho": dev.download("rho")}
    finally:
        dev.close()


def compare(got, want, what, allowed=None):
    mask = None if allowed is None else ~allowed
    for name in ("f", "vel", "rho"):
        es.assert_nan_aware_equal(got[name], want[name], f"{what}: {name}", mask)


@pytest.mark.gpu
@pytest.mark.parametrize("init", INITS)
@pytest.mark.parametrize("nb", BOXES, ids=box_id)
def test_run_shapes_equal_the_oracle(gpu, nb, init):
    want = reference((nb, init), lambda: rp.make(nb, init))
    for n in STEPS:
        grids, params = rp.make(nb, init)
        compare(run_steps(grids, params, n), want[n], f"{nb} {init} after {n} steps")


@pytest.mark.gpu
@pytest.mark.parametrize("zero", [0.0, -0.0], ids=["+0", "-0"])
@pytest.mark.parametrize("nb", [(1, 2, 1), (2, 1, 1)], ids=box_id)
def test_box_at_rest_equals_the_oracle(gpu, nb, zero):
    want = reference((nb, "rest", str(zero)), lambda: make_rest(nb, zero))
    for n in STEPS:
        grids, params = make_rest(nb, zero)
        compare(run_steps(grids, params, n), want[n], f"rest {nb} u = {zero} after {n} steps")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,which_k,place", rp.NF_CASES, ids=lambda v: str(v))
def test_one_nonfinite_population_equals_the_oracle(gpu, kind, which_k, place):
    want, allowed = rp.oracle_with_allowed(kind, which_k, place)
    assert int(allowed.sum()) <= 1
    grids, params = rp.nonfinite_case(kind, which_k, place)
    compare(run_steps(grids, params, 2), want, f"{kind} k={rp.NF_K[which_k]} {place} after 2 steps", allowed)


@pytest.mark.gpu
def test_switched_off_gives_the_same_bits(gpu, monkeypatch):
    nb = (5, 2, 3)
    records = run_steps(*rp.make(nb, "perturbed"), 3)
    monkeypatch.setenv("LUDWIG_RECORD_STEP", "0")
    f_path = run_steps(*rp.make(nb, "perturbed"), 3, records=False)
    compare(records, f_path, f"{nb} records against the f path after 3 steps")
