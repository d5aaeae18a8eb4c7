"""The record step's packed cell finish and its full-width outer face column (kernels.hpp finish_cell PACKED, DirLaneFace).

Bit for bit against the CPU oracle, NaN-aware (tests/_edge_states.py nan_aware_diff), on what tests/test_gpu_record_step.py does not have:

* run shapes: (1,2,3) - a lone block per run, whose face records come through the y neighbour of the x neighbour; (3,1,2) - a run of
  three with an idle fourth wave; (6,1,1) - a run of four plus a run of two. Both starts, after 1, 2 and 3 steps.
  LUDWIG_WIDE_ADDR is read when a level is created, not per call, and it widens the f path's addresses only:
  k_step_records takes its 64-bit form from the size of the record array alone (190 650 blocks and more), which no quick test reaches.
  The runs with the variable set therefore cover k_records_from_populations<4, true>, the first step, and nothing more.
* a box exactly at rest: every population its weight, u = +-0 and Pi = 0 - a `0 - x`, an `x * 0` or an inexact padded add shows here.
* one NaN or +Inf in one population of one cell - a direction with cx = -1, its opposite, one with cx = 0 - at x = 0 of a run's first
  block, x = 7 of a run's last block and in the lone block of (5,2,3): the value sits in one half of a packed pair, and crosses (or
  does not cross) the run's outer face. Two steps. Compared everywhere except the cells tests/_edge_states.py nonfinite_pull_cells
  names: for NaN none, for +Inf the one cell that pulls it on the first step - the oracle's own state after that
  step holds no Inf any more, so the second step adds none (test_nonfinite_cases_leave_out_one_cell_at_most, on the CPU).
"""
import numpy as np
import pytest

import _edge_states as es
from open_ludwig_amd import adapt, cases, execute_timestep_batch
from oracle import oracle

F32 = np.float32
BOXES = [(1, 2, 3), (3, 1, 2), (6, 1, 1)]
STEPS = (1, 2, 3)
INITS = ("taylor_green", "perturbed")


def box_id(b):
    return "x".join(map(str, b))


def make(nb, init):
    grids, params = cases.periodic_box(nb)
    if init == "perturbed":
        cases.init_perturbed(grids[0], 5)
    elif init == "rest":
        g = grids[0]
        w = np.asarray(es.W, dtype=np.float32)
        for name in ("f", "f_temp"):
            getattr(g, name)[...] = w
        for name in ("vel", "vel_temp"):
            getattr(g, name)[...] = F32(0.0)
        g.rho[...] = F32(1.0)
    return grids, params


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


_reference = {}


def reference(nb, init, steps=STEPS):
    key = (nb, init)
    if key not in _reference:
        grids, params = make(nb, init)
        _reference[key] = oracle_states(grids, params, steps)
    return _reference[key]


def run_and_compare(grids, params, n, want, what, allowed=None):
    dev = adapt(grids[0], 0)
    try:
        execute_timestep_batch([dev], 1, n, F32(0.0), params)
        assert dev.record_steps() == n, "a periodic box of plain cells steps by records"
        fn, vn = oracle.newest_buffers(0, n)
        mask = None if allowed is None else ~allowed
        for name, ref in ((fn, want["f"]), (vn, want["vel"]), ("rho", want["rho"])):
            es.assert_nan_aware_equal(dev.download(name), ref, f"{what} after {n} steps: {name}", mask)
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("init", INITS)
@pytest.mark.parametrize("nb", BOXES, ids=box_id)
def test_run_shapes_equal_the_oracle(gpu, nb, init):
    want = reference(nb, init)
    for n in STEPS:
        grids, params = make(nb, init)
        run_and_compare(grids, params, n, want[n], f"{nb} {init}")


@pytest.mark.gpu
@pytest.mark.parametrize("nb", BOXES, ids=box_id)
def test_run_shapes_with_wide_f_path_addresses(gpu, monkeypatch, nb):
    """see the module docstring: this reaches the first step's kernel, not k_step_records<4, true>"""
    monkeypatch.setenv("LUDWIG_WIDE_ADDR", "1")
    want = reference(nb, "perturbed")
    for n in (1, 3):
        grids, params = make(nb, "perturbed")
        run_and_compare(grids, params, n, want[n], f"{nb} wide")


@pytest.mark.gpu
def test_box_at_rest_equals_the_oracle(gpu):
    nb = (2, 1, 1)
    want = reference(nb, "rest", (1, 2))
    for n in (1, 2):
        grids, params = make(nb, "rest")
        run_and_compare(grids, params, n, want[n], "rest")


# ---- one non-finite population ----
NF_BOX = (5, 2, 3)
NF_K = {"cx-1": 0, "opposite": 26, "cx0": 10}            # c = (-1,-1,-1), (1,1,1), (0,-1,0)
NF_PLACE = {"first_x0": (1, 0), "last_x7": (4, 7), "lone": (5, 3)}      # block x (1-based) of the (5,2,3) box, cell x
NF_KIND = {"nan": np.nan, "+inf": np.inf}


def nonfinite_case(kind, which_k, place):
    """y = 0 and z = 5 of block (bx, 1, 2): a diagonal direction then also leaves the block in y"""
    grids, params = make(NF_BOX, "perturbed")
    g = grids[0]
    bx, x = NF_PLACE[place]
    b = int(g.block_pointer[bx - 1, 0, 1]) - 1
    assert b >= 0
    for name in ("f", "f_temp"):
        getattr(g, name)[x, 0, 5, b, NF_K[which_k]] = F32(NF_KIND[kind])
    return grids, params


def oracle_with_allowed(kind, which_k, place, check_nan=False):
    """the oracle's state after two steps, and the cells left out of the comparison: nonfinite_pull_cells of either step's input. A
    NaN names no cell (it is neither an Inf nor a finite set with an overflowing sum), so that is only computed where asked for."""
    grids, params = nonfinite_case(kind, which_k, place)
    g = grids[0]
    allowed = np.zeros((8, 8, 8, g.n_blocks), dtype=bool)
    f_in = g.f_temp.copy()                                 # the first step reads f_temp (f holds the same)
    for n in (1, 2):
        if kind != "nan" or check_nan:
            allowed |= es.nonfinite_pull_cells(g, f_in)
        oracle.execute_timestep_batch(grids, n, 1, F32(0.0), params)
        fn, vn = oracle.newest_buffers(0, n)
        f_in = getattr(g, fn).copy()
    return {"f": f_in, "vel": getattr(g, vn).copy(), "rho": g.rho.copy()}, allowed


NF_CASES = [(kd, k, pl) for kd in NF_KIND for k in NF_K for pl in NF_PLACE]


@pytest.mark.parametrize("kind,which_k,place", [c for c in NF_CASES if c[2] == "first_x0"], ids=lambda v: str(v))
def test_nonfinite_cases_leave_out_one_cell_at_most(kind, which_k, place):
    """CPU only: what the oracle alone excludes - nothing for NaN, the first step's puller for +Inf - and that the value spreads.
    (The other two placements were checked the same way when the cases were chosen; they differ in the block alone.)"""
    want, allowed = oracle_with_allowed(kind, which_k, place, check_nan=True)
    assert int(allowed.sum()) == (0 if kind == "nan" else 1)
    assert np.isnan(want["rho"]).sum() >= 27, "after two steps the 27 cells around the puller have met the value"
    assert np.isfinite(want["rho"]).sum() >= want["rho"].size - 125


@pytest.mark.gpu
@pytest.mark.parametrize("kind,which_k,place", NF_CASES, ids=lambda v: str(v))
def test_one_nonfinite_population_equals_the_oracle(gpu, kind, which_k, place):
    want, allowed = oracle_with_allowed(kind, which_k, place)
    assert int(allowed.sum()) <= 1
    grids, params = nonfinite_case(kind, which_k, place)
    run_and_compare(grids, params, 2, want, f"{kind} k={NF_K[which_k]} {place}", allowed)
