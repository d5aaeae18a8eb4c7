"""The HIP step on the topology table (tests/_topology_cases.py): ragged nests, a level 1 with holes, boxes one block wide.

What the block topology drives in the library - the work list (x-runs of 4, leftover chains, link bits, the merge of the two
launch classes), the LDS face hand-over with the patch phase of the GENERAL kernel, and the priority chain for a missing pull
source - is run here where it can go wrong, and has to land on the oracle's bits: every case, coarse steps 1-4 on one set of device
levels, every level, both A/B buffers and rho after every step. tests/test_step_topologies_host.py shows on the CPU that the oracle
is right on these tables (against the float64 restatement) and that the table holds the topologies it names.

The same check runs with the launch classes kept apart and merged, with 64-bit addressing and with a caller's shuffled work list;
part launches must give the bits of a whole-level launch; ludwig_level_info must report the class mix and linking the table was
built for; two cases are compared with the float64 restatement directly, without the oracle; the stencil observers
(velocity-gradient fields, subgrid model) must equal their float32 restatements on tables with holes and self-neighbours.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _gradient_ref as gref
import _step_ref as sr
import _step_ref_cases as sc
import _subgrid_ref as sref
import _topology_cases as tc
from open_ludwig_amd import _lib, adapt, execute_timestep_batch
from oracle import oracle
from test_gpu_parity import post_collision_rows

pytestmark = pytest.mark.gpu
F32 = np.float32
STATE = ("f", "f_temp", "vel", "vel_temp", "rho")
_info = {}              # case -> per level (n_fast_blocks, n_general_blocks, n_xrun_blocks) under the default order


@functools.lru_cache(maxsize=len(tc.OTHER_PATHS))
def oracle_states(name):
    """the oracle's state after each coarse step of the case: [step][level] name -> array (read-only, shared between tests)"""
    case = tc.CASES[name]
    grids, params = case.build()
    out = []
    for t in case.steps:
        oracle.execute_timestep_batch(grids, t, 1, F32(case.u), params)
        snap = []
        for g in grids:
            s = {n: getattr(g, n).copy() for n in STATE}
            if g.n_boundary_cells > 0:
                s["f_post_collision"] = g.f_post_collision.copy()
            for a in s.values():
                a.flags.writeable = False
                assert np.isfinite(a).all()
            snap.append(s)
        out.append(snap)
    return out


def assert_same_bits(label, level, host, want):
    """every state array of one device level against the expected ones; f_post_collision at the x-rows that are read (the library
    stores it nowhere else, include/ludwig_hip.h)"""
    for n, b in want.items():
        a = level.download(n)
        if n == "f_post_collision":
            m = post_collision_rows(host)
            assert m.any()
            a, b = a[m], b[m]
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError(f"{label} {n}: {bad.shape[0]} elements differ, first at {bad[0]}, hip {a[tuple(bad[0])]!r} expected {b[tuple(bad[0])]!r}")


def shuffled_items(n_blocks, seed):
    """a caller's work list: every (block << 3) | z once in a seeded shuffle with idle items (-1) sprinkled in; its length is no
    multiple of the workgroup's 4 waves, so the last group is partial and loose items have to be repacked"""
    rng = np.random.default_rng(seed)
    items = rng.permutation(8 * n_blocks).astype(np.int32)
    n_idle = 4 * int(rng.integers(1, 4)) + int(rng.integers(1, 4))
    for pos in sorted(rng.integers(0, items.size + 1, n_idle).tolist(), reverse=True):
        items = np.insert(items, pos, -1)
    assert items.size % 4 != 0 and (items >= 0).sum() == 8 * n_blocks
    return items


def run_against_oracle(name, caller_list=False, record=False):
    case = tc.CASES[name]
    grids, params = case.build()
    want = oracle_states(name)
    dev = [adapt(g, 0) for g in grids]
    try:
        if record:
            _info[name] = [(i.n_fast_blocks, i.n_general_blocks, i.n_xrun_blocks) for i in (d.info() for d in dev)]
        if caller_list:
            for lv, d in enumerate(dev):
                d.set_order(shuffled_items(d.n_blocks, 77 + lv))
        for t, snap in zip(case.steps, want):
            execute_timestep_batch(dev, t, 1, F32(case.u), params)
            for lv, (g, d) in enumerate(zip(grids, dev)):
                assert_same_bits(f"{name} t={t} level {lv + 1}", d, g, snap[lv])
    finally:
        for d in dev:
            d.close()


@pytest.mark.parametrize("name", list(tc.CASES))
def test_hip_equals_oracle_bit_for_bit(gpu, monkeypatch, name):
    for var in ("LUDWIG_MERGE_CLASSES", "LUDWIG_WIDE_ADDR"):
        monkeypatch.delenv(var, raising=False)
    run_against_oracle(name, record=True)


@pytest.mark.parametrize("name", tc.OTHER_PATHS)
@pytest.mark.parametrize("path", ["separate_classes", "merged_classes", "wide_addr", "caller_list"])
def test_other_kernel_paths_equal_oracle_bit_for_bit(gpu, monkeypatch, path, name):
    """the two block classes in separate launches and in one, 64-bit per-lane addresses, and a shuffled caller's work list - the
    switches are read when a level is created and when its order is set"""
    env = {"separate_classes": ("LUDWIG_MERGE_CLASSES", "0"), "merged_classes": ("LUDWIG_MERGE_CLASSES", "1"), "wide_addr": ("LUDWIG_WIDE_ADDR", "1")}
    if path in env:
        monkeypatch.setenv(*env[path])
    run_against_oracle(name, caller_list=path == "caller_list")


def test_part_launches_give_the_bits_of_a_whole_level_launch(gpu):
    """level 1 with holes, a seeded comm_boundary flag per block: the interior part, then the boundary part (the multi-GPU launch
    pattern) against one whole-level launch and against the oracle, over both A/B parities"""
    case = tc.CASES["level1_holes"]
    grids, params = case.build()
    g = grids[0]
    g.comm_boundary = (np.random.default_rng(13).random(g.n_blocks) < 0.4).astype(np.uint8)
    assert 0 < int(g.comm_boundary.sum()) < g.n_blocks
    lib = _lib.load()
    fl = params.to_c()
    whole, parts = adapt(g, 0), adapt(g, 0)
    try:
        for t in (1, 2):
            _lib.check(lib.ludwig_stream_collide(whole.handle, None, t, case.u, 0.5, 0.0, C.byref(fl), _lib.PART_ALL))
            for part in (_lib.PART_INTERIOR, _lib.PART_BOUNDARY):
                _lib.check(lib.ludwig_stream_collide(parts.handle, None, t, case.u, 0.5, 0.0, C.byref(fl), part))
            oracle.execute_timestep_batch(grids, t, 1, F32(case.u), params)       # no Bouzidi cell here: the step is the launch
            for n in STATE:
                a, b = whole.download(n), parts.download(n)
                assert np.array_equal(a, b), f"t={t} {n}: part launches differ from the whole-level launch"
                assert np.array_equal(a, getattr(g, n)), f"t={t} {n}: whole-level launch differs from the oracle"
    finally:
        whole.close()
        parts.close()


def test_level_info_reports_the_mix_the_table_was_built_for(gpu, monkeypatch):
    """what only the device can report: how the library classified and linked the blocks"""
    for var in ("LUDWIG_MERGE_CLASSES", "LUDWIG_WIDE_ADDR"):
        monkeypatch.delenv(var, raising=False)
    for name, case in tc.CASES.items():
        if name in _info:
            continue
        grids, _ = case.build()
        dev = [adapt(g, 0, upload_state=False) for g in grids]
        _info[name] = [(i.n_fast_blocks, i.n_general_blocks, i.n_xrun_blocks) for i in (d.info() for d in dev)]
        for d in dev:
            d.close()
    for name, levels in _info.items():
        print(f"\n{name:18s} " + "  ".join(f"fast {f} general {g} linked {x}" for f, g, x in levels), end="")
    flat = [lv for levels in _info.values() for lv in levels]
    assert any(f > 0 and g > 0 for f, g, _ in flat), "no level mixes all-neighbour and general blocks"
    assert any(0 < x < f for f, _, x in flat), "no level has both linked and lone all-neighbour blocks"
    # a block that is its own x neighbour is never linked to itself
    assert _info["periodic_1x3x1"] == [(3, 0, 0)]
    # the classification is the neighbour table's
    for name, case in tc.CASES.items():
        grids, _ = case.build()
        for g, (f, gen, x) in zip(grids, _info[name]):
            assert f == int(tc.all_neighbour_blocks(g).sum()) and f + gen == g.n_blocks and 0 <= x <= f, name


@pytest.mark.parametrize("name", tc.DIRECT)
def test_hip_matches_float64_restatement_directly(gpu, name):
    """the w_k arm and the all-general nest against ref64 itself (bounds and exclusion rule of tests/_step_ref.py), so that the
    value check there does not rest on the oracle; steps 1-2, each from the uploaded snapshot"""
    case = tc.CASES[name]
    grids, params = case.build()
    for t in case.steps[:2]:
        check = sc.StepCheck(grids, params, t, case.u)
        dev = [adapt(g, 0) for g in grids]
        try:
            execute_timestep_batch(dev, t, 1, F32(case.u), params)
            for lv, (g, d) in enumerate(zip(grids, dev)):
                assert check.excluded_share[lv] <= sr.MAX_EXCLUDED_SHARE
                ref = check.ref[lv]
                names = [ref.f_name, ref.vel_name, "rho"] + (["f_old", "rho_old", "vel_old"] if ref.old is not None else [])
                err = check.compare(lv, g, {n: d.download(n) for n in names}, f"{name} t={t} hip")
                print(f"\n{name} t={t} level {lv + 1}: HIP error / bound " + " ".join(f"{k} {v / sr.bound(k):.3f}" for k, v in err.items()), end="")
        finally:
            for d in dev:
                d.close()
        oracle.execute_timestep_batch(grids, t, 1, F32(case.u), params)


@pytest.mark.parametrize("name", tc.OBSERVED)
def test_stencil_observers_equal_their_restatements(gpu, name):
    """after coarse step 2, every level, both velocity buffers: vorticity and Q against tests/_gradient_ref.py, nu_t and the branch
    code against tests/_subgrid_ref.py - where a face neighbour is missing inside the domain, and where it is the block itself"""
    case = tc.CASES[name]
    grids, params = case.build()
    dev = [adapt(g, 0) for g in grids]
    try:
        execute_timestep_batch(dev, 1, 2, F32(case.u), params)
        for d, g in zip(dev, grids):
            scale = F32(1.0 / g.dx)
            for vel_name in ("vel", "vel_temp"):
                vel = d.download(vel_name)
                assert np.isfinite(vel).all() and np.abs(vel).max() > 0
                w, q = d.gradient_fields(vel_name, scale)
                rw, rq = gref.gradient_fields(vel, g.neighbor_table, g.obstacle, scale)
                assert np.array_equal(w, rw), f"{name} level {g.level_id} {vel_name}: vorticity"
                assert np.array_equal(q, rq), f"{name} level {g.level_id} {vel_name}: Q"
                nu, code = d.subgrid_fields(vel_name)
                rn, rc = sref.fields(vel, g.neighbor_table, g.obstacle, params.c_wale, params.nu_sgs_bg)
                assert np.array_equal(nu, rn), f"{name} level {g.level_id} {vel_name}: nu_t"
                assert np.array_equal(code, rc), f"{name} level {g.level_id} {vel_name}: code"
                assert np.abs(w).max() > 0 and (code > 0).any()
    finally:
        for d in dev:
            d.close()
