"""The record step's host side, without a GPU: the two entry points it adds to the C ABI (header, ctypes binding, exported symbols,
switch table) and its eligibility rule - ludwig_record_step_rule - on the topology fixtures of tests/_topology_cases.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _topology_cases as tc
from open_ludwig_amd import _lib, build, cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_NEIGHBOURS, HAS_OBSTACLE, HAS_SPONGE, HAS_NEAR_WALL, STORE_POST = 1, 2, 4, 8, 16      # csrc/lattice.hpp FLAG_*


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def block_flags(level):
    """the per-block flags word as the library forms it from the level's topology and geometry fields (csrc/ludwig_hip.hip scan_flags)"""
    fl = tc.all_neighbour_blocks(level).astype(np.int32) * ALL_NEIGHBOURS
    per_block = lambda a: np.asarray(a).reshape(-1, np.asarray(a).shape[3], order="F").any(axis=0)
    fl |= per_block(np.asarray(level.obstacle) != 0).astype(np.int32) * HAS_OBSTACLE
    fl |= per_block(np.asarray(level.sponge) > 0).astype(np.int32) * HAS_SPONGE
    wd = np.asarray(level.wall_dist)
    fl |= per_block((wd > 0) & (wd < 10)).astype(np.int32) * HAS_NEAR_WALL
    return np.ascontiguousarray(fl, dtype=np.int32)


def rule(lib, flags, n_owned=None, parent=0, temporal=0, post=0, wall=0):
    flags = np.ascontiguousarray(flags, dtype=np.int32)
    n = flags.size
    return lib.ludwig_record_step_rule(flags.ctypes.data if n else None, n, n if n_owned is None else n_owned, parent, temporal, post, wall)


def test_abi_additions(lib):
    header = open(os.path.join(ROOT, "include", "ludwig_hip.h")).read()
    for name in ("ludwig_record_step_rule", "ludwig_level_record_steps"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert lib.ludwig_abi_version() == 1                       # new symbols, no struct touched
    assert lib.ludwig_record_step_rule.argtypes == [C.c_void_p] + [C.c_int] * 6
    n = C.c_int64(-1)
    assert lib.ludwig_level_record_steps(None, C.byref(n)) == -1 and b"null" in lib.ludwig_last_error()
    assert lib.ludwig_record_step_rule(None, 3, 3, 0, 0, 0, 0) == -1
    assert lib.ludwig_record_step_rule(None, -1, -1, 0, 0, 0, 0) == -1
    julia = open(os.path.join(ROOT, "julia", "LudwigHIP.jl")).read()
    assert "ludwig_level_record_steps" in julia and "ludwig_record_step_rule" in julia
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`LUDWIG_RECORD_STEP=0`" in doc and "`LUDWIG_RECORD_ORDER=0/1`" in doc


def test_rule_on_plain_flags(lib):
    plain = np.full(12, ALL_NEIGHBOURS, np.int32)
    assert rule(lib, plain) == 1
    assert rule(lib, np.zeros(0, np.int32)) == 0                                   # an empty level
    assert rule(lib, plain, n_owned=8) == 0                                        # ghost blocks: more than one rank
    assert rule(lib, plain, parent=1) == 0 and rule(lib, plain, temporal=1) == 0
    assert rule(lib, plain, post=1) == 0 and rule(lib, plain, wall=1) == 0
    for bit in (HAS_OBSTACLE, HAS_SPONGE, HAS_NEAR_WALL, STORE_POST):
        one = plain.copy()
        one[7] |= bit
        assert rule(lib, one) == 0, bit
    edge = plain.copy()
    edge[0] = 0                                                                    # a block with a missing neighbour
    assert rule(lib, edge) == 0


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_rule_on_topology_fixtures(lib, name):
    """a fixture level steps by records exactly when it is a single all-periodic level of plain cells"""
    grids, params = tc.CASES[name].build()
    for i, g in enumerate(grids):
        fl = block_flags(g)
        got = rule(lib, fl, parent=int(i > 0), temporal=int(g.f_old is not None and np.asarray(g.f_old).size > 0),
                   post=int(g.n_boundary_cells > 0), wall=int(params.wall_model_active))
        plain = bool((fl == ALL_NEIGHBOURS).all())
        want = len(grids) == 1 and plain and not params.wall_model_active and g.n_boundary_cells == 0
        if want:
            assert name.startswith("periodic_"), name
        assert got == int(want and not (g.f_old is not None and np.asarray(g.f_old).size > 0)), (name, i)


def test_rule_on_boxes_with_one_special_cell(lib):
    grids, _ = cases.periodic_box((2, 2, 1))
    g = grids[0]
    assert rule(lib, block_flags(g)) == 1
    g.obstacle[3, 4, 5, 1] = True
    assert rule(lib, block_flags(g)) == 0
    g.obstacle[3, 4, 5, 1] = False
    g.sponge[1, 1, 1, 2] = np.float32(0.5)
    assert rule(lib, block_flags(g)) == 0
    g.sponge[1, 1, 1, 2] = 0
    g.wall_dist[0, 0, 0, 3] = np.float32(2.0)
    assert rule(lib, block_flags(g)) == 0
