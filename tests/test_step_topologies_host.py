"""The topology table (tests/_topology_cases.py) on the host: reference against reference, and what the table contains.

Oracle against float64: every case runs 4 coarse steps through the CPU oracle; before every step tests/_step_ref.py restates that one
step in float64 from the oracle's float32 state, and the oracle's result is compared under the bounds, the north star and the
exclusion cap of tests/_step_ref.py - the same StepCheck, the same constants as tests/test_step_reference_host.py.

Rounding bound: no case's e_ref (ref32 against ref64) exceeds the recorded MAX_E_REF.

Census: counted from neighbor_table, map_x/y/z and the domain extent alone, the table holds a level-1 pull whose source block is
missing inside the domain (the w_k arm), fine-level pulls with a missing source block beyond each of the six domain faces, re-entrant
corners, blocks that are their own neighbour along each axis, a block whose two x neighbours coincide, and same-kind x-chains of
every length 1..7; the body of nest_with_body has Bouzidi cells in both block classes. -s prints per case the block counts, e_ref, the oracle's error as a share of the bound and the excluded share.

Stencil observers: the restatements the device test compares with (tests/_gradient_ref.py, tests/_subgrid_ref.py) are checked once on
the level-1 table with holes against the neighbour rule written out cell by cell.
"""
import time

import numpy as np
import pytest

import _gradient_ref as gref
import _step_ref as sr
import _step_ref_cases as sc
import _subgrid_ref as sref
import _topology_cases as tc
from oracle import oracle

F32 = np.float32
KINDS = ("f", "vel", "rho")
_census = {}


def _state(level, ref):
    names = [ref.f_name, ref.vel_name, "rho"]
    if ref.post_read is not None:
        names.append("f_post_collision")
    if ref.old is not None:
        names += ["f_old", "rho_old", "vel_old"]
    return {n: getattr(level, n) for n in names}


def _pull_census(level, params):
    """per population and cell: is the source block missing, and where does the source cell lie - from the table, the maps and the extent"""
    geom = sr._Geom(level, params)
    shape = (sr.B, sr.B, sr.B, level.n_blocks)
    out = dict.fromkeys(("inside", "x_min", "x_max", "y_min", "y_max", "z_min", "z_max"), 0)
    for k in range(27):
        missing = ~geom.neighbour(-sr.C_K[k])[4]
        if not missing.any():
            continue
        s = [np.broadcast_to(geom.g[a] - sr.C_K[k][a], shape) for a in range(3)]
        beyond = {"x_min": s[0] < 1, "x_max": s[0] > geom.n_glob[0], "y_min": s[1] < 1, "y_max": s[1] > geom.n_glob[1],
                  "z_min": s[2] < 1, "z_max": s[2] > geom.n_glob[2]}
        inside = missing.copy()
        for name, m in beyond.items():
            out[name] += int((missing & m).sum())
            inside &= ~m
        out["inside"] += int(inside.sum())
    return out


def _reentrant_corners(level):
    """(block, diagonal direction) pairs: the diagonal block is absent although the axis neighbours it lies between all exist"""
    t = np.asarray(level.neighbor_table)
    n = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                d = (dx, dy, dz)
                if sum(v != 0 for v in d) < 2:
                    continue
                axes = [tuple(v if a == i else 0 for a, v in enumerate(d)) for i in range(3) if d[i]]
                ok = t[:, tc.direction(*d)] == 0
                for e in axes:
                    ok &= t[:, tc.direction(*e)] > 0
                n += int(ok.sum())
    return n


def _self_neighbours(level):
    """along each axis: blocks that are their own + and - neighbour; and blocks whose +x and -x neighbours coincide without being the block"""
    t = np.asarray(level.neighbor_table)
    me = np.arange(level.n_blocks) + 1
    own = []
    for a in range(3):
        e = [int(a == i) for i in range(3)]
        own.append(int(((t[:, tc.direction(*e)] == me) & (t[:, tc.direction(*(-v for v in e))] == me)).sum()))
    east, west = t[:, tc.direction(1, 0, 0)], t[:, tc.direction(-1, 0, 0)]
    return own, int(((east == west) & (east > 0) & (east != me)).sum())


def _body_census(level, params):
    """Bouzidi cells in all-neighbour and in general blocks, and obstacle cells on a domain face"""
    fast = tc.all_neighbour_blocks(level)[np.asarray(level.bouzidi_cell_block).astype(np.int64) - 1]
    geom = sr._Geom(level, params)
    obs = np.asarray(level.obstacle).astype(bool)
    at_face = np.zeros(obs.shape, dtype=bool)
    for a in range(3):
        at_face |= (geom.g[a] == 1) | (geom.g[a] == geom.n_glob[a])
    return int(fast.sum()), int((~fast).sum()), int((obs & at_face).sum())


def run_case(name):
    t0 = time.perf_counter()
    case = tc.CASES[name]
    grids, params = case.build()
    entry = {"blocks": [g.n_blocks for g in grids], "fast": [int(tc.all_neighbour_blocks(g).sum()) for g in grids],
             "e_ref": dict.fromkeys(KINDS, 0.0), "err": dict.fromkeys(KINDS, 0.0), "excluded": 0.0,
             "pulls": [_pull_census(g, params) for g in grids], "corners": [_reentrant_corners(g) for g in grids],
             "self": [_self_neighbours(g) for g in grids], "chains": sorted({len(c) for g in grids for c in tc.x_chains(g)}),
             "body": [_body_census(g, params) for g in grids]}
    for t in case.steps:
        check = sc.StepCheck(grids, params, t, case.u)
        oracle.execute_timestep_batch(grids, t, 1, F32(case.u), params)
        for k in KINDS:
            entry["e_ref"][k] = max(entry["e_ref"][k], check.e_ref[k])
        for lv, g in enumerate(grids):
            share = check.excluded_share[lv]
            entry["excluded"] = max(entry["excluded"], share)
            assert share <= sr.MAX_EXCLUDED_SHARE, f"{name} t={t} level {lv + 1}: {share:.4%} of the fluid cells left out"
            err = check.compare(lv, g, _state(g, check.ref[lv]), f"{name} t={t}")
            for k in err:
                entry["err"][k] = max(entry["err"][k], err[k])
    entry["seconds"] = time.perf_counter() - t0
    return entry


def census(name):
    """one run per case and session, whichever test asks first"""
    if name not in _census:
        _census[name] = run_case(name)
    return _census[name]


@pytest.mark.parametrize("name", list(tc.CASES))
def test_oracle_step_matches_float64_restatement(name):
    census(name)


def _whole_table():
    for name in tc.CASES:
        census(name)


def test_float32_rounding_stays_under_the_recorded_bound():
    """MAX_E_REF was measured on the table of tests/_step_ref_cases.py; the topologies may not need a larger one"""
    _whole_table()
    print("\ncase               blocks (all-neighbour)          s   excluded  e_ref f/vel/rho                  oracle err / bound f/vel/rho")
    for name, c in _census.items():
        blocks = " ".join(f"{n}({f})" for n, f in zip(c["blocks"], c["fast"]))
        print(f"{name:18s} {blocks:28s} {c['seconds']:5.1f} {c['excluded']:9.5%}  " + " ".join(f"{c['e_ref'][k]:.3e}" for k in KINDS)
              + "   " + " ".join(f"{c['err'][k] / sr.bound(k):.3f}" for k in KINDS))
    for kind in KINDS:
        measured = max(c["e_ref"][kind] for c in _census.values())
        worst = max(c["err"][kind] for c in _census.values())
        print(f"max e_ref {kind}: {measured:.4e} (recorded {sr.MAX_E_REF[kind]:.4e})   oracle max err {worst:.4e} = {worst / sr.bound(kind):.3f} of the bound")
        assert measured <= sr.MAX_E_REF[kind], f"{kind}: e_ref {measured:.4e} above MAX_E_REF {sr.MAX_E_REF[kind]:.4e}"
    print(f"largest excluded share {max(c['excluded'] for c in _census.values()):.5%}, seconds {sum(c['seconds'] for c in _census.values()):.1f}")


def test_table_holds_the_topologies_it_was_built_for():
    _whole_table()
    faces = ("x_min", "x_max", "y_min", "y_max", "z_min", "z_max")
    level1_inside = sum(c["pulls"][0]["inside"] for c in _census.values())
    fine = {f: sum(p[f] for c in _census.values() for p in c["pulls"][1:]) for f in faces + ("inside",)}
    fine_corners = sum(n for c in _census.values() for n in c["corners"][1:])
    own = [sum(s[0][a] for c in _census.values() for s in c["self"]) for a in range(3)]
    twins = sum(s[1] for c in _census.values() for s in c["self"])
    chains = sorted({n for c in _census.values() for n in c["chains"]})
    print(f"\nlevel-1 pulls with a missing source inside the domain: {level1_inside}")
    print("fine-level pulls with a missing source: " + " ".join(f"{k} {v}" for k, v in fine.items()))
    print(f"fine-level re-entrant corners (block, direction): {fine_corners}")
    print(f"blocks that are their own x / y / z neighbour: {own}; blocks whose +x and -x neighbours coincide: {twins}")
    print(f"same-kind x-chain lengths: {chains}")
    assert level1_inside > 0
    assert _census["level1_holes"]["pulls"][0]["inside"] > 0
    for f in faces + ("inside",):
        assert fine[f] > 0, f"no fine-level pull with a missing source block at {f}"
    assert fine_corners > 0
    assert all(n > 0 for n in own), own
    assert twins > 0
    assert set(range(1, 8)) <= set(chains), chains
    # what each named case was built for
    assert _census["level1_holes"]["chains"] == [1, 2, 3, 5, 6]
    assert _census["slab_nest"]["fast"] == [0, 0] and 10 in _census["slab_nest"]["chains"]
    assert _census["nest_with_body"]["fast"] == [5, 8]
    in_fast, in_general, at_face = _census["nest_with_body"]["body"][1]
    print(f"nest_with_body: Bouzidi cells in all-neighbour blocks {in_fast}, in general blocks {in_general}; obstacle cells on a domain face {at_face}")
    assert in_fast > 0 and in_general > 0 and at_face == 0
    assert _census["ragged_nest"]["blocks"] == [45, 56, 32] and all(n > 0 for n in _census["ragged_nest"]["corners"][1:])
    for f in faces:
        assert _census["ragged_nest"]["pulls"][1][f] > 0, f
    assert _census["periodic_2x1x1"]["self"][0][1] == 2
    assert all(len(c["blocks"]) <= tc.MAX_LEVELS and max(c["blocks"]) <= tc.MAX_BLOCKS for c in _census.values())
    assert sum(len(c["blocks"]) == 3 for n, c in _census.items() if n.startswith("random_")) == len(tc.RANDOM_SEEDS) // 2


def test_random_generator_keeps_its_ranges():
    drawn = {"temporal": set(), "symmetric": set(), "noise": set()}
    for seed, three in tc.RANDOM_SEEDS.items():
        dims, l1, p2, p3, flags = tc.random_topology(seed, three)
        n = dims[0] * dims[1] * dims[2]
        assert 4 <= dims[0] <= 6 and 2 <= dims[1] <= 3 and 2 <= dims[2] <= 3
        assert 0.85 * n - 0.5 <= len(l1) <= n and len(set(l1)) == len(l1)
        assert 0.20 * len(l1) - 0.5 <= len(p2) <= 0.40 * len(l1) + 0.5 and set(p2) <= set(l1)
        assert bool(p3) == three
        if p3:
            assert 0.10 * 8 * len(p2) - 0.5 <= len(p3) <= 0.25 * 8 * len(p2) + 0.5 and set(p3) <= set(tc.children(p2))
        assert tc.random_topology(seed, three) == (dims, l1, p2, p3, flags)
        for k in drawn:
            drawn[k].add(flags[k])
    assert drawn == {"temporal": {False, True}, "symmetric": {False, True}, "noise": {0.0, 0.01}}, drawn
    # the replacement rule: from 1 upward, two and three levels in turn, the next integer wherever a level exceeds the cap
    want, seed = {}, 0
    for three in (False, True) * 3:
        seed += 1
        while tc.random_topology(seed, three) is None:
            seed += 1
        want[seed] = three
    assert tc.RANDOM_SEEDS == want, want


def test_children_are_the_eight_blocks_under_each_parent():
    got = tc.children([(1, 1, 1), (3, 2, 5)])
    assert len(got) == 16 and got[0] == (1, 1, 1) and got[7] == (2, 2, 2)
    assert {((x + 1) // 2, (y + 1) // 2, (z + 1) // 2) for x, y, z in got} == {(1, 1, 1), (3, 2, 5)}


# ---- the observers' restatements on a table with holes, against the literal neighbour rule ----
def _holes_level_with_random_velocity():
    grids, params = tc.CASES["level1_holes"].build()
    g = grids[0]
    rng = np.random.default_rng(8)
    vel = rng.standard_normal((8, 8, 8, g.n_blocks, 3)).astype(F32) * F32(0.05)
    obst = rng.random((8, 8, 8, g.n_blocks)) < 0.1
    return g, params, vel, obst


CELLS = [(0, 0, 0), (7, 3, 5), (4, 7, 0), (2, 5, 7), (7, 7, 7), (0, 4, 4), (3, 0, 7)]


def test_gradient_restatement_equals_the_literal_neighbour_rule_around_the_holes():
    g, _, u, obst = _holes_level_with_random_velocity()
    scale = F32(1.0 / 0.37)
    w, q = gref.gradient_fields(u, g.neighbor_table, obst, scale)
    e = np.eye(3, dtype=int)
    for b in range(g.n_blocks):
        for (x, y, z) in CELLS:
            nv = lambda d: gref.neighbor_value(u, g.neighbor_table, x, y, z, b, *d)
            gr = [[(F32(0.5) * (nv(e[j])[i] - nv(-e[j])[i])) * scale for j in range(3)] for i in range(3)]
            if obst[x, y, z, b]:
                want_w, want_q = [F32(0)] * 3, F32(0)
            else:
                want_w = [gr[2][1] - gr[1][2], gr[0][2] - gr[2][0], gr[1][0] - gr[0][1]]
                want_q = F32(-0.5) * (((gr[0][0] * gr[0][0] + gr[1][1] * gr[1][1]) + gr[2][2] * gr[2][2])
                                      + F32(2.0) * ((gr[0][1] * gr[1][0] + gr[0][2] * gr[2][0]) + gr[1][2] * gr[2][1]))
            assert [w[x, y, z, b, k] for k in range(3)] == want_w, (b, x, y, z)
            assert q[x, y, z, b] == want_q, (b, x, y, z)


def test_subgrid_restatement_equals_the_literal_neighbour_rule_around_the_holes():
    g, params, vel, _ = _holes_level_with_random_velocity()
    nu, s2, code = sref.state(vel, g.neighbor_table, params.c_wale, params.nu_sgs_bg)
    for b in range(g.n_blocks):
        for (x, y, z) in CELLS:
            gm = np.empty((3, 3), dtype=F32)
            for j, d in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
                hi = gref.neighbor_value(vel, g.neighbor_table, x, y, z, b, *d)
                lo = gref.neighbor_value(vel, g.neighbor_table, x, y, z, b, *(-k for k in d))
                gm[:, j] = F32(0.5) * (hi - lo)
            with np.errstate(all="ignore"):
                one = sref.wale_state([[gm[i, j].reshape(1) for j in range(3)] for i in range(3)], params.c_wale, params.nu_sgs_bg)
            for got, want in zip((nu, s2, code), one):
                assert np.asarray(got[x, y, z, b]).tobytes() == np.asarray(want[0]).tobytes(), (b, x, y, z)
