"""The CPU oracle against an independent float64 restatement of the step (tests/_step_ref.py), one coarse step at a time.

The oracle runs each case of tests/_step_ref_cases.py for 4 coarse steps. Before every step the restatement reads the oracle's full
float32 state and computes that one step in float64 (expected values) and in float32 (calibration and branch record); the oracle
then takes the step and is compared. Rounding never accumulates: every step is an independent sample.

Asserted per step, level and field class: error / scale <= MARGIN * MAX_E_REF (tests/_step_ref.py: measured from ref32 against ref64,
not from the oracle); rho and u within the 1e-5 north star; the cells left out - where ref32 and ref64 branch differently, and the
readers of such cells within the step - stay under 0.5 % of the level's fluid cells, and are none at all where the start is smooth
and no wall model runs. The oracle exposes no branch record: a wrong branch shows through the value bound at the comparable cells.

The census test prints what DESIGN.md section 5 quotes (-s shows it) and checks that the table populates the branches it was built
for on both sides.
"""
import time

import numpy as np
import pytest

import _step_ref as sr
import _step_ref_cases as sc
from oracle import oracle

F32 = np.float32
_census = {}            # case -> dict(e_ref, err, excluded, branches set / clear counts)


def _state(level, check, lv):
    ref = check.ref[lv]
    names = [ref.f_name, ref.vel_name, "rho"]
    if ref.post_read is not None:
        names.append("f_post_collision")
    if ref.old is not None:
        names += ["f_old", "rho_old", "vel_old"]
    return {n: getattr(level, n) for n in names}


def run_case(name, stepper=None):
    """steps the case with the oracle (or `stepper(grids, params, t, u)`), checks every step, returns the census entry"""
    case = sc.CASES[name]
    grids, params = case.build()
    entry = {"e_ref": dict.fromkeys(("f", "vel", "rho"), 0.0), "err": dict.fromkeys(("f", "vel", "rho"), 0.0), "excluded": 0.0,
             "set": dict.fromkeys(sr.BRANCH_NAMES, 0), "clear": dict.fromkeys(sr.BRANCH_NAMES, 0), "branch_diff": 0}
    for t in case.steps:
        check = sc.StepCheck(grids, params, t, case.u)
        if stepper is None:
            oracle.execute_timestep_batch(grids, t, 1, F32(case.u), params)
        else:
            stepper(grids, params, t, case.u)
        for k in entry["e_ref"]:
            entry["e_ref"][k] = max(entry["e_ref"][k], check.e_ref[k])
        for lv, g in enumerate(grids):
            share = check.excluded_share[lv]
            entry["excluded"] = max(entry["excluded"], share)
            entry["branch_diff"] += check.branch_diff[lv]
            assert share <= sr.MAX_EXCLUDED_SHARE, f"{name} t={t} level {lv + 1}: {share:.4%} of the fluid cells left out"
            if case.smooth and not case.wall:
                assert share == 0 and check.branch_diff[lv] == 0, f"{name} t={t} level {lv + 1}: cells left out of a smooth case"
            err = check.compare(lv, g, _state(g, check, lv), f"{name} t={t}")
            for k in err:
                entry["err"][k] = max(entry["err"][k], err[k])
            fluid = ~np.asarray(g.obstacle).astype(bool)
            for br in check.ref[lv].branches:
                for bit in sr.BRANCH_NAMES:
                    on = (br & bit) != 0
                    entry["set"][bit] += int(on.sum())
                    entry["clear"][bit] += int((~on & fluid).sum())
    return entry


@pytest.mark.parametrize("name", list(sc.CASES))
def test_oracle_step_matches_float64_restatement(name):
    t0 = time.perf_counter()
    _census[name] = run_case(name)
    _census[name]["seconds"] = time.perf_counter() - t0


def test_measured_float32_rounding_is_what_the_bounds_were_taken_from():
    """MAX_E_REF is the maximum of e_ref over the case table: no case may exceed it, and it may not be padded beyond 1.5 x of what the
    table gives (so that the bound follows the reference's own rounding, not a convenient figure)."""
    assert set(_census) == set(sc.CASES), "run the whole file: this test reads the cases' results"
    for kind in ("f", "vel", "rho"):
        measured = max(c["e_ref"][kind] for c in _census.values())
        assert measured <= sr.MAX_E_REF[kind], f"{kind}: e_ref {measured:.4e} above MAX_E_REF {sr.MAX_E_REF[kind]:.4e}"
        assert sr.MAX_E_REF[kind] <= 1.5 * measured, f"{kind}: MAX_E_REF {sr.MAX_E_REF[kind]:.4e} padded over the measured {measured:.4e}"
        worst = max(c["err"][kind] for c in _census.values())
        assert worst <= sr.ORACLE_MAX_ERR[kind] * 1.02, f"{kind}: oracle error {worst:.4e} above the recorded {sr.ORACLE_MAX_ERR[kind]:.4e}"
    assert sr.MARGIN == 4.0


def test_branch_census():
    """Every data-dependent branch of the step is taken AND not taken somewhere in the table, except two sides no state can reach:
    WM_LAW clear needs u+ = ln(y+) / 0.41 + 5.2 <= 0.1 inside y+ > 11.81, where it is at least 11.2; the Bouzidi bits are clear at
    every unlisted cell."""
    assert set(_census) == set(sc.CASES), "run the whole file: this test reads the cases' results"
    total_set = {b: sum(c["set"][b] for c in _census.values()) for b in sr.BRANCH_NAMES}
    total_clear = {b: sum(c["clear"][b] for c in _census.values()) for b in sr.BRANCH_NAMES}
    print("\ncase                                  s   excluded  e_ref f/vel/rho                  oracle err f/vel/rho")
    for name, c in _census.items():
        print(f"{name:36s} {c['seconds']:5.1f} {c['excluded']:9.5%}  " + " ".join(f"{c['e_ref'][k]:.3e}" for k in ("f", "vel", "rho"))
              + "   " + " ".join(f"{c['err'][k]:.3e}" for k in ("f", "vel", "rho")))
    for kind in ("f", "vel", "rho"):
        print(f"max e_ref {kind}: {max(c['e_ref'][kind] for c in _census.values()):.4e}   oracle max err: {max(c['err'][kind] for c in _census.values()):.4e}")
    print(f"largest excluded share {max(c['excluded'] for c in _census.values()):.5%}, cells with differing branches "
          f"{sum(c['branch_diff'] for c in _census.values())}, seconds {sum(c['seconds'] for c in _census.values()):.1f}")
    for b, n in sr.BRANCH_NAMES.items():
        print(f"  {n:16s} set {total_set[b]:9d}  clear {total_clear[b]:9d}")
    for b, n in sr.BRANCH_NAMES.items():
        assert total_set[b] > 0, f"no cell takes {n}"
        if b != sr.WM_LAW:
            assert total_clear[b] > 0, f"no fluid cell leaves {n}"
    # the wall-model conditions are nested: the clear side has to be populated INSIDE the enclosing one
    assert total_set[sr.WM_DIST] > total_set[sr.WM_UMAG] > total_set[sr.WM_YPLUS] > 0
    assert total_set[sr.WM_UMAG] > total_set[sr.WM_FORCE] > 0
    assert total_set[sr.WALE_OP1] > total_set[sr.WALE_DENOM] > total_set[sr.WALE_EDDY] > 0
    # each special case holds the branch it was built for
    assert _census["omega_floor"]["set"][sr.OMEGA_FLOOR] > 0 and _census["omega_floor"]["clear"][sr.OMEGA_FLOOR] > 0
    assert _census["density_clamp"]["set"][sr.RHO_CLAMP] > 0
    assert _census["wall_at_rest"]["set"][sr.WM_DIST] > _census["wall_at_rest"]["set"][sr.WM_UMAG]
    assert _census["thin_yz"]["set"][sr.BZ_NO_BEHIND] > 0 and _census["thin_yz"]["set"][sr.BZ_OUT_OF_RANGE] > 0
    for name, c in _census.items():
        if "_z1" in name or name.startswith("thin"):
            assert c["set"][sr.BZ_LT_HALF] > 0 and c["set"][sr.BZ_GE_HALF] > 0, name
        if sc.CASES[name].wall:
            assert c["set"][sr.WM_DIST] > 0, name


def test_tunnel_table_is_pairwise():
    rows = sc.TUNNEL_TABLE
    for i in range(7):
        for j in range(i + 1, 7):
            want = {(a, b) for a in ((1, 2, 3) if i == 0 else (0, 1)) for b in (0, 1)}
            assert {(r[i], r[j]) for r in rows} == want, (i, j)
    for case in sc.CASES.values():
        assert len(case.steps) >= 4 and {t % 2 for t in case.steps} == {0, 1}


def test_pull_sources_cover_every_edge_condition():
    """the static side of the case table: each stand-in for a missing pull source occurs, including the competitions the cases were built
    for (a cell at a y and a z mirror at once; a fine cell whose missing source is outside y-min, where mirror wins over interface)"""
    grids, params = sc.CASES["thin_yz"].build()
    g = sr.geometry(grids[0], params)
    codes = np.stack([g.code(k) for k in range(27)], axis=-1)
    for c in (sr._INLET, sr._OUTLET, sr._YMIR, sr._ZMIR):
        assert (codes == c).any()
    assert (((codes == sr._YMIR).any(axis=-1)) & ((codes == sr._ZMIR).any(axis=-1))).any()
    assert not (codes == sr._WEIGHT).any()
    grids, params = sc.CASES["interface_at_ymin"].build()
    g = sr.geometry(grids[1], params)
    codes = np.stack([g.code(k) for k in range(27)], axis=-1)
    both = (codes == sr._IFACE).any(axis=-1) & (codes == sr._YMIR).any(axis=-1)
    assert both.any() and (codes == sr._INLET).any()


def test_noise_restated_exactly():
    """gradient_noise against the oracle's export of the same function (integer hash: exact), at seeds around the wrap"""
    L = oracle.lib()
    for a, b, c in [(1, 1, 0), (17, 33, 999999), (64, 5, 0), (8, 8, 123456), (31, 2, 1)]:
        assert sr.gradient_noise(a, b, c, 1234) == L.oracle_gradient_noise(a, b, c, 1234)
