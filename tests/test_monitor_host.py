"""The flow monitor without a GPU: host_monitor against brute-force definitions (loops over cells, nothing vectorised), the tree sum
against the halving definition, merge of per-rank records, cell coordinates against the flow file's geometry and the probes' frame, the
advanced.flow_monitor keys, the CSV text and the warnings. Every comparison is exact unless it says otherwise."""
import math
import os

import numpy as np
import pytest

from open_ludwig_amd import cases, monitor as mon, output as out_mod, preprocess as pp, probes as pm

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BALL = os.path.join(G, "ball1m_config.yaml")
F32, F64 = np.float32, np.float64


def _halving(x):
    """the definition, in plain Python floats: x = x[0::2] + x[1::2] with +0.0 appended when the length is odd"""
    x = [float(v) for v in x]
    if not x:
        return 0.0
    while len(x) > 1:
        if len(x) % 2:
            x.append(0.0)
        x = [x[i] + x[i + 1] for i in range(0, len(x), 2)]
    return x[0]


def brute(rho, vel, obstacle, coords):
    """the record by its definition, cell by cell"""
    nb = rho.shape[3]
    rec = mon.Record()
    best = {"rho_min": None, "rho_max": None, "v2_max": None}      # (value, key)
    first_bad = None
    s_rho, s_rv2 = [], []
    for b in range(nb):
        br, bv = [], []
        for c in range(512):
            i, j, k = c % 8, (c // 8) % 8, c // 64
            term_r = term_v = 0.0
            if not obstacle[i, j, k, b]:
                rec.n_fluid += 1
                r = F32(rho[i, j, k, b])
                ux, uy, uz = (F32(vel[i, j, k, b, a]) for a in range(3))
                with np.errstate(over="ignore", invalid="ignore"):
                    v2 = F32(F32(F32(ux * ux) + F32(uy * uy)) + F32(uz * uz))
                key = tuple(int(v) for v in coords[b]) + (c,)
                if all(math.isfinite(float(v)) for v in (r, ux, uy, uz, v2)):
                    term_r, term_v = float(r), float(r) * float(v2)
                    for name, val, better in (("rho_min", r, lambda a, b_: a < b_), ("rho_max", r, lambda a, b_: a > b_),
                                              ("v2_max", v2, lambda a, b_: a > b_)):
                        cur = best[name]
                        if cur is None or better(val, cur[0]) or (val == cur[0] and key < cur[1]):
                            best[name] = (val, key)
                else:
                    rec.n_bad += 1
                    if first_bad is None or key < first_bad:
                        first_bad = key
            br.append(term_r)
            bv.append(term_v)
        s_rho.append(_halving(br))
        s_rv2.append(_halving(bv))
    for name, got in best.items():
        if got is not None:
            setattr(rec, name, got[0])
            setattr(rec, "cell_" + name, got[1])
    rec.first_bad = first_bad
    rec.sum_rho, rec.sum_rho_v2 = F64(_halving(s_rho)), F64(_halving(s_rv2))
    return rec


def _level(shape, seed):
    grids, _ = cases.periodic_box(shape, init=False)
    g = grids[0]
    cases.init_perturbed(g, seed)
    return g


def _same(a: mon.Record, b: mon.Record):
    assert a == b, f"\n{a}\n{b}"
    for name in ("rho_min", "rho_max", "v2_max", "sum_rho", "sum_rho_v2"):        # == lets -0.0 pass for +0.0: the bits too
        x, y = getattr(a, name), getattr(b, name)
        if x != 0:
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), name


@pytest.mark.parametrize("shape,seed", [((1, 1, 1), 1), ((3, 1, 1), 2), ((2, 2, 3), 3)])
def test_host_monitor_equals_the_definition_on_random_levels(shape, seed):
    g = _level(shape, seed)
    rng = np.random.default_rng(seed)
    g.obstacle[...] = rng.random(g.obstacle.shape) < 0.2
    rec = mon.host_monitor(g.rho, g.vel, g.obstacle, g.active_block_coords)
    _same(rec, brute(g.rho, g.vel, g.obstacle, g.active_block_coords))
    assert rec.n_bad == 0 and rec.first_bad is None and rec.n_fluid == int((~g.obstacle).sum())
    assert rec.rho_mean == float(rec.sum_rho) / rec.n_fluid and rec.kinetic_energy == 0.5 * float(rec.sum_rho_v2)
    fluid_speed = np.sqrt(((g.vel.astype(F64) ** 2).sum(axis=4))[~g.obstacle]).max()
    assert rec.speed_max == pytest.approx(fluid_speed, rel=1e-6) and rec.mach == rec.speed_max * math.sqrt(3.0)


def test_non_finite_overflow_signed_zeros_ties_and_hidden_extremes():
    g = _level((2, 2, 3), 5)
    nb = g.n_blocks
    g.obstacle[...] = False
    g.obstacle[:, :, :, 4] = True                                   # an all-obstacle block
    g.rho[...] = np.abs(g.rho)
    g.rho[3, 2, 1, 7] = np.nan
    g.vel[1, 1, 1, 2, 0] = np.inf
    g.vel[1, 1, 2, 2, 2] = -np.inf
    g.vel[5, 5, 5, 9, 1] = F32(3e19)                                # finite, its square is not
    g.vel[0, 0, 0, 0, :] = (F32(1.1e19), F32(1.1e19), F32(1.1e19))  # each square finite, the sum is not
    # equal minima in two blocks, the later block listed first in memory order of the plant
    g.rho[7, 7, 7, 10] = F32(0.25)
    g.rho[0, 1, 0, 3] = F32(0.25)
    # +0.0 and -0.0 speeds tie: the whole of block 1 at rest with mixed signs
    g.vel[:, :, :, 1, :] = F32(0.0)
    g.vel[2, 0, 0, 1, :] = F32(-0.0)
    # extremes hidden in obstacle cells
    g.obstacle[4, 4, 4, 6] = True
    g.rho[4, 4, 4, 6] = F32(1e-9)
    g.obstacle[4, 4, 5, 6] = True
    g.rho[4, 4, 5, 6] = F32(77.0)
    g.vel[4, 4, 5, 6, :] = F32(9.0)
    g.obstacle[4, 5, 5, 6] = True
    g.rho[4, 5, 5, 6] = np.nan
    rec = mon.host_monitor(g.rho, g.vel, g.obstacle, g.active_block_coords)
    _same(rec, brute(g.rho, g.vel, g.obstacle, g.active_block_coords))
    assert rec.n_bad == 5 and rec.n_fluid == (nb - 1) * 512 - 3
    assert rec.first_bad == tuple(g.active_block_coords[0]) + (0,)
    assert rec.rho_min == F32(0.25) and rec.cell_rho_min == tuple(g.active_block_coords[3]) + (8,)
    assert float(rec.rho_max) < 77.0 and math.isfinite(float(rec.v2_max)) and float(rec.v2_max) < 1.0
    # shuffling the block order moves no extreme and no cell: the tie rule is about coordinates
    perm = np.random.default_rng(0).permutation(nb)
    shuffled = mon.host_monitor(g.rho[:, :, :, perm], g.vel[:, :, :, perm], g.obstacle[:, :, :, perm],
                                [g.active_block_coords[p] for p in perm])
    assert shuffled.same_but_sums(rec)


def test_zero_sign_tie_takes_the_lowest_cell():
    g = _level((1, 1, 1), 9)
    g.obstacle[...] = False
    g.vel[...] = F32(0.0)
    g.vel[3, 0, 0, 0, 0] = F32(-0.0)
    g.rho[...] = F32(1.0)
    g.rho[5, 0, 0, 0] = F32(-0.0)
    g.rho[6, 0, 0, 0] = F32(0.0)
    rec = mon.host_monitor(g.rho, g.vel, g.obstacle, g.active_block_coords)
    _same(rec, brute(g.rho, g.vel, g.obstacle, g.active_block_coords))
    assert rec.cell_v2_max == (1, 1, 1, 0) and rec.cell_rho_min == (1, 1, 1, 5) and rec.cell_rho_max == (1, 1, 1, 0)
    assert np.signbit(rec.rho_min)


def test_level_with_every_fluid_cell_bad_and_empty_levels():
    g = _level((3, 1, 1), 4)
    g.obstacle[...] = False
    g.obstacle[:, :, 0, :] = True
    g.rho[...] = np.nan
    rec = mon.host_monitor(g.rho, g.vel, g.obstacle, g.active_block_coords)
    _same(rec, brute(g.rho, g.vel, g.obstacle, g.active_block_coords))
    assert rec.n_bad == rec.n_fluid == 3 * 448 and rec.n_counted == 0
    assert rec.rho_min == F32(np.inf) and rec.rho_max == F32(-np.inf) and rec.v2_max == F32(-np.inf)
    assert rec.cell_rho_min is rec.cell_rho_max is rec.cell_v2_max is None and rec.first_bad == (1, 1, 1, 64)
    assert rec.sum_rho == 0.0 and rec.sum_rho_v2 == 0.0 and math.isnan(rec.rho_mean) and math.isnan(rec.speed_max)
    assert mon.host_monitor(g.rho, g.vel, g.obstacle, g.active_block_coords, n_owned=0) == mon.Record()
    g.obstacle[...] = True
    assert mon.host_monitor(g.rho, g.vel, g.obstacle, g.active_block_coords) == mon.Record()


def test_only_owned_blocks_are_read():
    g = _level((3, 1, 1), 6)
    g.rho[:, :, :, 2] = np.nan
    rec = mon.host_monitor(g.rho, g.vel, g.obstacle, g.active_block_coords, n_owned=2)
    _same(rec, brute(g.rho[:, :, :, :2], g.vel[:, :, :, :2], g.obstacle[:, :, :, :2], g.active_block_coords[:2]))
    assert rec.n_bad == 0 and rec.n_fluid == 1024


@pytest.mark.parametrize("n", [1, 3, 512, 513, 1025])
def test_tree_sum_equals_the_halving_definition(n):
    rng = np.random.default_rng(n)
    x = rng.random(n) * 10.0 ** rng.integers(-8, 8, n)
    assert mon.tree_sum(x) == _halving(x)
    # chunks of 512 first, then the chunk results: the same tree, so the same bits (what the device does)
    chunks = [mon.tree_sum(x[i:i + 512]) for i in range(0, n, 512)]
    assert mon.tree_sum(np.array(chunks)) == _halving(x)
    if n > 3:
        assert mon.tree_sum(x) != float(np.cumsum(x)[-1]) or n < 8          # an order of its own, not the sequential one
    # through host_monitor: n blocks of constant rho_b, so the per-block results are 512 rho_b exactly
    rho = np.zeros((8, 8, 8, n), F32, order="F")
    rho[...] = (rng.integers(1, 1 << 20, n).astype(F32) / F32(1 << 10))[None, None, None, :]
    vel = np.zeros((8, 8, 8, n, 3), F32, order="F")
    coords = [(b + 1, 1, 1) for b in range(n)]
    rec = mon.host_monitor(rho, vel, np.zeros(rho.shape, bool), coords)
    assert rec.sum_rho == _halving(512.0 * rho[0, 0, 0, :].astype(F64)) and rec.sum_rho_v2 == 0.0


def test_merge_of_rank_records():
    g = _level((4, 2, 1), 11)
    g.rho[...] = F32(1.0)                                           # every cell ties for both extremes of rho
    g.vel[2, 2, 2, 5, :] = np.nan                                   # a bad cell on one rank only
    whole = mon.host_monitor(g.rho, g.vel, g.obstacle, g.active_block_coords)
    # rank 0 holds blocks 4..7 (the HIGHER coordinates), rank 1 blocks 0..3: rank order and coordinate order disagree
    parts = []
    for sel in (np.arange(4, 8), np.arange(0, 4)):
        parts.append(mon.host_monitor(g.rho[:, :, :, sel], g.vel[:, :, :, sel], g.obstacle[:, :, :, sel],
                                      [g.active_block_coords[b] for b in sel]))
    assert parts[0].n_bad == 1 and parts[1].n_bad == 0
    merged = mon.merge([parts[0], None, parts[1]])
    assert merged.same_but_sums(whole)
    assert merged.cell_rho_min == merged.cell_rho_max == (1, 1, 1, 0) and merged.first_bad == tuple(g.active_block_coords[5]) + (146,)
    assert merged.sum_rho == parts[0].sum_rho + parts[1].sum_rho and merged.sum_rho_v2 == parts[0].sum_rho_v2 + parts[1].sum_rho_v2
    assert mon.merge([]) == mon.Record() and mon.merge([None, parts[1]]) == parts[1]
    # a strictly better value on the later rank wins whatever its cell
    a, b = mon.Record(**vars(parts[0])), mon.Record(**vars(parts[1]))
    b.rho_max, b.cell_rho_max = F32(1.5), (9, 9, 9, 511)
    assert mon.merge([a, b]).cell_rho_max == (9, 9, 9, 511) and mon.merge([b, a]).rho_max == F32(1.5)


def test_cell_coordinates_agree_with_the_flow_file_and_the_probes():
    grids, _ = cases.tunnel_with_sphere(levels=2, wall_model=True)
    offset = np.array([3.25, -1.5, 0.75])
    for lvl, g in enumerate(grids):
        g.dx = 1.0 / (1 << lvl)
    for lvl, b, c in ((0, 5, 0), (0, 17, 511), (1, 3, 8 + 64 * 2 + 5)):
        g = grids[lvl]
        cell = tuple(g.active_block_coords[b]) + (c,)
        xyz = np.array(mon.cell_coordinates(cell, g.dx, offset))
        # the flow file: the voxel's eight corner points (float32) average to the centre
        geo = out_mod._flow_geometry(grids, [(lvl, b)])
        corners = geo["points"][geo["connectivity"][8 * c: 8 * c + 8]].astype(F64)
        assert np.abs(corners.mean(axis=0) - (xyz + offset)).max() <= 1e-6 * np.abs(corners).max()      # float32 points
        # the probes' frame: a probe at these coordinates has this cell as its base cell, with zero weights
        plan = pm.plan_probes(xyz[None, :], grids, offset)
        assert int(plan.level[0]) == lvl and int(plan.blocks[0, 0]) == b and int(plan.cells[0, 0]) == c
        assert np.array_equal(plan.weights[0], np.zeros(3, F32))
    assert mon.cell_coordinates((1, 1, 1, 0), 0.5) == (0.25, 0.25, 0.25)
    assert mon.cell_coordinates((2, 1, 3, 1 + 8 * 2 + 64 * 3), 2.0, (1.0, 1.0, 1.0)) == (18.0, 4.0, 38.0)


def test_yaml_keys_and_refusals():
    for name in ("ball1m", "bunny", "cube1m", "wing5deg"):                  # stability_check: true everywhere, read by nobody
        cfg = pp.load_case_configuration(os.path.join(G, f"{name}_config.yaml"))
        assert not cfg.flow_monitor_enabled and not cfg.flow_monitor_stop_on_divergence
    cfg = pp.load_case_configuration(BALL, {"advanced": {"flow_monitor": {"enabled": True}}})
    assert cfg.flow_monitor_enabled and not cfg.flow_monitor_stop_on_divergence
    cfg = pp.load_case_configuration(BALL, {"advanced": {"flow_monitor": {"enabled": True, "stop_on_divergence": True}}})
    assert cfg.flow_monitor_enabled and cfg.flow_monitor_stop_on_divergence
    cfg = pp.load_case_configuration(BALL, {"advanced": {"flow_monitor": {}}})
    assert not cfg.flow_monitor_enabled
    for bad, word in (([True], "mapping"), ("yes", "mapping"), ({"enabled": "yes"}, "enabled"), ({"enabled": 1}, "enabled"),
                      ({"enabled": True, "stop_on_divergence": "no"}, "stop_on_divergence")):
        with pytest.raises(ValueError, match=word):
            pp.load_case_configuration(BALL, {"advanced": {"flow_monitor": bad}})


def test_csv_text():
    assert mon.CSV_HEADER == ("Step,StateStep,Level,FluidCells,NonFiniteCells,RhoMin,RhoMax,RhoMean,SpeedMax,Mach,KineticEnergy,"
                              "RhoMinX,RhoMinY,RhoMinZ,RhoMaxX,RhoMaxY,RhoMaxZ,SpeedMaxX,SpeedMaxY,SpeedMaxZ,"
                              "FirstNonFiniteX,FirstNonFiniteY,FirstNonFiniteZ")
    rec = mon.Record(1024, 0, F32(0.998), F32(1.25), F32(0.0625), (1, 1, 1, 0), (2, 1, 1, 9), (1, 2, 1, 511), None, F64(1024.5), F64(3.0))
    row = mon.csv_row(500, 503, 2, rec, 0.5, (1.0, 0.0, -1.0))
    assert row == ("500,503,2,1024,0,0.998,1.25,1.00048828125,0.25,0.4330127018922193,1.5,"
                   "-0.75,0.25,1.25,3.75,0.75,1.25,2.75,7.75,4.75,,,")
    assert len(row.split(",")) == len(mon.CSV_HEADER.split(","))
    # the RhoMin text is convergence.csv's
    assert row.split(",")[5] == out_mod.convergence_csv_row(500, 1.0, 1.0, 0.05, F32(0.998), 1.0, None, None).split(",")[4]
    empty = mon.csv_row(7, 7, 1, mon.Record(n_fluid=3, n_bad=3, first_bad=(1, 1, 1, 2)), 1.0)
    assert empty == "7,7,1,3,3,inf,-inf,nan,nan,nan,0.0," + ",,," * 3 + "2.5,0.5,0.5"


def test_warning_texts():
    healthy = mon.Record(512, 0, F32(0.99), F32(1.01), F32(0.01), (1, 1, 1, 0), (1, 1, 1, 1), (1, 1, 1, 2), None, F64(512.0), F64(1.0))
    assert mon.warnings_of(healthy, 100, 1) == []
    at_threshold = mon.Record(**{**vars(healthy), "v2_max": np.nextafter(F32(0.09), F32(0)), "rho_min": F32(0.5), "rho_max": F32(1.5)})
    assert mon.warnings_of(at_threshold, 1, 1) == []                # strict comparisons: 0.5 and 1.5 are exact, the speed is just below 0.3
    over = mon.Record(**{**vars(at_threshold), "v2_max": F32(0.09)})             # float32 0.09 lies above 0.09
    assert mon.warnings_of(over, 1, 1)[1:] == ["  - High velocity: 0.3000 (Ma > 0.5)"]
    sick = mon.Record(512, 2, F32(0.25), F32(1.75), F32(0.25), (1, 1, 1, 0), (1, 1, 1, 1), (1, 1, 1, 2), (2, 1, 1, 9), F64(510.0), F64(1.0))
    got = mon.warnings_of(sick, 1500, 3, 0.5, (1.0, 1.0, 1.0))
    assert got == ["[WARNING] Step 1500 level 3 stability issues:", "  - High velocity: 0.5000 (Ma > 0.5)", "  - Low density: 0.2500",
                   "  - High density: 1.7500",
                   "  - Non-finite cells: 2, the first in block (2, 1, 1) cell (1, 1, 0) at (3.75, -0.25, -0.75)"]
    err = mon.FlowDiverged(1500, 3, (2, 1, 1, 9), (3.75, -0.25, -0.75), 2)
    assert isinstance(err, RuntimeError) and (err.step, err.level, err.cell, err.coordinates) == (1500, 3, (2, 1, 1, 9), (3.75, -0.25, -0.75))
    assert "level 3" in str(err) and "(2, 1, 1)" in str(err)
    all_bad = mon.Record(n_fluid=4, n_bad=4, first_bad=(1, 1, 1, 0))
    assert len(mon.warnings_of(all_bad, 1, 1)) == 2


# ---- run_case with the CPU oracle: the host fallback (a stepper without monitor()) ----
CUBE = {"basic": {"num_levels": 1, "surface_resolution": 7, "simulation": {"steps": 10, "output_freq": 8}},
        "advanced": {"boundary": {"method": "bounce_back"}, "high_re": {"wall_model": {"enabled": False}},
                     "numerics": {"c_wale": 0.0, "nu_sgs_background": 0.0}, "diagnostics": {"freq": 4}}}


def test_run_case_with_the_oracle_writes_rows_from_downloaded_fields_and_leaves_the_rest_unchanged(tmp_path):
    import filecmp
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _steppers import OracleStepper
    from open_ludwig_amd import case
    from open_ludwig_amd.statistics import t_sub_after
    from oracle import oracle
    oracle.set_num_threads(min(8, os.cpu_count() or 1))
    runs, logs = {}, []
    for on in (False, True):
        cfg = pp.load_case_configuration(os.path.join(G, "cube1m_config.yaml"), {**CUBE, "advanced": {**CUBE["advanced"], "flow_monitor": {"enabled": on}}})
        setup = pp.setup_multilevel_domain(cfg, os.path.join(G, "cube1m.stl"))
        holder = {}

        def factory(grids):
            holder["st"] = OracleStepper(grids)
            return holder["st"]
        out = os.path.join(tmp_path, "on" if on else "off")
        case.run_case(cfg, factory, setup=setup, out_dir=out, log=logs.append)
        runs[on] = (out, setup, holder["st"])
    off, on = runs[False][0], runs[True][0]
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + ["flow_monitor.csv"])
    for name in os.listdir(off):
        if name != "convergence.csv":                                       # wall time and MLUPS columns
            assert filecmp.cmp(os.path.join(off, name), os.path.join(on, name), shallow=False), name
    lines = open(os.path.join(on, "flow_monitor.csv")).read().splitlines()
    conv = [l.split(",") for l in open(os.path.join(on, "convergence.csv")).read().splitlines()[1:]]
    # async_depth 8: batches end at 8 and 10; the diagnostics step is 8 (state 8); the last step, 10, is none and gets a record of its own
    assert lines[0] == mon.CSV_HEADER and [l.split(",")[:3] for l in lines[1:]] == [["8", "8", "1"], ["10", "10", "1"]]
    assert [c[0] for c in conv] == ["8"] and lines[1].split(",")[5] == conv[0][4]      # level 1's RhoMin is convergence.csv's rho_min
    (grids, _, params, _), st = runs[True][1], runs[True][2]
    g = grids[0]
    rec = mon.host_monitor(st.field(0, "rho"), st.field(0, "vel_temp" if t_sub_after(0, 10) % 2 == 0 else "vel"), g.obstacle, g.active_block_coords)
    assert lines[2] == mon.csv_row(10, 10, g.level_id, rec, g.dx, params.mesh_offset) and rec.n_bad == 0 and rec.n_fluid == int((~g.obstacle).sum())
