"""The state machine around the record step (ludwig_hip.hip: f_valid, rec_valid, rho_in_rec, rec_eligible, rec_banned, rec_hold).

While a plain level steps by 11-float records its f, f_temp, vel, vel_temp and rho are stale, and every entry point that reads, writes or
hands them out has to bring them back first. Here every such entry point (tests/_record_state_cases.py lists them) is the FIRST call
that touches a level after record steps, and what it returns - or what the next steps make of what it wrote - is compared bit for bit
with the f path of the same binary (LUDWIG_RECORD_STEP=0, read per step call, proven equal to the oracle elsewhere) and with the CPU
oracle. tests/test_record_state_host.py shows on the CPU that the states used here differ between steps n and n - 2 almost everywhere,
so a reader of stale arrays cannot pass; the first-reader tests assert it again on the device outputs themselves.

One 32^3 (4,4,4) or 40 x 16 x 24 (5,2,3) periodic box per test, at most a handful of steps."""
import ctypes as C

import numpy as np
import pytest

import _edge_states as es
import _halo_ref as href
import _observer_sets as obs
from open_ludwig_amd import _lib, adapt, cases, execute_timestep_batch, order as order_mod, physics, streamlines as st, warm_start as ws
from oracle import oracle

pytestmark = pytest.mark.gpu
F32 = np.float32
STATE = ("f", "f_temp", "vel", "vel_temp", "rho")
NB, NB2 = (4, 4, 4), (5, 2, 3)
SEED, OTHER_SEED = 5, 9
SWITCH = "LUDWIG_RECORD_STEP"


def box(nb=NB, seed=SEED):
    grids, params = cases.periodic_box(nb)
    cases.init_perturbed(grids[0], seed)
    return grids, params


def snapshot(g):
    out = {name: getattr(g, name).copy() for name in STATE}
    for a in out.values():
        a.setflags(write=False)
    return out


_oracle = {}


def oracle_states(nb, upto=8):
    """the oracle's five state arrays after 0 .. upto steps of the perturbed box: computed once per box, never changed afterwards"""
    if nb not in _oracle:
        grids, params = box(nb)
        out = [snapshot(grids[0])]
        for t in range(1, upto + 1):
            oracle.execute_timestep_batch(grids, t, 1, F32(0.0), params)
            out.append(snapshot(grids[0]))
        _oracle[nb] = out
    return _oracle[nb]


def newest(state, t):
    """rho and the newest velocity of a five-array state after t steps"""
    return {"rho": state["rho"], "vel": state[obs.newest_vel(t)]}


def step(mp, dev, t0, n, params, records, **observers):
    """n steps from coarse step t0 on: by records where the rule allows it, or on the f path of the same binary"""
    if records:
        mp.delenv(SWITCH, raising=False)
    else:
        mp.setenv(SWITCH, "0")
    try:
        execute_timestep_batch(dev if isinstance(dev, list) else [dev], t0, n, F32(0.0), params, **observers)
    finally:
        mp.delenv(SWITCH, raising=False)


def same(got, want, what):
    assert len(got) == len(want) > 0, what
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}, output {i}: {a.dtype} {a.shape} against {b.dtype} {b.shape}"
        if a.dtype.kind == "f":
            es.assert_nan_aware_equal(a, b, f"{what}, output {i}")
        else:
            assert np.array_equal(a, b), f"{what}, output {i}"


def differ(a, b):
    return len(a) != len(b) or any(np.asarray(x).shape != np.asarray(y).shape or not np.array_equal(x, y, equal_nan=np.asarray(x).dtype.kind == "f")
                                   for x, y in zip(a, b))


def assert_state(dev, want, what):
    for name in STATE:
        es.assert_nan_aware_equal(dev.download(name), want[name], f"{what}: {name}")


class Levels:
    """device levels that are closed together, whatever the test does"""

    def __init__(self):
        self.open = []

    def add(self, x):
        self.open.append(x)
        return x

    def adapt(self, g):
        return self.add(adapt(g, 0))

    def close(self):
        for x in reversed(self.open):
            x.close()


@pytest.fixture
def levels(gpu):
    L = Levels()
    yield L
    L.close()


# ---- a. first reader -------------------------------------------------------------------------------------------------------------
DOWNLOADS = tuple("download_" + name for name in STATE)
FIRST_READERS = obs.KINDS + tuple(k for k in obs.LEVEL_KINDS if k not in obs.BANNING_KINDS) + DOWNLOADS
# what reads the buffers of parity 1 whatever the step: after one step nothing has written there yet, so no staleness can show
READS_PARITY_ONE = ("download_f_temp", "download_vel_temp", "gradient_vel_temp")


def reader(kind, grids, dev, t, state, levels):
    """(make, sample) of one reader kind on `dev`, reading the state after coarse step t"""
    if kind in DOWNLOADS:
        return obs.Nothing, lambda _: [dev.download(kind[len("download_"):])]
    if kind in obs.KINDS:
        return obs.makers(grids, dev, t)[kind]
    target = levels.adapt(grids[0]) if kind == "warm_start" else None
    return obs.level_makers(grids, dev, t, state, target)[kind]


def read(kind, grids, dev, t, state, levels):
    make, sample = reader(kind, grids, dev, t, state, levels)
    S = make()
    try:
        return sample(S)
    finally:
        S.close()


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("kind", FIRST_READERS)
def test_first_reader(levels, monkeypatch, kind, n):
    """n = 1: one parity in records, with rho in it; 2: both parities in records; 3: both, the other one newest"""
    grids, params = box()
    want = oracle_states(NB)
    rec, twin, old = levels.adapt(grids[0]), levels.adapt(grids[0]), levels.adapt(grids[0])
    m = max(n - 2, 0)
    step(monkeypatch, rec, 1, n, params, True)
    step(monkeypatch, twin, 1, n, params, False)
    step(monkeypatch, old, 1, max(m, 1), params, False)
    if m == 0:                                                              # the content at upload, on a level that has stepped (the subgrid
        for name in STATE:                                                  # readers want the constants of a step)
            old.upload(name, getattr(grids[0], name))
    assert (rec.record_steps(), twin.record_steps(), old.record_steps()) == (n, 0, 0)
    state = newest(want[n], n)
    # the twin's output, and what the same call returns from the content the same buffers had two steps earlier (or at upload)
    out_twin = read(kind, grids, twin, n, state, levels)
    out_old = read(kind, grids, old, n, state, levels)
    out_rec = read(kind, grids, rec, n, state, levels)                    # the first call that touches the level after its record steps
    same(out_rec, out_twin, f"{kind} after {n} record steps against the f path")
    if kind in DOWNLOADS:
        same(out_rec, [want[n][kind[len("download_"):]]], f"{kind} after {n} record steps against the oracle")
    if kind not in obs.CONSTANT_ON_A_PLAIN_LEVEL and not (n == 1 and kind in READS_PARITY_ONE):
        assert differ(out_twin, out_old), f"{kind}: the state after {n} steps and the one after {m} give the same output, so the comparison shows nothing"
    step(monkeypatch, rec, n + 1, 2, params, True)
    step(monkeypatch, twin, n + 1, 2, params, False)
    assert (rec.record_steps(), twin.record_steps()) == (n + 2, 0), "a reader neither bans the record step nor invalidates the records"
    assert_state(rec, want[n + 2], f"{kind} after {n} record steps, two steps on")
    assert_state(twin, want[n + 2], f"{kind} after {n} f-path steps, two steps on")


def test_both_step_entry_points_step_by_records(levels, monkeypatch):
    """ludwig_step and ludwig_stream_collide of a whole level without a parent, call by call"""
    grids, params = box(NB2)
    want = oracle_states(NB2)
    rec = levels.adapt(grids[0])
    monkeypatch.delenv(SWITCH, raising=False)
    for t in (1, 2, 3, 4):
        if t % 2:
            physics.perform_timestep_v2(rec, None, F32(0.5), F32(0.0), params, t, F32(0.0))
        else:
            physics.stream_collide(rec, None, F32(0.5), F32(0.0), params, t, part=_lib.PART_ALL)
    assert rec.record_steps() == 4
    assert_state(rec, want[4], "four steps through ludwig_step and ludwig_stream_collide")


# ---- b. writers ------------------------------------------------------------------------------------------------------------------
UPLOADS = tuple("upload_" + name for name in STATE)
WRITERS = UPLOADS + ("halo_unpack", "init_equilibrium", "init_from_source", "field_ptr", "rho_store")


def halo_unpack(dev, field, index, words):
    """ludwig_halo_unpack (k_scatter) of `words` into the elements `index` of `field`"""
    import torch
    idx = torch.as_tensor(np.ascontiguousarray(index, dtype=np.int64), device="cuda:0")
    src = torch.as_tensor(np.ascontiguousarray(words).view(np.float32), device="cuda:0")
    torch.cuda.synchronize()
    _lib.check(_lib.load().ludwig_halo_unpack(dev.handle, _lib.FIELD_NAMES[field], C.c_void_p(idx.data_ptr()), idx.numel(), C.c_void_p(src.data_ptr()),
                                              None))
    dev.synchronize()


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("op", WRITERS)
def test_writer(levels, monkeypatch, op, n):
    """the write is the first call after n record steps; two further steps show what the level made of it"""
    grids, params = box(NB2)
    (other,), _ = box(NB2, OTHER_SEED)
    g = grids[0]
    rec, twin = levels.adapt(g), levels.adapt(g)
    step(monkeypatch, rec, 1, n, params, True)
    step(monkeypatch, twin, 1, n, params, False)
    oracle.execute_timestep_batch(grids, 1, n, F32(0.0), params)
    assert rec.record_steps() == n
    against_oracle, expected = True, n + 2
    if op in UPLOADS:
        name = op[len("upload_"):]
        getattr(g, name)[...] = getattr(other, name)
        for dev in (rec, twin):
            dev.upload(name, getattr(g, name))
    elif op == "halo_unpack":
        name = "f_temp" if n % 2 == 0 else "f"                            # the next step's input
        index = obs.self_plan_lists(g.n_blocks)[1]["f"]
        words = href.bits(getattr(other, name))[index]
        getattr(g, name)[...] = href.as_field(href.unpack(href.bits(getattr(g, name)), index, words), g.n_blocks, 27)
        for dev in (rec, twin):
            halo_unpack(dev, name, index, words)
    elif op == "init_equilibrium":
        oracle.init_equilibrium(g)
        for dev in (rec, twin):
            dev.init_equilibrium()
    elif op == "init_from_source":
        against_oracle = False
        src = levels.add(ws.DeviceFlowSource(st.host_levels([other], lambda li: (other.rho, other.vel))))
        counts = [dev.init_from_source(src, (1.0, 1.0, 1.0, 0.5, 0.25, 0.0), 1.0, (1.0, 0.0, 0.0, 0.0)) for dev in (rec, twin)]
        assert np.array_equal(counts[0], counts[1]) and counts[0][0] > 0
    elif op == "field_ptr":
        expected = n                                                       # a raw pointer is out: the f path for good
        for dev in (rec, twin):
            assert dev.field_ptr("vel")[0]
    else:
        for dev in (rec, twin):
            dev.set_rho_store(True)
            dev.set_rho_store(False)
    step(monkeypatch, rec, n + 1, 2, params, True)
    step(monkeypatch, twin, n + 1, 2, params, False)
    assert (rec.record_steps(), twin.record_steps()) == (expected, 0)
    got = {name: rec.download(name) for name in STATE}
    for name in STATE:
        es.assert_nan_aware_equal(got[name], twin.download(name), f"{op} after {n} record steps, two steps on, against the f path: {name}")
    if against_oracle:
        oracle.execute_timestep_batch(grids, n + 1, 2, F32(0.0), params)
        for name in STATE:
            es.assert_nan_aware_equal(got[name], getattr(g, name), f"{op} after {n} record steps, two steps on, against the oracle: {name}")


# ---- c. eligibility through geometry ---------------------------------------------------------------------------------------------
GEOMETRY = {"obstacle": (True, False), "sponge": (F32(0.25), F32(0.0)), "wall_dist": (F32(2.0), F32(100.0))}


@pytest.mark.parametrize("field", list(GEOMETRY))
def test_geometry_upload_changes_the_path_and_back(levels, monkeypatch, field):
    """one special cell uploaded after two record steps: the f path; the field cleared again: records again. The oracle's level gets the
    same cell (a wall distance changes nothing while the wall model is off, but such a level is not a plain one)."""
    grids, params = box(NB2)
    g = grids[0]
    rec = levels.adapt(g)
    on, off = GEOMETRY[field]
    t, by_records = 0, 0
    for value, records in ((None, True), (on, False), (off, True)):
        if value is not None:
            getattr(g, field)[3, 4, 5, 7] = value
            rec.upload(field, getattr(g, field))
        step(monkeypatch, rec, t + 1, 2, params, True)
        oracle.execute_timestep_batch(grids, t + 1, 2, F32(0.0), params)
        t += 2
        by_records += 2 if records else 0
        assert rec.record_steps() == by_records, f"{field} = {value}: after {t} steps"
        assert_state(rec, {name: getattr(g, name) for name in STATE}, f"{field} = {value}, after {t} steps")


# ---- d. bans ---------------------------------------------------------------------------------------------------------------------
def nest():
    """a 24^3 periodic box with its middle block refined: level 1 is a plain level until level 2 reads it"""
    grids, params = cases.periodic_box((3, 3, 3))
    cases.init_perturbed(grids[0], SEED)
    tau_child = 0.5 + (float(grids[0].tau) - 0.5) / 2.0
    child = cases.refine_region(grids[0], (2, 2, 2), (2, 2, 2), tau_child, temporal=False)
    cases.init_perturbed(child, SEED + 1)
    return grids + [child], params


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_a_level_that_becomes_a_parent_is_banned(levels, monkeypatch, native):
    """native: the batch of two levels holds both on the f path from its first step. python: level 1's step of coarse step 3 is one more
    record step (ludwig_step without a parent, outside any batch), and level 2's step right after it is the first reader"""
    grids, params = nest()
    dev = [levels.adapt(g) for g in grids]
    monkeypatch.delenv(SWITCH, raising=False)
    execute_timestep_batch(dev[:1], 1, 2, F32(0.0), params)
    oracle.execute_timestep_batch(grids[:1], 1, 2, F32(0.0), params)
    assert dev[0].record_steps() == 2
    execute_timestep_batch(dev, 3, 2, F32(0.0), params, native=native)      # the first thing that reads level 1 is level 2's interface pass
    oracle.execute_timestep_batch(grids, 3, 2, F32(0.0), params)
    banned_at = 2 if native else 3
    assert (dev[0].record_steps(), dev[1].record_steps()) == (banned_at, 0)
    assert_state(dev[0], {name: getattr(grids[0], name) for name in STATE}, "level 1 after the nest's steps")
    for name in ("f", "vel", "rho"):                                        # level 2's newest state
        es.assert_nan_aware_equal(dev[1].download(name), getattr(grids[1], name), f"level 2 after the nest's steps: {name}")
    execute_timestep_batch(dev[:1], 5, 1, F32(0.0), params)
    oracle.execute_timestep_batch(grids[:1], 5, 1, F32(0.0), params)
    assert dev[0].record_steps() == banned_at, "a level another level has read stays on the f path"
    assert_state(dev[0], {name: getattr(grids[0], name) for name in STATE}, "level 1 alone afterwards")


def test_halo_plan_made_mid_run(levels, monkeypatch):
    """ludwig_halo_plan_create after two record steps: the plan packs the current state, the level stays on the f path, and what an unpack
    writes is seen by the next step"""
    grids, params = box(NB2)
    (other,), _ = box(NB2, OTHER_SEED)
    g = grids[0]
    rec = levels.adapt(g)
    step(monkeypatch, rec, 1, 2, params, True)
    oracle.execute_timestep_batch(grids, 1, 2, F32(0.0), params)
    assert rec.record_steps() == 2
    send, recv = obs.self_plan_lists(g.n_blocks)
    plan = levels.add(obs.self_plan(rec, send, recv))                       # the first call after the record steps
    fields = {"f": "f_temp", "vel": "vel_temp", "rho": "rho"}               # the newest state after step 2 = the input of step 3
    for group, name in fields.items():
        _lib.check(plan.pack(group, name))
        sent = plan.read_send(group)
        want = href.pack(href.bits(getattr(g, name)), send[group])
        assert np.array_equal(sent, want), f"{group} / {name}: {href.first_difference(sent, want)}"
    for group, name in fields.items():
        K = obs.iw.GROUP_COMPONENTS[group]
        words = href.bits(getattr(other, name))[recv[group]]
        plan.write_recv(group, words)
        _lib.check(plan.unpack(group, name))
        getattr(g, name)[...] = href.as_field(href.unpack(href.bits(getattr(g, name)), recv[group], words), g.n_blocks, K)
    step(monkeypatch, rec, 3, 2, params, True)
    oracle.execute_timestep_batch(grids, 3, 2, F32(0.0), params)
    assert rec.record_steps() == 2, "a level with a halo plan stays on the f path"
    assert_state(rec, {name: getattr(g, name) for name in STATE}, "two steps after the unpack")


# ---- e. observed batches ---------------------------------------------------------------------------------------------------------
IN_BATCH = {"probes": "probes", "surface_stats": "surface", "force_series": "forces", "tracers": "tracers", "flux_planes": "fluxes", "modes": "modes"}
OLD_ENTRY = ("probes", "surface_stats", "force_series", "tracers")
HOWS = [(k, h) for k in IN_BATCH for h in ("native", "python")] + [(k, "old_entry") for k in OLD_ENTRY]


def collected(kind, S, t):
    """what a set holds after its batches"""
    if kind == "modes":
        return [x for col in (0, 1) for x in (S.download(0, col)[0], np.array([S.download(0, col)[1]]))]
    if kind == "tracers":
        S.snapshot(t)
    out = S.download()
    return [np.asarray(x) for x in (out if isinstance(out, (tuple, list)) else (out,))]


def old_entry_batch(kind, dev, S, t0, n, params):
    """the entry points from before the observer list, each with its own argument list"""
    lib, fl = _lib.load(), params.to_c()
    head = ((C.c_void_p * 1)(dev.handle), 1, t0, n, 0.0, C.byref(fl))
    h, sched = S.handle, (S.start_step, S.interval)
    if kind == "probes":
        rc = lib.ludwig_execute_timestep_batch_probes(*head, h, *sched)
    elif kind == "surface_stats":
        rc = lib.ludwig_execute_timestep_batch_sampled(*head, C.byref(_lib.BatchSamplers(None, 0, 1, h.value, *sched)))
    elif kind == "force_series":
        rc = lib.ludwig_execute_timestep_batch_loads(*head, None, h, *sched)
    else:
        rc = lib.ludwig_execute_timestep_batch_tracers(*head, None, None, 0, 1, h, *sched)
    _lib.check(rc)


@pytest.mark.parametrize("kind,how", HOWS, ids=[f"{k}-{h}" for k, h in HOWS])
def test_observed_batch(levels, monkeypatch, kind, how):
    """a record batch, an observed batch, a record batch. native / old_entry: the observed batch holds the level on the f path; python:
    every step is a record step and every sample brings the arrays back."""
    grids, params = box()
    want = oracle_states(NB)
    got = {}
    for path in ("records", "f"):
        records = path == "records"
        dev = levels.adapt(grids[0])
        S = levels.add(obs.batch_set(kind, grids, dev, 3))
        step(monkeypatch, dev, 1, 2, params, records)
        if how == "old_entry":
            if not records:
                monkeypatch.setenv(SWITCH, "0")
            old_entry_batch(kind, dev, S, 3, 3, params)
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            step(monkeypatch, dev, 3, 3, params, records, native=how == "native", **{IN_BATCH[kind]: S})
        assert dev.record_steps() == ((5 if how == "python" else 2) if records else 0)
        series = collected(kind, S, 5)
        step(monkeypatch, dev, 6, 1, params, records)
        assert dev.record_steps() == ((6 if how == "python" else 3) if records else 0)
        got[path] = (series, {name: dev.download(name) for name in STATE})
    same(got["records"][0], got["f"][0], f"{kind} series, {how}")
    for name in STATE:
        es.assert_nan_aware_equal(got["records"][1][name], got["f"][1][name], f"{kind}, {how}: {name} against the f path")
        es.assert_nan_aware_equal(got["records"][1][name], want[6][name], f"{kind}, {how}: {name} against the oracle")


# the cases tests/_record_state_cases.py may name (tests/test_record_state_host.py checks that it names no other)
PARAMETERS = {"test_first_reader": FIRST_READERS, "test_writer": WRITERS, "test_geometry_upload_changes_the_path_and_back": tuple(GEOMETRY),
              "test_a_level_that_becomes_a_parent_is_banned": ("native", "python"), "test_observed_batch": tuple(f"{k}-{h}" for k, h in HOWS),
              "test_seeded_walk": tuple(str(s) for s in range(5))}


# ---- f. seeded walks -------------------------------------------------------------------------------------------------------------
WALK_OPS = ("step", "two_steps", "download", "reader", "upload", "rho_store", "set_order", "observed_batch")
WALK_READERS = tuple(k for k in FIRST_READERS if k not in DOWNLOADS)


def walk_plan(seed, n_ops=12):
    """the operations of one walk with their arguments, drawn up front so that a failure can print them"""
    rng = np.random.default_rng(1000 + seed)
    plan = []
    for _ in range(n_ops):
        op = WALK_OPS[int(rng.integers(len(WALK_OPS)))]
        arg = {"download": lambda: STATE[int(rng.integers(5))], "reader": lambda: WALK_READERS[int(rng.integers(len(WALK_READERS)))],
               "upload": lambda: STATE[int(rng.integers(5))], "rho_store": lambda: bool(rng.integers(2)), "set_order": lambda: int(rng.integers(2)),
               "observed_batch": lambda: list(IN_BATCH)[int(rng.integers(len(IN_BATCH)))]}.get(op, lambda: None)()
        plan.append((op, arg))
    return plan


@pytest.mark.parametrize("seed", range(5))
def test_seeded_walk(levels, monkeypatch, seed):
    """one step, then twelve operations, each first on the f-path twin and then on the record level: every output on the way and the state at the end"""
    grids, params = box()
    (other,), _ = box(NB, OTHER_SEED)
    g = grids[0]
    coords = np.asarray(g.active_block_coords)
    orders = (order_mod.build("block_planes", coords), order_mod.build("run_per_xcd", coords))
    plan = walk_plan(seed)
    twin, rec = levels.adapt(g), levels.adapt(g)
    step(monkeypatch, twin, 1, 1, params, False)                            # every walk starts one step in
    step(monkeypatch, rec, 1, 1, params, True)
    t = 1
    log = []
    try:
        for op, arg in plan:
            log.append((t, op, arg))
            state = newest({name: twin.download(name) for name in ("rho", "vel", "vel_temp")}, t) if op == "reader" else None
            outs = []
            for dev, records in ((twin, False), (rec, True)):
                out = []
                if op in ("step", "two_steps"):
                    step(monkeypatch, dev, t + 1, 1 if op == "step" else 2, params, records)
                elif op == "download":
                    out = [dev.download(arg)]
                elif op == "reader":
                    out = read(arg, grids, dev, t, state, levels)
                elif op == "upload":
                    dev.upload(arg, getattr(other, arg))
                elif op == "rho_store":
                    dev.set_rho_store(arg)
                elif op == "set_order":
                    dev.set_order(orders[arg])
                else:
                    S = levels.add(obs.batch_set(arg, grids, dev, t + 1))
                    step(monkeypatch, dev, t + 1, 2, params, records, **{IN_BATCH[arg]: S})
                    out = collected(arg, S, t + 2)
                outs.append(out)
            t += {"step": 1, "two_steps": 2, "observed_batch": 2}.get(op, 0)
            if outs[0] or outs[1]:
                same(outs[1], outs[0], f"operation {len(log)}: {op} {arg} at step {t}")
        for name in STATE:
            es.assert_nan_aware_equal(rec.download(name), twin.download(name), f"after the walk: {name}")
        assert twin.record_steps() == 0 and rec.record_steps() > 0
    except AssertionError as e:
        raise AssertionError(f"walk {seed}, operations (step, operation, argument) so far: {log}\n{e}") from e
