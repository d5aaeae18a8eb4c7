"""Force series on the device (ludwig_force_series_*, ludwig_execute_timestep_batch_loads, DeviceForceSeries, HipStepper.force_series_*,
run_case's forces_series.csv). k_force_chunks evaluates the float32 expressions of forces.force_series_contributions with
-ffp-contract=off and k_force_chunks / k_force_combine add their float64 values in the one balanced tree of forces.tree_sum_f64, so every
check against the numpy restatement is bit equality of the nine sums and the coverage count."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from open_ludwig_amd import _lib, adapt, case, cases, execute_timestep_batch, force_series as fs, forces, preprocess as pp, probes as pm
from open_ludwig_amd import surface_stats as ss
from open_ludwig_amd.statistics import sample_steps, t_sub_after

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _probes_common as pcommon  # noqa: E402
import _surface_common as common  # noqa: E402

F32 = np.float32
U = F32(0.05)
STATES = ("f", "f_temp", "rho", "vel", "vel_temp")
SIZES = (1, 2, 511, 512, 513, 1025, 512 * 512 + 1)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(got, want):
    """bit equality of two (sums [9], covered)"""
    return np.array_equal(_bits(got[0]), _bits(want[0])) and int(got[1]) == int(want[1])


# ---- uploaded states, synthetic triangle sets ----
@pytest.fixture(scope="module")
def uploaded(gpu):
    """one tunnel level with random rho / vel / vel_temp uploaded; shared and never stepped; a test that uploads another state puts
    these arrays back"""
    grids, _ = cases.tunnel_with_sphere(levels=1, wall_model=True)
    g = grids[0]
    rng = np.random.default_rng(11)
    fields = {"rho": np.asfortranarray((1.0 + 0.02 * rng.standard_normal(g.rho.shape)).astype(F32)),
              "vel": np.asfortranarray((0.05 * rng.standard_normal(g.vel.shape)).astype(F32)),
              "vel_temp": np.asfortranarray((0.05 * rng.standard_normal(g.vel.shape)).astype(F32))}
    d = adapt(g, 0)
    for k, v in fields.items():
        d.upload(k, v)
    sparams = SimpleNamespace(mesh_offset=np.array([0.3, -0.7, 1.9]), rho_physical=1.225, velocity_scale=40.0, u_physical=2.0,
                              reference_area=10.0, reference_chord=3.0, moment_center=(19.2, 16.0, 16.0), time_scale=0.01)
    yield g, d, fields, sparams
    d.close()


def _synthetic(g, n, seed, missing=True):
    """n triangles on random fluid cells of level g (some without a cell), random normals, areas and centres; the areas span twelve
    decades, so that the float64 sums round and their order shows (float32 terms of one magnitude would add exactly in any order)"""
    rng = np.random.default_rng(seed)
    fluid = np.argwhere(~g.obstacle)                                 # rows x, y, z, block
    pick = fluid[rng.integers(0, len(fluid), n)]
    found = np.ones(n, bool)
    if missing and n > 2:
        found[rng.integers(0, n, max(1, n // 9))] = False
    blocks = np.where(found, pick[:, 3], -1).astype(np.int32)
    cells = np.where(found, pick[:, 0] + 8 * pick[:, 1] + 64 * pick[:, 2], 0).astype(np.int32)
    nrm = rng.standard_normal((n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    plan = ss.SurfacePlan(found, blocks, cells, rng.uniform(0.2, 1.5, n).astype(F32), nrm)
    mesh = SimpleNamespace(centers=rng.uniform(0.0, 40.0, (n, 3)), normals=nrm.astype(np.float64),
                           areas=rng.uniform(0.01, 2.0, n) * 10.0 ** rng.integers(-6, 7, n))
    return plan, mesh


def _device_record(d, g, plan, mesh, sparams, t_sub):
    F = fs.from_mesh(mesh, plan, d, 0, g.tau, sparams, capacity=2)
    try:
        F.sample(t_sub, 5)
        steps, sums, cov = F.download()
        assert steps.tolist() == [5] and sums.shape == (1, 9) and F.download()[0].size == 0      # the ring is empty again
        return sums[0], int(cov[0])
    finally:
        F.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_record_of_uploaded_state_equals_the_restatement(uploaded, n):
    """one chunk, a partial chunk, an odd number of chunks, and 512 * 512 + 1: the smallest n with a second combine launch; the odd
    sub-step reads vel, the even one vel_temp"""
    g, d, fields, sparams = uploaded
    plan, mesh = _synthetic(g, n, n)
    assert plan.found.any()
    for t_sub, vel in ((3, "vel"), (4, "vel_temp")):
        want = fs.host_record(mesh, plan, fields["rho"], fields[vel], g.tau, sparams)
        got = _device_record(d, g, plan, mesh, sparams, t_sub)
        assert _same(got, want), (n, vel, got, want)
        assert np.abs(want[0]).min() > 0 and want[1] == int(plan.found.sum())
        if n >= 511:                                                 # the pairing order shows: a sequential float64 sum gives other bits
            vals = ss.sample_values(plan, fields["rho"], fields[vel], g.tau, sparams)
            seq = np.cumsum(forces.force_series_contributions(mesh, *vals[:4], sparams)[0].astype(np.float64), axis=0)[-1]
            assert (_bits(seq) != _bits(want[0])).sum() >= 5, (n, vel)
    other = fs.host_record(mesh, plan, fields["rho"], fields["vel"], g.tau, sparams)
    assert not _same(other, want)                                    # the buffers do differ


@pytest.mark.gpu
def test_pairing_order_cancellation_and_signed_zeros(uploaded):
    """two huge opposite pressure contributions in different chunks among small ones (any other pairing order rounds differently), a
    column whose every contribution is a signed zero (n_y = 0: -0.0 where p > 0, +0.0 where p < 0), and a set whose every contribution
    to a column is -0.0: the total keeps the sign exactly where the tree appends nothing"""
    g, d, fields, sparams = uploaded
    n = 1536
    plan, mesh = _synthetic(g, n, 77, missing=False)
    a, b = 5, 1029
    for arr in (plan.blocks, plan.cells, plan.wall_dist):
        arr[b] = arr[a]
    plan.normals[:, 1] = 0.0
    plan.normals[a] = (0.8, 0.0, 0.6)
    plan.normals[b] = -plan.normals[a]
    mesh.normals = plan.normals.astype(np.float64)
    mesh.areas[a] = mesh.areas[b] = 3.0e11
    mesh.centers[b] = mesh.centers[a]
    want = fs.host_record(mesh, plan, fields["rho"], fields["vel"], g.tau, sparams)
    vals = ss.sample_values(plan, fields["rho"], fields["vel"], g.tau, sparams)
    contrib, _ = forces.force_series_contributions(mesh, *vals[:4], sparams)
    assert contrib[a, 0] == -contrib[b, 0] and abs(contrib[a, 0]) > 1e4 * np.abs(np.delete(contrib[:, 0], [a, b])).max()
    assert not contrib[:, 1].any() and np.signbit(contrib[:, 1]).any() and not np.signbit(contrib[:, 1]).all()
    seq = np.float64(0.0)
    for v in contrib[:, 0].astype(np.float64):
        seq += v
    assert seq != want[0][0]                                         # a sequential sum is NOT the tree's value here
    got = _device_record(d, g, plan, mesh, sparams, 3)
    assert _same(got, want), (got, want)
    assert want[0][1] == 0.0 and not np.signbit(want[0][1])
    # all -0.0 in column 1: rho > 1 everywhere mapped (p > 0), n_y = 0. n = 1024 = two full chunks: -0.0; n = 1025: +0.0 is appended
    rho_hi = np.asfortranarray(np.abs(fields["rho"] - 1.0) + F32(1.001))
    d.upload("rho", rho_hi)
    try:
        for m, negative in ((2, True), (1024, True), (1025, False), (3, False)):
            sub, msub = plan.subset(np.arange(m)), SimpleNamespace(centers=mesh.centers[:m], normals=mesh.normals[:m], areas=mesh.areas[:m])
            want = fs.host_record(msub, sub, rho_hi, fields["vel"], g.tau, sparams)
            assert want[0][1] == 0.0 and bool(np.signbit(want[0][1])) == negative, m
            got = _device_record(d, g, sub, msub, sparams, 3)
            assert _same(got, want), (m, got, want)
    finally:
        d.upload("rho", fields["rho"])


@pytest.mark.gpu
def test_non_finite_state_shows_in_the_same_columns(uploaded):
    g, d, fields, sparams = uploaded
    n = 700
    plan, mesh = _synthetic(g, n, 5, missing=False)
    rho, vel = fields["rho"].copy(order="F"), fields["vel"].copy(order="F")

    def cell(i):
        c = int(plan.cells[i])
        return c % 8, (c // 8) % 8, c // 64, int(plan.blocks[i])
    seen = {}
    # an Inf velocity alone (u_t is NaN, so the shear is skipped: zeros), a velocity whose square overflows (the pressure columns stay
    # finite, the shear and moment columns do not), then a NaN rho as well (every column)
    for name in ("inf", "overflow", "nan"):
        x, y, z, b = cell(600)
        vel[x, y, z, b, 1] = np.inf if name != "overflow" else F32(1.0e30)
        if name == "nan":
            x, y, z, b = cell(40)
            rho[x, y, z, b] = np.nan
        d.upload("rho", rho)
        d.upload("vel", vel)
        try:
            with np.errstate(all="ignore"):
                want = fs.host_record(mesh, plan, rho, vel, g.tau, sparams)
            got = _device_record(d, g, plan, mesh, sparams, 3)
        finally:
            d.upload("rho", fields["rho"])
            d.upload("vel", fields["vel"])
        assert np.array_equal(np.isfinite(got[0]), np.isfinite(want[0])) and np.array_equal(np.isnan(got[0]), np.isnan(want[0])), name
        assert np.array_equal(got[0], want[0], equal_nan=True) and got[1] == want[1], name
        fin = np.isfinite(want[0])
        assert np.array_equal(_bits(got[0][fin]), _bits(want[0][fin])), name
        seen[name] = fin.copy()
    assert seen["inf"].all()
    assert seen["overflow"][:3].all() and not seen["overflow"][3:].any()
    assert not seen["nan"].any()


@pytest.mark.gpu
def test_an_empty_set_gives_records_of_zeros(uploaded):
    """the named edge case: a rank that owns no triangle"""
    g, d, fields, sparams = uploaded
    plan, mesh = _synthetic(g, 4, 1)
    sub, msub = plan.subset([]), SimpleNamespace(centers=mesh.centers[:0], normals=mesh.normals[:0], areas=mesh.areas[:0])
    got = _device_record(d, g, sub, msub, sparams, 3)
    assert np.array_equal(_bits(got[0]), _bits(np.zeros(9))) and got[1] == 0


# ---- stepped tunnels, sampled inside the batch ----
def _tunnel(levels):
    grids, params = cases.tunnel_with_sphere(levels=levels, wall_model=True)
    mesh, center, radius = common.tunnel_sphere_mesh(grids)
    return grids, params, mesh, common.tunnel_params(center, radius)


def _newest(d, fin, t):
    return d.download("rho"), d.download("vel_temp" if t_sub_after(fin, t) % 2 == 0 else "vel")


N_STEPS = 8


@pytest.fixture(scope="module", params=[1, 2, 3])
def stepped(gpu, request):
    """a tunnel of 1, 2, 3 levels and the host restatement of the record after each of N_STEPS coarse steps, from the fields a second
    set of levels downloads after stepping there one step at a time; computed once, shared, never changed"""
    levels = request.param
    grids, params, mesh, sparams = _tunnel(levels)
    fin = levels - 1
    plan = ss.plan_surface(mesh, grids[fin], sparams)
    assert plan.found.sum() > 500
    ref = [adapt(g, 0) for g in grids]
    want, wrong = {}, {}
    try:
        for t in range(1, N_STEPS + 1):
            execute_timestep_batch(ref, t, 1, U, params)
            rho, vel = _newest(ref[fin], fin, t)
            want[t] = fs.host_record(mesh, plan, rho, vel, grids[fin].tau, sparams)
            wrong[t] = fs.host_record(mesh, plan, rho, ref[fin].download("vel" if t_sub_after(fin, t) % 2 == 0 else "vel_temp"),
                                      grids[fin].tau, sparams)
        end_state = [{n: d.download(n) for n in STATES} for d in ref]
    finally:
        for d in ref:
            d.close()
    return SimpleNamespace(levels=levels, fin=fin, grids=grids, params=params, mesh=mesh, sparams=sparams, plan=plan, want=want,
                           wrong=wrong, end_state=end_state)


def _run(s, start, interval, batch, capacity=16):
    dev = [adapt(g, 0) for g in s.grids]
    F = fs.from_mesh(s.mesh, s.plan, dev[s.fin], s.fin, s.grids[s.fin].tau, s.sparams, start, interval, capacity)
    try:
        for t0 in range(1, N_STEPS + 1, batch):
            execute_timestep_batch(dev, t0, batch, U, s.params, forces=F)
        got = F.download()
        state = [{n: d.download(n) for n in STATES} for d in dev]
    finally:
        F.close()
        for d in dev:
            d.close()
    return got, state


@pytest.mark.gpu
@pytest.mark.parametrize("start,interval", [(1, 1), (2, 3)])
def test_records_sampled_in_the_batch_equal_the_restatement(stepped, start, interval):
    s = stepped
    steps_want = sample_steps(1, N_STEPS, start, interval)
    first = None
    for batch in (8, 4, 1):
        (steps, sums, cov), state = _run(s, start, interval, batch)
        assert steps.tolist() == list(steps_want), batch
        for i, t in enumerate(steps_want):
            assert _same((sums[i], cov[i]), s.want[t]), (s.levels, batch, t, sums[i], s.want[t][0])
            assert not _same((sums[i], cov[i]), s.wrong[t])          # the other velocity buffer gives another record
        if first is None:
            first = (sums, cov)
        assert np.array_equal(_bits(sums), _bits(first[0])) and np.array_equal(cov, first[1])
        # the flow is the flow of a run without the set
        for lvl, (a, b) in enumerate(zip(s.end_state, state)):
            for name in STATES:
                assert np.array_equal(a[name], b[name]), f"level {lvl + 1} {name}: the set changed the flow"
    parities = {t_sub_after(s.fin, t) % 2 for t in steps_want}
    assert parities == ({0, 1} if s.levels == 1 else {1})            # one level: even steps read vel_temp
    assert all(c == int(s.plan.found.sum()) for c in first[1])


@pytest.mark.gpu
def test_native_batch_python_recursion_and_explicit_sample_agree(stepped):
    s = stepped
    got = []
    for mode in ("python", "explicit"):
        dev = [adapt(g, 0) for g in s.grids]
        F = fs.from_mesh(s.mesh, s.plan, dev[s.fin], s.fin, s.grids[s.fin].tau, s.sparams, 2, 3, 4)
        try:
            if mode == "explicit":
                for t in range(1, N_STEPS + 1):
                    execute_timestep_batch(dev, t, 1, U, s.params)
                    if F.is_sample_step(t):
                        F.sample(t_sub_after(s.fin, t), t)
            else:
                execute_timestep_batch(dev, 1, N_STEPS, U, s.params, native=False, forces=F)
            got.append(F.download())
        finally:
            F.close()
            for d in dev:
                d.close()
    for steps, sums, cov in got:
        assert steps.tolist() == [2, 5, 8]
        for i, t in enumerate(steps):
            assert _same((sums[i], cov[i]), s.want[int(t)])


# ---- the ring ----
@pytest.mark.gpu
def test_ring_overflow_fails_before_any_step_and_bad_arguments_are_refused(gpu):
    grids, params, mesh, sparams = _tunnel(2)
    plan = ss.plan_surface(mesh, grids[1], sparams)
    lib = _lib.load()
    dev = [adapt(g, 0) for g in grids]
    other = adapt(grids[1], 0)
    F = fs.from_mesh(mesh, plan, dev[1], 1, grids[1].tau, sparams, 1, 1, 2)
    X = fs.from_mesh(mesh, plan, other, 1, grids[1].tau, sparams, 1, 1, 2)
    fl = params.to_c()
    try:
        execute_timestep_batch(dev, 1, 2, U, params)
        before = [{n: d.download(n) for n in STATES} for d in dev]

        def batch(f, t0, n, start=1, interval=1):
            arr = (C.c_void_p * len(dev))(*[d.handle for d in dev])
            return lib.ludwig_execute_timestep_batch_loads(arr, len(dev), t0, n, float(U), C.byref(fl), None, f.handle, start, interval)
        assert batch(F, 3, 3) == -5 and "overflow the ring" in lib.ludwig_last_error().decode()          # 3 records, room for 2
        assert batch(X, 3, 2) == -1 and "not in the batch" in lib.ludwig_last_error().decode()
        assert batch(F, 3, 2, 1, 0) == -1 and "interval" in lib.ludwig_last_error().decode()
        for lvl, d in enumerate(dev):
            for n in STATES:
                assert np.array_equal(before[lvl][n], d.download(n)), f"level {lvl + 1} {n}: stepped before failing"
        assert F.download()[0].size == 0
        assert batch(F, 3, 2) == 0                                   # fills the ring
        assert batch(F, 5, 1) == -5                                  # full: one more record does not fit
        with pytest.raises(_lib.LudwigError) as e:
            F.sample(t_sub_after(1, 4), 4)
        assert e.value.code == -5 and "ring full" in str(e.value)
        sums = np.zeros((2, 9)); cov = np.zeros(2, np.int64); steps = np.zeros(2, np.int64); k = C.c_int32(0)
        assert lib.ludwig_force_series_download(F.handle, sums.ctypes.data, cov.ctypes.data, steps.ctypes.data, 1, C.byref(k)) == -1
        assert F.download()[0].tolist() == [3, 4]                    # still there after the refused download
        assert batch(F, 5, 1, 7, 1) == 0 and F.download()[0].size == 0      # no sampled step in the batch: nothing to fit
        h = C.c_void_p()
        sp = _lib.SurfaceParams(0.0, 0.5, 0.0, 0.0, 0.0, 1.0, 1.0, 0)
        i32 = lambda *v: np.array(v, np.int32)
        f = np.zeros(3, np.float32)
        for blocks, cells in ((i32(grids[1].n_blocks), i32(0)), (i32(-2), i32(0)), (i32(0), i32(512)), (i32(0), i32(-1))):
            assert lib.ludwig_force_series_create(dev[1].handle, 1, blocks.ctypes.data, cells.ctypes.data, f.ctypes.data, f.ctypes.data,
                                                  f.ctypes.data, f.ctypes.data, C.byref(sp), 4, C.byref(h)) == -1 and not h.value
        assert lib.ludwig_force_series_create(dev[1].handle, 0, None, None, None, None, None, None, C.byref(sp), 0, C.byref(h)) == -1
        assert lib.ludwig_force_series_sample(F.handle, -1, 1) == -1
    finally:
        F.close()
        X.close()
        for d in dev + [other]:
            d.close()


@pytest.mark.gpu
def test_stepper_cuts_its_batch_where_the_ring_fills_and_gives_the_same_records(stepped):
    s = stepped
    got = []
    for capacity in (2, 64):
        st = case.HipStepper(s.grids, upload_state=True)             # the perturbed start of the shared reference, not the rest state
        try:
            plan = st.force_series_setup(s.mesh, s.sparams, 1, 1, capacity)
            assert plan.n == s.plan.n
            st.batch(1, N_STEPS, U, s.params)
            got.append(st.force_series())
        finally:
            st.close()
    for steps, sums, cov in got:
        assert steps.tolist() == list(range(1, N_STEPS + 1))
        for i, t in enumerate(steps):
            assert _same((sums[i], cov[i]), s.want[int(t)]), (capacity, t)


# ---- bystanders ----
@pytest.mark.gpu
def test_probes_and_surface_statistics_unchanged_by_a_force_series(gpu):
    grids, params, mesh, sparams = _tunnel(3)
    pplan = pcommon.tunnel_points(grids)
    splan = ss.plan_surface(mesh, grids[2], sparams)
    out = []
    for with_forces in (False, True):
        dev = [adapt(g, 0) for g in grids]
        P = pm.DeviceProbes(pplan, dev, 8, 1, 2)
        S = ss.DeviceSurfaceStats(splan, dev[2], 2, grids[2].tau, sparams, 1, 1)
        F = fs.from_mesh(mesh, splan, dev[2], 2, grids[2].tau, sparams, 2, 2, 8) if with_forces else None
        try:
            execute_timestep_batch(dev, 1, 8, U, params, probes=P, surface=S, forces=F)
            out.append((P.download(), S.download(), [{n: d.download(n) for n in STATES} for d in dev]))
            if F is not None:
                assert F.download()[0].tolist() == [2, 4, 6, 8]
        finally:
            P.close()
            S.close()
            if F is not None:
                F.close()
            for d in dev:
                d.close()
    (p0, s0, f0), (p1, s1, f1) = out
    assert p0[0].tolist() == p1[0].tolist() == [1, 3, 5, 7]
    assert np.array_equal(p0[1].view(np.uint32), p1[1].view(np.uint32))
    assert s0[1] == s1[1] == 8 and np.array_equal(_bits(s0[0]), _bits(s1[0])) and np.abs(s0[0]).max() > 0
    for a, b in zip(f0, f1):
        for n in STATES:
            assert np.array_equal(a[n], b[n]), n


RE266K = {"basic": {"surface_resolution": 25, "flow": {"velocity": 4.0}, "simulation": {"steps": 16, "output_freq": 16}},
          "advanced": {"diagnostics": {"freq": 8}}}


class _Recording(case.HipStepper):
    """a HipStepper that keeps the finest level's rho and `vel` at the end of every batch() call"""
    saved = {}

    def batch(self, t_start, n, u_curr, params):
        super().batch(t_start, n, u_curr, params)
        fin = len(self.dev) - 1
        _Recording.saved[t_start + n - 1] = (self.dev[fin].download("rho"), self.dev[fin].download("vel"))


@pytest.mark.gpu
def test_ball1m_run_case_writes_the_series_and_nothing_else_changes(gpu, tmp_path):
    out, logs = {}, []
    for on in (False, True):
        over = {**RE266K, "advanced": {**RE266K["advanced"], "forces": {"series": {"enabled": on, "start_step": 3, "interval": 1}}}}
        cfg = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"), over)
        setup = pp.setup_multilevel_domain(cfg, os.path.join(G, "ball1m.stl"))
        d = os.path.join(tmp_path, "on" if on else "off")
        case.run_case(cfg, _Recording if on else case.HipStepper, setup=setup, out_dir=d, log=logs.append if on else None)
        out[on] = (d, setup, cfg)
    off, on = out[False][0], out[True][0]
    names = sorted(os.listdir(off))
    assert sorted(os.listdir(on)) == sorted(names + ["forces_series.csv"])
    for n in names:
        a, b = open(os.path.join(off, n), "rb").read(), open(os.path.join(on, n), "rb").read()
        if n == "convergence.csv":                                     # wall time and MLUPS columns
            strip = lambda raw: [[c for k, c in enumerate(l.split(b",")) if k not in (1, 5)] for l in raw.splitlines()]
            a, b = strip(a), strip(b)
        assert a == b, n
    _, (grids, mesh, params, _), cfg = out[True]
    assert cfg.async_depth == 8 and cfg.diag_freq == 8 and len(grids) == 3 and not cfg.symmetric_analysis
    head = open(os.path.join(on, "forces_series.csv")).readline().strip().split(",")
    rows = [l.strip().split(",") for l in open(os.path.join(on, "forces_series.csv"))][1:]
    assert head == fs.csv_header().split(",") and [int(r[0]) for r in rows] == list(range(3, 17))
    fhead = open(os.path.join(on, "forces.csv")).readline().strip().split(",")
    frows = {int(r[0]): r for r in [l.strip().split(",") for l in open(os.path.join(on, "forces.csv"))][1:]}
    assert sorted(frows) == [8, 16]
    # rows of one batch carry that batch's inlet speed, as forces.csv's row at its end does
    by_step = {int(r[0]): r for r in rows}
    for t in (8, 16):
        assert by_step[t][:3] == frows[t][:3] and by_step[t - 1][2] == frows[t][2]
    # the series' rows at the diagnostics steps against forces.csv: the same float32 terms (the nested finest level ends on an odd
    # sub-step: both read `vel`), summed in float32 pairwise there and in the float64 tree here: within n 2^-23 sum|x_i| per column
    fin = len(grids) - 1
    plan = ss.plan_surface(mesh, grids[fin], params)
    n_tri = plan.n
    for t in (8, 16):
        rho, vel = _Recording.saved[t]
        p, tx, ty, tz, _ = ss.sample_values(plan, rho, vel, grids[fin].tau, params)
        mag = np.abs(forces.force_series_contributions(mesh, p, tx, ty, tz, params)[0].astype(np.float64)).sum(axis=0)
        bound = {"Fx_N": mag[0] + mag[3], "Fy_N": mag[1] + mag[4], "Fz_N": mag[2] + mag[5], "Mx_Nm": mag[6], "My_Nm": mag[7],
                 "Mz_Nm": mag[8]}
        for col, m in bound.items():
            got, want = float(by_step[t][head.index(col)]), float(frows[t][fhead.index(col)])
            tol = n_tri * 2.0 ** -23 * m
            print(f"step {t} {col}: series {got!r} forces.csv {want!r} |diff| {abs(got - want):.3e} bound {tol:.3e}")
            assert m > 0 and abs(got - want) <= tol, (t, col, got, want, tol)
        assert int(by_step[t][head.index("Coverage")]) == int(np.count_nonzero(np.abs(p) > 1e-10))
    assert len([l for l in logs if l.startswith("force series C")]) == 3
