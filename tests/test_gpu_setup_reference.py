"""The HIP step on levels the REAL set-up made (preprocess.setup_multilevel_domain from an STL file), not on cases.add_sphere's.

Two planted cases of tests/_setup_cases.py, each 2 levels of at most 64 blocks: the thin tilted slab with wall model and sponge, and the
aligned box at dx = 0.02 whose axis links have q = 0.5 and q = 1.0. Their set-up arrays are pinned by tests/test_setup_reference_host.py
(both methods, bit for bit, against the restatement); here they drive the step:
  - 4 coarse steps in one native batch of case.HipStepper equal the oracle bit for bit on every level: both population buffers, rho,
    both velocity buffers, and f_post_collision at the rows the Bouzidi pass read;
  - each single step equals tests/_step_ref.coarse_step in float64 under _step_ref.bound, MAX_E_REF and MAX_EXCLUDED_SHARE, unchanged;
  - ludwig_bouzidi_correction alone on an uploaded state of the slab equals the restatement's Bouzidi arm (tests/_step_ref.bouzidi_arm, the
    function _level_step calls, in float32) bit for bit.
"""
import numpy as np
import pytest

import _setup_cases as C
import _step_ref as sr
import _step_ref_cases as sc
from open_ludwig_amd import adapt, cases, execute_timestep_batch, physics, preprocess as pp
from open_ludwig_amd.case import HipStepper
from oracle import oracle

pytestmark = pytest.mark.gpu
F32 = np.float32
U = 0.05
STEPS = (1, 2, 3, 4)
NAMES = ("thin_slab", "aligned_box_002")


def build(name, folder):
    kw, stl = C.device_case(name, folder)
    cfg = pp.CaseConfig(**kw)
    grids, _, dp, rep = pp.setup_multilevel_domain(cfg, stl)
    assert len(grids) == 2 and all(len(g.active_block_coords) <= 64 for g in grids) and rep.bouzidi_cells[-1] > 0
    params = pp.solver_params(cfg, dp)
    for i, g in enumerate(grids):
        cases.init_perturbed(g, 7 + i, u_mean=U)
    return grids, params


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("setup_cases")


def test_cases_are_what_they_claim(folder):
    grids, params = build("aligned_box_002", folder)
    q = np.asarray(grids[-1].bouzidi_q_map).astype(np.float64)
    assert (q == 0.5).sum() > 1000 and (q == 1.0).sum() > 1000 and grids[-1].dx == float(F32(0.02))
    grids, params = build("thin_slab", folder)
    assert params.wall_model_active and all((g.sponge > 0).any() for g in grids) and all((g.wall_dist < F32(100)).any() for g in grids)
    assert grids[-1].dx == 2.0 ** -5


@pytest.mark.parametrize("name", NAMES)
def test_set_up_levels_step_like_the_restatement_and_the_oracle(gpu, folder, name):
    grids, params = build(name, folder)
    start = [{n: np.array(getattr(g, n)) for n in sr._STATE + ("f_post_collision",) if hasattr(g, n)} for g in grids]
    worst = dict.fromkeys(("f", "vel", "rho"), 0.0)
    check = None
    for t in STEPS:
        check = sc.StepCheck(grids, params, t, U)
        for k in check.e_ref:
            assert check.e_ref[k] <= sr.MAX_E_REF[k], f"{name} t={t}: e_ref {k} {check.e_ref[k]:.3e} above the recorded {sr.MAX_E_REF[k]:.3e}"
        dev = [adapt(g, 0) for g in grids]
        try:
            execute_timestep_batch(dev, t, 1, F32(U), params, native=True)
            got = []
            for lv, (g, d) in enumerate(zip(grids, dev)):
                assert check.excluded_share[lv] <= sr.MAX_EXCLUDED_SHARE, f"{name} t={t} level {lv + 1}: {check.excluded_share[lv]:.4%} left out"
                ref = check.ref[lv]
                names = [ref.f_name, ref.vel_name, "rho"] + (["f_post_collision"] if ref.post_read is not None else [])
                if ref.old is not None:
                    names += ["f_old", "rho_old", "vel_old"]
                got.append({n: d.download(n) for n in names})
                err = check.compare(lv, g, got[-1], f"{name} t={t} hip")
                for k in err:
                    worst[k] = max(worst[k], err[k])
        finally:
            for d in dev:
                d.close()
        oracle.execute_timestep_batch(grids, t, 1, F32(U), params)
        # the same single step, bit for bit against the oracle
        for lv, g in enumerate(grids):
            ref = check.ref[lv]
            for n, a in got[lv].items():
                if n.endswith("_old"):
                    continue
                want = np.asarray(getattr(g, n))
                if n == "f_post_collision":
                    a, want = a[ref.post_read], want[ref.post_read]
                assert np.array_equal(a.view(np.uint32), want.view(np.uint32)), f"{name} t={t} level {lv + 1} {n}: differs from the oracle"
    print(f"\n{name}: HIP max error / scale " + " ".join(f"{k} {v:.3e}" for k, v in worst.items())
          + "   bounds " + " ".join(f"{k} {sr.bound(k):.3e}" for k in worst))
    # the four steps again as ONE native batch from the start state, against the oracle's state after them
    for g, s in zip(grids, start):
        end = {n: np.array(getattr(g, n)) for n in s}
        for n, a in s.items():
            getattr(g, n)[...] = a
        s.update(end)                                  # s now holds the oracle's end state, g the start state
    st = HipStepper(grids, upload_state=True)
    try:
        st.batch(STEPS[0], len(STEPS), F32(U), params)
        for lv, s in enumerate(start):
            for n in ("f", "f_temp", "rho", "vel", "vel_temp", "f_post_collision"):
                if n not in s or (n == "f_post_collision" and check.ref[lv].post_read is None):
                    continue
                a, want = st.field(lv, n), s[n]
                if n == "f_post_collision":
                    a, want = a[check.ref[lv].post_read], want[check.ref[lv].post_read]
                assert np.array_equal(a.view(np.uint32), want.view(np.uint32)), f"{name} batch level {lv + 1} {n}: differs from the oracle"
    finally:
        st.close()


@pytest.mark.parametrize("t", (1, 2))
def test_bouzidi_correction_alone_equals_the_restatements_arm(gpu, folder, t):
    grids, params = build("thin_slab", folder)
    level = grids[-1]
    rng = np.random.default_rng(3)
    level.f_post_collision[...] = (np.asarray(level.f) * (1.0 + 0.05 * rng.standard_normal(level.f.shape))).astype(np.float32)
    out_name = "f_temp" if t % 2 == 0 else "f"           # the output buffer of step t (src/solver_control.jl:35-41)
    # the restatement's own arm (tests/_step_ref.bouzidi_arm, the function _level_step calls), in float32
    want = np.array(getattr(level, out_name), dtype=np.float32)
    br = np.zeros(want.shape[:4], dtype=np.uint16)
    sr.bouzidi_arm(np.float32, level, sr.geometry(level, params), params, np.asarray(level.f_post_collision), want, br)
    assert ((br & sr.BZ_LT_HALF) != 0).sum() > 100 and ((br & sr.BZ_GE_HALF) != 0).sum() > 100
    dev = adapt(level, 0)
    try:
        physics.apply_bouzidi_correction(dev, t, params.q_min_threshold)
        got = dev.download(out_name)
        other = dev.download("f" if out_name == "f_temp" else "f_temp")
    finally:
        dev.close()
    assert (want != np.asarray(getattr(level, out_name))).sum() > 1000
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    assert np.array_equal(other, np.asarray(getattr(level, "f" if out_name == "f_temp" else "f_temp")))     # the other buffer is left alone
