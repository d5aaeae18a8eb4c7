"""The HIP step against the float64 restatement of the step (tests/_step_ref.py), one coarse step at a time.

Same case table, snapshots and bounds as tests/test_step_reference_host.py. Before every step the snapshot (the host levels' full
float32 state) is uploaded to fresh device levels, one batch of one coarse step runs through execute_timestep_batch (the native
driver), and the downloaded state is compared with ref64 under the bounds and the exclusion rule of tests/_step_ref.py.
The expected values are the restatement's, never the oracle's: the oracle only moves the host state on to the next snapshot, so the
test keeps its meaning for a step that is no longer bit-identical to it. A subset also runs through the Python recursion
(ludwig_step per level) and with 64-bit addressing (LUDWIG_WIDE_ADDR).
"""
import numpy as np
import pytest

import _step_ref as sr
import _step_ref_cases as sc
from open_ludwig_amd import adapt, execute_timestep_batch
from oracle import oracle            # advances the snapshots only

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_case(name, native=True):
    case = sc.CASES[name]
    grids, params = case.build()
    worst = dict.fromkeys(("f", "vel", "rho"), 0.0)
    for t in case.steps:
        check = sc.StepCheck(grids, params, t, case.u)
        dev = [adapt(g, 0) for g in grids]
        try:
            execute_timestep_batch(dev, t, 1, F32(case.u), params, native=native)
            for lv, (g, d) in enumerate(zip(grids, dev)):
                share = check.excluded_share[lv]
                assert share <= sr.MAX_EXCLUDED_SHARE, f"{name} t={t} level {lv + 1}: {share:.4%} of the fluid cells left out"
                if case.smooth and not case.wall:
                    assert share == 0
                ref = check.ref[lv]
                names = [ref.f_name, ref.vel_name, "rho"]
                if ref.post_read is not None:
                    names.append("f_post_collision")
                if ref.old is not None:
                    names += ["f_old", "rho_old", "vel_old"]
                err = check.compare(lv, g, {n: d.download(n) for n in names}, f"{name} t={t} hip")
                for k in err:
                    worst[k] = max(worst[k], err[k])
        finally:
            for d in dev:
                d.close()
        oracle.execute_timestep_batch(grids, t, 1, F32(case.u), params)
    print(f"\n{name}: HIP max error / scale " + " ".join(f"{k} {v:.3e}" for k, v in worst.items())
          + "   bounds " + " ".join(f"{k} {sr.bound(k):.3e}" for k in worst))
    return worst


@pytest.mark.parametrize("name", list(sc.CASES))
def test_hip_batch_matches_float64_restatement(gpu, name):
    run_case(name)


@pytest.mark.parametrize("name", sc.SUBSET)
def test_hip_step_per_level_matches_float64_restatement(gpu, name):
    """the Python recursion: ludwig_step and ludwig_save_old level by level"""
    run_case(name, native=False)


@pytest.mark.parametrize("name", sc.SUBSET)
def test_hip_wide_addressing_matches_float64_restatement(gpu, monkeypatch, name):
    monkeypatch.setenv("LUDWIG_WIDE_ADDR", "1")
    run_case(name)
