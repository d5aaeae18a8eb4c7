"""Fourier modes, host side (open_ludwig_amd/modes.py, the advanced.fourier_modes configuration, the mirrors of ludwig_modes_*): the
weight table, the window schedule, finalize on synthetic tones within bounds derived from float32 rounding, the configuration errors by
key name, and what the library refuses without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import yaml

from open_ludwig_amd import _lib, build, case, modes, preprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


# ---- the table ----
@pytest.mark.parametrize("window", ["hann", "rectangular"])
def test_weight_table_columns(window):
    N, interval, ts, freqs = 12, 3, 2.5e-4, (37.0, 110.5, 3.0)
    W = modes.weight_table(N, interval, ts, freqs, window)
    assert W.shape == (N, 1 + 2 * len(freqs)) and W.dtype == np.float64
    n = np.arange(N, dtype=np.float64)
    w = 0.5 * (1.0 - np.cos(2.0 * np.pi * n / N)) if window == "hann" else np.ones(N)
    t = n * interval * ts
    assert np.array_equal(W[:, 0], w)
    for k, f in enumerate(freqs):
        assert np.array_equal(W[:, 1 + 2 * k], w * np.cos(2.0 * np.pi * f * t))
        assert np.array_equal(W[:, 2 + 2 * k], -(w * np.sin(2.0 * np.pi * f * t)))
    if window == "rectangular":
        assert (W[:, 0] == 1.0).all()
    else:
        assert W[0, 0] == 0.0
        assert abs(W[:, 0].sum() - N / 2) <= 4 * N * 2.0 ** -53


@pytest.mark.parametrize("N", [2, 7, 64, 1000])      # (N = 1 has the single weight 0: the identity needs N >= 2)
def test_hann_sum(N):
    w = modes.weight_table(N, 1, 1.0, (), "hann")[:, 0]
    assert w[0] == 0.0 and abs(w.sum() - N / 2) <= 4 * N * 2.0 ** -53


def test_unknown_window_and_sample_count():
    with pytest.raises(ValueError, match="advanced.fourier_modes.window"):
        modes.weight_table(8, 1, 1.0, (1.0,), "hamming")
    with pytest.raises(ValueError, match="advanced.fourier_modes.samples"):
        modes.weight_table(0, 1, 1.0, (1.0,), "hann")


# ---- the schedule ----
@pytest.mark.parametrize("start", [1, 5])
@pytest.mark.parametrize("interval", [1, 3])
def test_rows_and_window_ends_against_a_walk(start, interval):
    N, last = 8, 60
    row, ends, rows = 0, [], {}
    for t in range(1, last + 1):
        if t >= start and (t - start) % interval == 0:
            rows[t] = row
            row += 1
            if row == N:
                ends.append(t)
                row = 0
    for t, r in rows.items():
        assert modes.row_of(t, start, interval, N) == r
    assert modes.window_end_steps(1, last, start, interval, N) == ends and ends
    for first in (1, 7, ends[0], ends[0] + 1, last):
        for stop in (first, min(first + 7, last), last):
            assert modes.window_end_steps(first, stop, start, interval, N) == [e for e in ends if first <= e <= stop]
    with pytest.raises(ValueError):
        modes.row_of(start - 1, start, interval, N)
    if interval > 1:
        with pytest.raises(ValueError):
            modes.row_of(start + 1, start, interval, N)


# ---- finalize on a synthetic tone ----
@pytest.mark.parametrize("window", ["hann", "rectangular"])
@pytest.mark.parametrize("N", [16, 32, 64])
@pytest.mark.parametrize("c,a,phi", [(1.0, 0.01, 0.3), (0.05, 0.02, -2.5), (-0.03, 1e-4, 3.0)])
def test_finalize_recovers_a_tone_on_a_bin(window, N, c, a, phi):
    """v_n = float32(c + a cos(2 pi f t_n + phi)), f on bin b of the window. Each sample is off by at most 2^-24 (|c| + |a|) (float32
    rounding); mean and amplitude are weighted means of the samples (times 2 for the amplitude), so they err by at most 2^-23 (|c| + |a|),
    the phase by that over a. A table frequency two or more bins away reads an amplitude below the same bound."""
    interval, ts = 3, 1.25e-4
    bound = 2.0 ** -23 * (abs(c) + abs(a))
    for b in sorted({2, N // 4, N // 2 - 2}):
        f = b / (N * interval * ts)
        others = [bb for bb in (b + 2, b - 2, N // 2 - 1) if 1 <= bb <= N // 2 - 1 and abs(bb - b) >= 2]
        f_other = others[0] / (N * interval * ts)
        W = modes.weight_table(N, interval, ts, (f, f_other), window)
        t = np.arange(N) * interval * ts
        v = (c + a * np.cos(2.0 * np.pi * f * t + phi)).astype(np.float32)
        S = np.zeros((5, 1))
        for n in range(N):
            modes.host_accumulate(S, W[n], v[n:n + 1])
        mean, amp, phase = modes.finalize(S, W)
        assert abs(mean[0] - c) <= bound, (b, mean[0] - c)
        assert abs(amp[0, 0] - a) <= bound, (b, amp[0, 0] - a)
        dphi = (phase[0, 0] - phi + np.pi) % (2.0 * np.pi) - np.pi
        assert abs(dphi) <= bound / a, (b, dphi)
        assert amp[1, 0] <= bound, (b, amp[1, 0])


def test_host_accumulate_is_multiply_then_add_and_propagates_non_finite():
    S = np.zeros((3, 4))
    v = np.array([1.5, np.nan, np.inf, -2.0], dtype=np.float32)
    modes.host_accumulate(S, np.array([2.0, 0.0, 2.0 ** -60]), v)
    modes.host_accumulate(S, np.array([1.0, 1.0, 1.0]), np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32))
    want0 = np.float64(2.0) * v.astype(np.float64) + np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32).astype(np.float64)
    assert np.array_equal(S[0], want0, equal_nan=True)
    assert np.isnan(S[1, 1]) and np.isnan(S[1, 2]) and S[1, 0] == np.float64(np.float32(0.1))      # 0 x NaN and 0 x Inf are NaN
    assert S[2, 0] == 2.0 ** -60 * 1.5 + np.float64(np.float32(0.1))


# ---- configuration ----
def _config(tmp_path, fm):
    with open(os.path.join(G, "ball1m_config.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    if fm is not None:
        cfg.setdefault("advanced", {})["fourier_modes"] = fm
    p = tmp_path / "case.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


class _Params:
    u_physical, reference_length, time_scale = 10.0, 0.5, 1.0e-3


def test_configuration_defaults_and_strouhal(tmp_path):
    off = pp.load_case_configuration(_config(tmp_path, None))
    assert off.fourier_modes_enabled is False and off.fourier_modes_frequencies == () and off.fourier_modes_strouhal == ()
    assert pp.load_case_configuration(_config(tmp_path, {"enabled": False, "samples": -3})).fourier_modes_enabled is False
    on = pp.load_case_configuration(_config(tmp_path, {"enabled": True, "start_step": 5, "interval": 3, "samples": 8, "frequencies": [12.5],
                                                       "strouhal": [0.2, 0.4], "window": "rectangular", "repeat": False}))
    assert (on.fourier_modes_enabled, on.fourier_modes_start_step, on.fourier_modes_interval, on.fourier_modes_samples) == (True, 5, 3, 8)
    assert on.fourier_modes_window == "rectangular" and on.fourier_modes_repeat is False
    lines = []
    plan = modes.plan_modes(on, _Params, lines.append)
    assert plan.frequencies_hz == (12.5, 0.2 * 10.0 / 0.5, 0.4 * 10.0 / 0.5)          # frequencies first, then St u / L
    assert plan.strouhal == pytest.approx((12.5 * 0.5 / 10.0, 0.2, 0.4), rel=1e-15)
    assert np.array_equal(plan.W, modes.weight_table(8, 3, 1.0e-3, plan.frequencies_hz, "rectangular"))
    assert len(lines) == 3 and all("shorter than one period" in l for l in lines)     # 24 ms against periods of 80, 250 and 125 ms
    dflt = pp.load_case_configuration(_config(tmp_path, {"enabled": True, "frequencies": [1.0]}))
    assert (dflt.fourier_modes_start_step, dflt.fourier_modes_interval, dflt.fourier_modes_window, dflt.fourier_modes_repeat) == (1, 1, "hann", True)


@pytest.mark.parametrize("fm,key", [
    ({"enabled": True, "samples": 8}, "advanced.fourier_modes"),                                          # zero modes
    ({"enabled": True, "frequencies": [1.0] * 9, "strouhal": [0.1] * 8}, "advanced.fourier_modes"),      # 17 modes
    ({"enabled": True, "frequencies": [1.0], "samples": 0}, "advanced.fourier_modes.samples"),
    ({"enabled": True, "frequencies": [1.0], "samples": 65537}, "advanced.fourier_modes.samples"),
    ({"enabled": True, "frequencies": [1.0], "window": "hamming"}, "advanced.fourier_modes.window"),
    ({"enabled": True, "frequencies": [1.0], "interval": 0}, "advanced.fourier_modes.interval"),
    ({"enabled": True, "frequencies": [-1.0]}, "advanced.fourier_modes.frequencies"),
    ("yes", "advanced.fourier_modes"),
])
def test_configuration_errors_name_the_key(tmp_path, fm, key):
    with pytest.raises(ValueError) as e:
        pp.load_case_configuration(_config(tmp_path, fm))
    assert key in str(e.value)


def test_nyquist_violation_names_the_key(tmp_path):
    ok = pp.load_case_configuration(_config(tmp_path, {"enabled": True, "interval": 2, "frequencies": [249.9]}))
    modes.plan_modes(ok, _Params)                                  # 249.9 Hz x 2 ms < 0.5
    for f in (250.0, 400.0):
        bad = pp.load_case_configuration(_config(tmp_path, {"enabled": True, "interval": 2, "frequencies": [f]}))
        with pytest.raises(ValueError, match=r"advanced\.fourier_modes.*Nyquist"):
            modes.plan_modes(bad, _Params)
    bad = pp.load_case_configuration(_config(tmp_path, {"enabled": True, "strouhal": [26.0]}))       # 520 Hz at 1 ms
    with pytest.raises(ValueError, match=r"advanced\.fourier_modes.*Nyquist"):
        modes.plan_modes(bad, _Params)


def test_run_case_refuses_a_stepper_without_modes_setup(tmp_path):
    """no host fallback: the test oracle stepper, which offers no modes_setup, ends the run before the first step"""
    from _steppers import OracleStepper
    cfg = pp.load_case_configuration(os.path.join(G, "ball1m_config.yaml"),
                                     {"basic": {"surface_resolution": 25}, "advanced": {"fourier_modes": {"enabled": True, "samples": 4,
                                                                                                          "strouhal": [0.2]}}})
    setup = pp.setup_multilevel_domain(cfg, os.path.join(G, "ball1m.stl"))
    with pytest.raises(RuntimeError, match=r"advanced\.fourier_modes.*modes_setup"):
        case.run_case(cfg, OracleStepper, steps=2, setup=setup)


# ---- mirrors ----
FUNCTIONS = ("ludwig_modes_create", "ludwig_modes_destroy", "ludwig_modes_reset", "ludwig_modes_accumulate", "ludwig_modes_download")


def test_header_binding_and_julia_agree():
    header = open(os.path.join(ROOT, "include", "ludwig_hip.h")).read()
    assert re.search(r"LUDWIG_OBSERVE_MODES\s*=\s*5\b", header) and "typedef struct LudwigModes LudwigModes;" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ludwig_[a-z_0-9]+)\s*\(", code))
    for fn in FUNCTIONS:
        assert fn in declared and fn in _lib.EXPORTED_SYMBOLS, fn
    assert _lib.OBSERVE_MODES == 5
    assert re.search(r"#define LUDWIG_ABI_VERSION 1\b", header)
    build.build_library()
    assert _lib.load().ludwig_abi_version() == 1
    jl = open(os.path.join(ROOT, "julia", "LudwigHIP.jl")).read()
    assert re.search(r"^const OBSERVE_MODES = Int32\(5\)\s*$", jl, re.M)
    assert "entry(OBSERVE_MODES, modes, start_step, interval)" in jl
    called = set(re.findall(r"ccall\(\(:(\w+), LIB\)", jl))
    assert set(FUNCTIONS) <= called and called <= declared, called - declared


# ---- without a device ----
def test_library_refuses_bad_arguments_without_a_device():
    build.build_library()
    lib = _lib.load()
    W = np.ones((4, 3))
    one = (C.c_void_p * 1)(None)
    out = C.c_void_p(1)
    assert lib.ludwig_modes_create(None, 1, 3, 4, W.ctypes.data, C.byref(out)) == -1 and b"null" in lib.ludwig_last_error()
    assert out.value is None                                                       # the out pointer is cleared first
    assert lib.ludwig_modes_create(one, 1, 3, 4, None, C.byref(out)) == -1 and b"null" in lib.ludwig_last_error()
    assert lib.ludwig_modes_create(one, 1, 3, 4, W.ctypes.data, None) == -1 and b"null" in lib.ludwig_last_error()
    for m, n, word in ((0, 4, b"columns"), (34, 4, b"columns"), (3, 0, b"rows"), (3, 65537, b"rows")):
        assert lib.ludwig_modes_create(one, 1, m, n, W.ctypes.data, C.byref(out)) == -1
        assert word in lib.ludwig_last_error() and out.value is None
    assert lib.ludwig_modes_create(one, 1, 3, 4, W.ctypes.data, C.byref(out)) == -1 and b"level 1 is null" in lib.ludwig_last_error()
    assert lib.ludwig_modes_accumulate(None, 0, 1, 0) == -1 and b"null" in lib.ludwig_last_error()
    assert lib.ludwig_modes_reset(None) == -1 and b"null" in lib.ludwig_last_error()
    assert lib.ludwig_modes_download(None, 0, 0, None, 0, None) == -1 and b"null" in lib.ludwig_last_error()
    lib.ludwig_modes_destroy(None)                                                  # destroying nothing is a no-op
