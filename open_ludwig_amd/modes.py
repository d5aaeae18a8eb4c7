"""Fourier modes of the flow accumulated while stepping (advanced.fourier_modes; no reference counterpart).

Per cell and per chosen frequency f_k the run accumulates the windowed sums sum_n w_n v_n cos(2 pi f_k t_n) and -sum_n w_n v_n sin(2 pi f_k
t_n) of v = rho, ux, uy, uz over the N samples of a window, t_n = n interval time_scale counted from the window's first sample. The device
library knows only a weight table W [N, 1 + 2K] (weight_table) and adds the state times one row per sample (ludwig_modes_*, _lib.ModeSet):
S[m] = S[m] + W[n, m] * float64(v), one multiply and then one add, which host_accumulate restates bit for bit. finalize turns the sums of a
finished window into the windowed mean, and an amplitude and a phase per frequency:
    sw = sum_n w_n,  mean = S[0] / sw
    A_k = (S[1 + 2k] - mean sum_n W[n, 1 + 2k]) + i (S[2 + 2k] - mean sum_n W[n, 2 + 2k])      (the mean's leakage removed, by linearity)
    amplitude = 2 |A_k| / sw,  phase = atan2(Im A_k, Re A_k)
so that a signal c + a cos(2 pi f_k t + phi) with f_k on a bin of the window gives mean c, amplitude a and phase phi: the phase is that of
a cosine at the window's first sample.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

WINDOWS = ("hann", "rectangular")
MAX_MODES = 16
MAX_SAMPLES = 65536
KEY = "advanced.fourier_modes"


def window_weights(n_samples: int, window: str) -> np.ndarray:
    """w_n, n = 0..N-1: "hann" the periodic 0.5 (1 - cos(2 pi n / N)), "rectangular" 1"""
    n = np.arange(int(n_samples), dtype=np.float64)
    if window == "hann":
        return 0.5 * (1.0 - np.cos(2.0 * np.pi * n / float(n_samples)))
    if window == "rectangular":
        return np.ones(int(n_samples), dtype=np.float64)
    raise ValueError(f"{KEY}.window must be one of {', '.join(WINDOWS)}, got {window!r}")


def weight_table(n_samples: int, interval: int, time_scale: float, frequencies_hz: Sequence[float], window: str = "hann") -> np.ndarray:
    """W [N, 1 + 2K] Float64: column 0 = w_n, column 1 + 2k = w_n cos(2 pi f_k t_n), column 2 + 2k = -(w_n sin(2 pi f_k t_n)) with
    t_n = n interval time_scale"""
    if int(n_samples) < 1:
        raise ValueError(f"{KEY}.samples must be >= 1, got {n_samples}")
    w = window_weights(n_samples, window)
    t = np.arange(int(n_samples), dtype=np.float64) * float(int(interval)) * float(time_scale)
    W = np.empty((int(n_samples), 1 + 2 * len(frequencies_hz)), dtype=np.float64)
    W[:, 0] = w
    for k, f in enumerate(frequencies_hz):
        arg = 2.0 * np.pi * float(f) * t
        W[:, 1 + 2 * k] = w * np.cos(arg)
        W[:, 2 + 2 * k] = -(w * np.sin(arg))
    return W


def row_of(step: int, start_step: int, interval: int, n_samples: int) -> int:
    """the table row of sampled coarse step `step` = start_step + (j N + n) interval: n"""
    d = int(step) - int(start_step)
    if d < 0 or d % int(interval) != 0:
        raise ValueError(f"fourier modes: step {step} is no sampled step (start {start_step}, interval {interval})")
    return (d // int(interval)) % int(n_samples)


def window_end_steps(first: int, last: int, start_step: int, interval: int, n_samples: int) -> List[int]:
    """the steps of first..last at which a window completes: start_step + (j N + N - 1) interval, j >= 0"""
    span = int(n_samples) * int(interval)
    e0 = int(start_step) + (int(n_samples) - 1) * int(interval)
    j = max(0, -((e0 - int(first)) // span))
    out = []
    while e0 + j * span <= int(last):
        out.append(e0 + j * span)
        j += 1
    return out


def host_accumulate(S: np.ndarray, w_row: np.ndarray, v: np.ndarray) -> np.ndarray:
    """one sample as the device takes it: S [M, ...] Float64, w_row [M], v [...] Float32 -> S[m] = S[m] + w_row[m] * float64(v), in place"""
    v64 = np.asarray(v).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(S.shape[0]):
            S[m] = S[m] + np.float64(w_row[m]) * v64
    return S


def finalize(S, W: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(mean [...], amplitude [K, ...], phase [K, ...]) in Float64 from the sums S [M, ...] of a finished window of table W [N, M]"""
    S = np.asarray(S, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    K = (W.shape[1] - 1) // 2
    sw = W[:, 0].sum()
    col = W.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = S[0] / sw
        amp = np.empty((K,) + S.shape[1:], dtype=np.float64)
        phase = np.empty_like(amp)
        for k in range(K):
            re = S[1 + 2 * k] - mean * col[1 + 2 * k]
            im = S[2 + 2 * k] - mean * col[2 + 2 * k]
            amp[k] = 2.0 * np.hypot(re, im) / sw
            phase[k] = np.arctan2(im, re)
    return mean, amp, phase


# ---- configuration (preprocess.CaseConfig.fourier_modes_*) ----
@dataclass(frozen=True)
class ModesPlan:
    start_step: int
    interval: int
    samples: int
    window: str
    repeat: bool
    frequencies_hz: Tuple[float, ...]
    strouhal: Tuple[float, ...]         # f L / U of every mode
    W: np.ndarray

    @property
    def n_modes(self) -> int:
        return len(self.frequencies_hz)


def plan_modes(cfg, params, log=None) -> ModesPlan:
    """the frequencies (cfg.fourier_modes_frequencies, then cfg.fourier_modes_strouhal as f = St u_physical / reference_length of
    `params`), checked against the sampling rate, and the weight table. ValueError by key name."""
    scale = float(params.u_physical) / float(params.reference_length)
    freqs = [float(f) for f in cfg.fourier_modes_frequencies] + [float(s) * scale for s in cfg.fourier_modes_strouhal]
    if not 1 <= len(freqs) <= MAX_MODES:
        raise ValueError(f"{KEY}: frequencies and strouhal must name 1 to {MAX_MODES} modes in all, got {len(freqs)}")
    dt = float(cfg.fourier_modes_interval) * float(params.time_scale)
    n = int(cfg.fourier_modes_samples)
    for f in freqs:
        if not (math.isfinite(f) and f > 0.0):
            raise ValueError(f"{KEY}: frequency {f} Hz must be finite and > 0")
        if f * dt >= 0.5:
            raise ValueError(f"{KEY}: frequency {f:.6g} Hz is at or above the sampling Nyquist {0.5 / dt:.6g} Hz "
                             f"(interval {cfg.fourier_modes_interval} x time step {params.time_scale:.6g} s)")
        if f * dt * n < 1.0 and log:
            log(f"fourier modes: warning: the window of {n} samples ({n * dt:.6g} s) is shorter than one period of {f:.6g} Hz")
    W = weight_table(n, cfg.fourier_modes_interval, params.time_scale, freqs, cfg.fourier_modes_window)
    return ModesPlan(int(cfg.fourier_modes_start_step), int(cfg.fourier_modes_interval), n, str(cfg.fourier_modes_window),
                     bool(cfg.fourier_modes_repeat), tuple(freqs), tuple(f / scale for f in freqs), W)


# ---- result files ----
CSV_HEADER = ("LastStep,FirstStep,Samples,Interval,Window,Mode,Frequency_Hz,Strouhal,Level,FluidCells,HalfSumVelocityAmplitudeSquared")


def level_energy(amp_k: np.ndarray, obstacle: np.ndarray) -> Tuple[int, float]:
    """(non-obstacle cells, 1/2 sum over them of |u_x|^2 + |u_y|^2 + |u_z|^2 in Float64) of one mode's amplitude [8,8,8,nb,4] on a level"""
    fluid = ~np.asarray(obstacle).astype(bool)
    u = np.asarray(amp_k, dtype=np.float64)[..., 1:4][fluid]
    return int(fluid.sum()), 0.5 * float((u[:, 0] ** 2 + u[:, 1] ** 2 + u[:, 2] ** 2).sum())


def csv_row(plan: ModesPlan, first_step: int, last_step: int, k: int, level_id: int, n_fluid: int, energy: float) -> str:
    return "%d,%d,%d,%d,%s,%d,%.10e,%.10e,%d,%d,%.10e" % (last_step, first_step, plan.samples, plan.interval, plan.window, k,
                                                        plan.frequencies_hz[k], plan.strouhal[k], level_id, n_fluid, energy)
