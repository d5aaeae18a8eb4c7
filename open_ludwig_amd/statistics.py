"""Time-averaged flow statistics (no reference counterpart: the reference writes instantaneous snapshots only).

The sums live on the device (libludwig_hip.so, ludwig_level_stats_*): per owned cell, in Float64, S_rho, S_u (x, y, z) and
S_uu (xx, yy, zz, xy, yz, xz - VTK's symmetric-tensor order), each a plain sequential addition in sample order. This module holds
the host side: which sub-step a level has finished after a coarse step, which coarse steps are sampled, and the finalisation
of the sums into mean rho, mean u, the Reynolds stresses R_ij = <u_i u_j> - <u_i><u_j> and k = tr(R) / 2.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

# (i, j) of the six S_uu components
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))


def t_sub_after(level_index: int, t_coarse: int) -> int:
    """the sub-step level `level_index` (0-based) has finished once coarse step t_coarse is over: 2^l t + 2^l - 1
    (level 1 follows the parity of t; every finer level ends on an odd sub-step, whose output is `vel`)"""
    m = 1 << int(level_index)
    return m * int(t_coarse) + m - 1


def is_sample_step(step: int, start_step: int, interval: int) -> bool:
    return step >= start_step and (step - start_step) % interval == 0


def check_schedule(what: str, start_step: int, interval: int) -> Tuple[int, int]:
    """(start_step, interval) of an observer's schedule as ints; ValueError below 1"""
    if int(start_step) < 1 or int(interval) < 1:
        raise ValueError(f"{what}: start_step {start_step} and interval {interval} must be >= 1")
    return int(start_step), int(interval)


def sample_steps(first: int, last: int, start_step: int, interval: int) -> List[int]:
    """the sampled coarse steps in [first, last]: start_step + k interval, k = 0, 1, ..."""
    if last < max(first, start_step):
        return []
    lo = max(first, start_step)
    k0 = -(-(lo - start_step) // interval)
    return list(range(start_step + k0 * interval, last + 1, interval))


def finalize(s_rho: np.ndarray, s_u: np.ndarray, s_uu: np.ndarray, n: int) -> Dict[str, np.ndarray]:
    """sums [..], [.., 3], [.., 6] over n samples -> mean_rho [..], mean_u [.., 3], reynolds_stress [.., 6] (xx yy zz xy yz xz),
    tke [..]; Float64. n = 0 gives NaN everywhere."""
    with np.errstate(invalid="ignore", divide="ignore"):
        nn = np.float64(n) if n > 0 else np.float64(np.nan)
        mean_rho = s_rho / nn
        mean_u = s_u / nn
        rs = np.empty(s_uu.shape, dtype=np.float64, order="F")
        for m, (i, j) in enumerate(PAIRS):
            rs[..., m] = s_uu[..., m] / nn - mean_u[..., i] * mean_u[..., j]
        tke = 0.5 * (rs[..., 0] + rs[..., 1] + rs[..., 2])
    return {"mean_rho": mean_rho, "mean_u": mean_u, "reynolds_stress": rs, "tke": tke}
