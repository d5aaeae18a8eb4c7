"""The subgrid model made visible (no reference counterpart: the reference folds its WALE eddy viscosity into tau_turb and drops it).

The device (libludwig_hip.so, ludwig_level_subgrid_*) evaluates the step's own WALE function (kernels.hpp wale_state), in float32, on
the gradient the step forms: g_ij = 0.5 (u_i(+e_j) - u_i(-e_j)) in lattice units, the cell's own value where no block lies across a
face. Evaluated on the velocity sub-step t wrote, nu_t is bit for bit the value sub-step t + 1 collides with. nu_t is the EFFECTIVE
viscosity: it includes the `nu_sgs_background` floor, max(nu_model, nu_bg), because that is what the step uses; the code field says
where the floor acts (CODES). c_wale and nu_sgs_background are the ones the level's last step was given, not arguments.

Per owned cell the device keeps three Float64 sums over the samples, each a plain sequential addition in sample order: S_nu of nu_t,
S_nunu of nu_t^2 and S_eps of nu_t |S|^2 with |S|^2 = 2 S_ij S_ij (products of the float32 values widened first: exact). This module
holds the host side: the finalisation of the sums.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from .forces import lattice_viscosity

# the code field: which branch of the model gave nu_t
CODE_NO_OP1, CODE_NO_DENOM, CODE_FLOOR, CODE_MODEL = range(4)
CODES = {CODE_NO_OP1: "OP1 <= 1e-12: no model value, nu_t = nu_sgs_background",
         CODE_NO_DENOM: "denom <= 1e-12: no model value, nu_t = nu_sgs_background",
         CODE_FLOOR: "the model is evaluated and is not above nu_sgs_background: the floor wins",
         CODE_MODEL: "the model is above the floor"}
DEFAULT_CK = 0.094
# flow_mean_%06d.vtu: (VTU name, key of finalize's result), in file order
MEAN_ARRAYS = (("EddyViscosityRatioMean", "nu_ratio_mean"), ("EddyViscosityRatioRms", "nu_ratio_rms"), ("SubgridTke", "k_sgs"),
               ("SubgridDissipation", "eps_sgs"), ("ResolvedTkeShare", "resolved_share"))


def level_viscosity(tau) -> np.float32:
    """nu of a level from its tau, Float32: the expression the wall shear uses (forces.lattice_viscosity)"""
    return np.float32(lattice_viscosity(tau))


def ratio_field(nu_t: np.ndarray, tau) -> np.ndarray:
    """EddyViscosityRatio of flow_%06d.vtu: nu_t / nu of the level, a Float32 division"""
    return (np.asarray(nu_t, dtype=np.float32) / level_viscosity(tau)).astype(np.float32)


def finalize(s_nu: np.ndarray, s_nunu: np.ndarray, s_eps: np.ndarray, n: int, nu_level, c_k: float = DEFAULT_CK,
             resolved_tke: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """sums over n samples -> Float64 arrays of the sums' shape:
      nu_ratio_mean   <nu_t> / nu
      nu_ratio_rms    sqrt(max(<nu_t^2> - <nu_t>^2, 0)) / nu
      k_sgs           <nu_t^2> / (c_k Delta)^2, the mean of Yoshizawa's k_sgs = (nu_t / (c_k Delta))^2 with Delta = 1 cell of the level:
                      exact, because the sum is of nu_t^2 and not of nu_t. Lattice velocity is the same unit on every level, as for the
                      resolved k of statistics.finalize. nu_t includes the background floor, so this is the model's EFFECTIVE value.
      eps_sgs         <nu_t |S|^2>, the mean subgrid dissipation in lattice units of the level
      resolved_share  with resolved_tke (statistics.finalize's tke): k / (k + k_sgs), Pope's measure of a resolved LES (>= 0.8); 1.0
                      where the denominator is 0
    nu_level: the level's molecular viscosity (level_viscosity). n = 0 gives NaN everywhere."""
    with np.errstate(invalid="ignore", divide="ignore"):
        nn = np.float64(n) if n > 0 else np.float64(np.nan)
        nu = np.float64(nu_level)
        mean = np.asarray(s_nu, dtype=np.float64) / nn
        mean2 = np.asarray(s_nunu, dtype=np.float64) / nn
        out = {"nu_ratio_mean": mean / nu,
               "nu_ratio_rms": np.sqrt(np.maximum(mean2 - mean * mean, 0.0)) / nu,
               "k_sgs": mean2 / (np.float64(c_k) * 1.0) ** 2,
               "eps_sgs": np.asarray(s_eps, dtype=np.float64) / nn}
        if resolved_tke is not None:
            k = np.asarray(resolved_tke, dtype=np.float64)
            den = k + out["k_sgs"]
            out["resolved_share"] = np.where(den == 0.0, 1.0, k / np.where(den == 0.0, 1.0, den))
    return out
