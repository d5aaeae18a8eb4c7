"""Float32 restatement of the subgrid observer (kernels.hpp wale_state, k_subgrid), for the tests.

Written from the model's formula in the step's operand order (reference src/physics_kernels.jl:251-300; kernels.hpp wale_state, which
finish_cell calls), on tests/_gradient_ref.gradient_tensor(vel, neighbor_table, scale = 1): the gradient in lattice units with the
cell's own value where no block lies across a face. Every operation is one float32 numpy ufunc, so the result is what the device
computes with -ffp-contract=off, bit for bit. It does not call tests/_step_ref.py: test_subgrid_host.py ties the two together.
The Float64 sums are restated as the sequential additions the device makes."""
import numpy as np

import _gradient_ref as gref

F32 = np.float32
F64 = np.float64
TINY = F32(1.0e-12)
NO_OP1, NO_DENOM, FLOOR, MODEL = range(4)


def wale_state(g, c_wale, nu_bg):
    """g[i][j]: float32 arrays. Returns (nu_eddy after the floor, s2 = 2 OP2, code int8), obstacle cells NOT yet masked."""
    (g11, g12, g13), (g21, g22, g23), (g31, g32, g33) = g
    c_wale, nu_bg = F32(c_wale), F32(nu_bg)
    half, two, three = F32(0.5), F32(2.0), F32(3.0)
    with np.errstate(all="ignore"):
        gsq11 = g11 * g11 + g12 * g21 + g13 * g31
        gsq12 = g11 * g12 + g12 * g22 + g13 * g32
        gsq13 = g11 * g13 + g12 * g23 + g13 * g33
        gsq21 = g21 * g11 + g22 * g21 + g23 * g31
        gsq22 = g21 * g12 + g22 * g22 + g23 * g32
        gsq23 = g21 * g13 + g22 * g23 + g23 * g33
        gsq31 = g31 * g11 + g32 * g21 + g33 * g31
        gsq32 = g31 * g12 + g32 * g22 + g33 * g32
        gsq33 = g31 * g13 + g32 * g23 + g33 * g33
        tr_term = (gsq11 + gsq22 + gsq33) / three
        sd11, sd22, sd33 = gsq11 - tr_term, gsq22 - tr_term, gsq33 - tr_term
        sd12, sd13, sd23 = half * (gsq12 + gsq21), half * (gsq13 + gsq31), half * (gsq23 + gsq32)
        s12, s13, s23 = half * (g12 + g21), half * (g13 + g31), half * (g23 + g32)
        op1 = sd11 * sd11 + sd22 * sd22 + sd33 * sd33 + two * (sd12 * sd12 + sd13 * sd13 + sd23 * sd23)
        op2 = g11 * g11 + g22 * g22 + g33 * g33 + two * (s12 * s12 + s13 * s13 + s23 * s23)
        has_op1 = op1 > TINY
        op1_32 = op1 * np.sqrt(op1)
        op2_52 = op2 * op2 * np.sqrt(np.maximum(op2, TINY))                      # np.maximum propagates NaN, as Julia's max does
        denom = op2_52 + op1 * np.sqrt(np.sqrt(np.maximum(op1, TINY)))
        has_denom = has_op1 & (denom > TINY)
        model = (c_wale * c_wale) * op1_32 / denom
        nu = np.where(has_denom, model, F32(0.0)).astype(F32)
        above = has_denom & (nu > nu_bg)
        code = np.where(above, MODEL, np.where(has_denom, FLOOR, np.where(has_op1, NO_DENOM, NO_OP1))).astype(np.int8)
        nu = np.maximum(nu, nu_bg).astype(F32)
        s2 = (two * op2).astype(F32)
    assert op1.dtype == F32 and denom.dtype == F32 and model.dtype == F32
    return nu, s2, code


def state(vel, neighbor_table, c_wale, nu_bg):
    """(nu_eddy, s2, code) [8,8,8,nb] of every cell from a velocity buffer, obstacle cells not masked"""
    return wale_state(gref.gradient_tensor(vel, neighbor_table, F32(1.0)), c_wale, nu_bg)


def fields(vel, neighbor_table, obstacle, c_wale, nu_bg):
    """what ludwig_level_subgrid_fields_download gives: (nu_eddy, code as a float) float32, obstacle cells 0"""
    nu, _, code = state(vel, neighbor_table, c_wale, nu_bg)
    solid = np.asarray(obstacle).astype(bool)
    return (np.asfortranarray(np.where(solid, F32(0), nu).astype(F32)),
            np.asfortranarray(np.where(solid, F32(0), code.astype(F32)).astype(F32)))


def zero_sums(n_blocks):
    return [np.zeros((8, 8, 8, n_blocks), dtype=F64, order="F") for _ in range(3)]


def accumulate(sums, vel, neighbor_table, obstacle, c_wale, nu_bg):
    """one sample into [S_nu, S_nunu, S_eps], in place: the device's sequential Float64 additions (obstacle cells add +0.0)"""
    nu, s2, _ = state(vel, neighbor_table, c_wale, nu_bg)
    solid = np.asarray(obstacle).astype(bool)
    n, e = nu.astype(F64), s2.astype(F64)
    with np.errstate(all="ignore"):
        sums[0] += np.where(solid, 0.0, n)
        sums[1] += np.where(solid, 0.0, n * n)
        sums[2] += np.where(solid, 0.0, n * e)
    return sums
