"""The levels the wall-diagnostics tests share: the 16-block wall-modelled tunnel after 3 and 4 steps (both velocity buffers), the
2-level tunnel, and the wall-model entries of tests/_edge_states.py after their own step counts. Each case is (name, grids, params,
steps, u)."""
from __future__ import annotations

import dataclasses

import numpy as np

from open_ludwig_amd import cases
import _edge_states as es

F32 = np.float32
U = F32(0.05)


def tunnel(steps: int):
    grids, params = cases.tunnel_with_sphere((4, 2, 2), tau=0.5003, levels=1, wall_model=True, inlet_turbulence=0.0)
    return (f"tunnel16_{steps}steps", grids, params, steps, U)


def tunnel_two_levels(steps: int = 3):
    grids, params = cases.tunnel_with_sphere((5, 3, 4), tau=0.5003, levels=2, wall_model=True, inlet_turbulence=0.0)
    return (f"tunnel2level_{steps}steps", grids, params, steps, U)


def edge_entries():
    """the three wall-model entries after their own step counts, and - for the near-wall cells the model skips, which those leave empty -
    wall_umag_edges after ONE step (its two cells then hold |u| = 1e-6 exactly and one ulp more: either side of `u_mag > 1e-6`) and
    wall_model_tau_half (nu_visc = 0: every near-wall cell is skipped)"""
    entries = [es.wall_umag_edges(), es.wall_y_plus_edges(), es.wall_distance_edges(),
               dataclasses.replace(es.wall_umag_edges(), name="wall_umag_edges_1step", steps=1), es.wall_model_tau_half()]
    return [(e.name, e.grids, e.params, e.steps, F32(e.u)) for e in entries]


def single_level_cases():
    return [tunnel(3), tunnel(4)] + edge_entries()


def vel_name(level_index: int, t_coarse: int) -> str:
    """the buffer a level's last sub-step of coarse step t_coarse wrote"""
    from open_ludwig_amd.statistics import t_sub_after
    return "vel_temp" if t_sub_after(level_index, t_coarse) % 2 == 0 else "vel"
