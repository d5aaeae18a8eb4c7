"""Inputs of the subgrid observer's tests, shared by tests/test_subgrid_host.py (does every branch code occur?) and
tests/test_gpu_subgrid.py (the device against tests/_subgrid_ref.py on the same inputs).

Uploaded boxes: non-periodic level-1 block sets whose velocity buffer is planted, not stepped to. The recipe for the codes is that of
tests/_edge_states.py (wale_branches): a uniform flow gives OP1 = 0 (code 0), cells whose neighbours carry gradients of about 3e-3
give OP1 > 1e-12 with denom <= 1e-12 (code 1), gradients of about 3e-2 evaluate the model (code 3 with the default background
viscosity), and a nu_sgs_background above the model's value makes the floor win there (code 2)."""
import dataclasses

import numpy as np

from open_ludwig_amd import cases

F32 = np.float32
# name -> (block coordinates, grid dimensions, nu_sgs_background or None for the builder's 0.0005)
BOXES = {
    "one_block": ([(1, 1, 1)], (1, 1, 1), None),                                 # every face is missing
    "three_in_an_L": ([(1, 1, 1), (2, 1, 1), (1, 2, 1)], (2, 2, 1), 0.05),       # present and missing faces mixed; the floor wins
    "box27": (cases.full_box_coords(3, 3, 3), (3, 3, 3), None),                  # block (2, 2, 2) is fully interior
}
# amplitudes of the planted patches: (first x of the patch, amplitude)
PATCHES = ((0, 3e-3), (3, 3e-2), (6, 1e-2))


def uploaded_box(name):
    """(grids, params, vel [8,8,8,nb,3] to upload into both velocity buffers). The level is at rest with obstacle cells on block faces."""
    coords, dims, nu_bg = BOXES[name]
    level = cases.make_level(1, coords, dims, 0.5006, temporal=False)
    cases.set_state(level, F32(1.0), F32(0.0), F32(0.0), F32(0.0))
    nb = level.n_blocks
    level.obstacle[0, 5:7, 5:7, 0] = True                    # on the -x face, the +x face and a +y / +z edge of blocks
    level.obstacle[7, 6, 1:3, nb - 1] = True
    level.obstacle[2:4, 7, 7, nb // 2] = True
    params = cases.SolverParams(domain_nx=8 * dims[0], domain_ny=8 * dims[1], domain_nz=8 * dims[2], wall_model_active=False, c_wale=0.5,
                                nu_sgs_bg=0.0005 if nu_bg is None else nu_bg, inlet_turbulence=0.0, use_temporal_interp=False,
                                sponge_blend_dist=False)
    rng = np.random.default_rng(29 + nb)
    vel = np.zeros((8, 8, 8, nb, 3), dtype=F32, order="F")
    vel[..., 0] = F32(0.03)                                   # uniform: code 0
    for b in range(nb):
        for x0, amp in PATCHES:                               # patches that reach over the block's faces in y and z
            vel[x0:x0 + 2, :, 2 * (b % 3):2 * (b % 3) + 3, b, :] += (amp * rng.uniform(-1, 1, (2, 8, 3, 3))).astype(F32)
    b = nb // 2                                               # the interior block of box27
    vel[4, 0, 6, b, 1] = np.nan                               # non-finite velocities, one of each, on and off block faces
    vel[7, 4, 7, b, 0] = np.inf
    vel[2, 3, 0, nb - 1, 2] = -np.inf
    return [level], params, vel


def with_background(params, nu_bg):
    return dataclasses.replace(params, nu_sgs_bg=nu_bg)
