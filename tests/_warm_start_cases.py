"""Shared cases and checks of the warm-start tests (host and device)."""
import numpy as np

import _iso_cases as ic
from open_ludwig_amd import cases, warm_start as ws

F32 = np.float32
STATE_FIELDS = ("f", "f_temp", "vel", "vel_temp", "rho")
OLD_FIELDS = ("f_old", "vel_old", "rho_old")


def level_state(g, vel_name="vel"):
    """a FlowState level of a host BlockLevel's own arrays"""
    return dict(block_pointer=g.block_pointer, obstacle=g.obstacle, rho=g.rho, vel=getattr(g, vel_name), dx=g.dx)


def state_of(grids, offset=(0.0, 0.0, 0.0), u_lattice=0.05, step=0):
    return ws.FlowState([level_state(g) for g in grids], offset, u_lattice, step, "test")


def small_tunnel(levels=3, temporal=True, nb=(4, 2, 2)):
    """cases.tunnel_with_sphere on 4 x 2 x 2 level-1 blocks: 16, 96 and 128 blocks on levels 1-3, obstacle cells on every level,
    Bouzidi cells on the finest, a perturbed non-equilibrium start state"""
    return cases.tunnel_with_sphere(nb, levels=levels, temporal=temporal, tau=0.5006)


# ---- the planted source: a 2-level nest with a hole, obstacle cells on block faces and two non-finite cells ----
NEST_ABSENT = (2, 2, 2)
NEST_FINE = ((2, 2, 2), (3, 2, 2))                 # fine blocks: coarse cells 4..11 x 4..7 x 4..7, across the coarse blocks (1,1,1) | (2,1,1)


def planted_nest():
    """source levels (streamlines.host_levels tuples) of a 2 x 2 x 2-block coarse level without block (2, 2, 2) and a 2-block fine patch
    across the x face between the coarse blocks (1, 1, 1) and (2, 1, 1); smooth rho and u; obstacle cells on block faces of both levels;
    one NaN velocity on the coarse level and one +Inf density on the fine one"""
    coarse = [c for c in cases.full_box_coords(2, 2, 2) if c != NEST_ABSENT]
    g1 = cases.make_level(1, coarse, (2, 2, 2), 0.6)
    g2 = cases.make_level(2, list(NEST_FINE), (4, 4, 4), 0.55)
    out = []
    for g, s in ((g1, 1.0), (g2, 0.5)):
        x = ic.cell_centres(sorted(g.active_block_coords)) * s
        rho = np.asfortranarray((1.0 + 0.01 * np.cos(0.2 * x[..., 0] + 0.1 * x[..., 1] * x[..., 2])).astype(F32))
        vel = np.asfortranarray(np.stack([0.04 + 0.01 * np.sin(0.3 * x[..., 1]), 0.008 * np.cos(0.4 * x[..., 2] + 0.1 * x[..., 0]),
                                          0.002 * np.sin(0.5 * x[..., 0])], axis=-1).astype(F32))
        out.append([g, rho, vel])
    b = {tuple(c): i for i, c in enumerate(g1.active_block_coords)}
    g1.obstacle[7, 2:5, 1:4, b[(1, 1, 1)]] = True                # on the +x face of (1, 1, 1), below the fine patch
    g1.obstacle[0, 3, 5, b[(2, 1, 2)]] = True                    # on the -x face of (2, 1, 2)
    g1.obstacle[3:6, 7, 6, b[(1, 1, 2)]] = True                  # on the +y face of (1, 1, 2)
    g2.obstacle[7, 3:5, 2:4, 0] = True                           # on the face between the two fine blocks
    g2.obstacle[2, 0, 5, 1] = True                               # on the patch's outer -y face
    out[0][2][5, 2, 3, b[(1, 2, 1)], 1] = np.nan
    out[1][1][4, 5, 6, 1] = np.inf
    return [(np.asarray(g.block_pointer), np.asarray(g.obstacle).astype(bool), rho, vel) for g, rho, vel in out]


NEST_SCALE = 0.5
NEST_FALLBACK = (1.0, 0.0125, 0.0, 0.0)
NEST_B = (-3.1, 2.3, 1.7)


def nest_map(level_index):
    """a = 0.75 2^-li (non-dyadic: the weights are no multiples of a power of two) and a shift that puts the 32 x 16 x 16-cell
    tunnel (24 x 12 x 12 source cells) across the source's 16^3 cells: out of it on both x ends, over the absent block, across the
    fine patch's edge and over the obstacle cells"""
    a = 0.75 * 2.0 ** -level_index
    return np.array([a, a, a, *NEST_B], F32)


def upload_result(dev_level, res, temporal):
    """what ludwig_level_init_from_source writes, through ludwig_level_upload"""
    for name in STATE_FIELDS + (OLD_FIELDS if temporal else ()):
        dev_level.upload(name, res[name.split("_")[0]])


def assert_level_equals(dev_level, res, temporal, what=""):
    """every array the call writes equals init_host's, bit for bit"""
    for name in STATE_FIELDS + (OLD_FIELDS if temporal else ()):
        got, want = dev_level.download(name), np.asfortranarray(res[name.split("_")[0]])
        assert got.dtype == want.dtype == F32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what} {name}: {int((got != want).sum())} of {got.size} differ"
