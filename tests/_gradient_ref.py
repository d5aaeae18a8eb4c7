"""Float32 restatement of the velocity-gradient fields (ludwig_level_gradient_fields_*), for the tests.

The neighbour value is get_velocity_neighbor (reference src/physics_utils.jl:44-67): a face neighbour inside the block directly,
across a block face through neighbor_table[b, dir] (1-based, dir = (ox+1) + 3(oy+1) + 9(oz+1) + 1), and the cell's own value
where that entry is 0. g_ij = (0.5 (u_i(+e_j) - u_i(-e_j))) * scale; vorticity = (g32 - g23, g13 - g31, g21 - g12);
Q = -0.5 (((g11 g11 + g22 g22) + g33 g33) + 2 ((g12 g21 + g13 g31) + g23 g32)); obstacle cells 0. Every operation is one float32
numpy ufunc, in this order, so the result is what the device computes, bit for bit."""
import numpy as np

B = 8
F32 = np.float32


def padded_velocity(vel: np.ndarray, neighbor_table: np.ndarray) -> np.ndarray:
    """vel [8,8,8,nb,3] -> [10,10,10,nb,3]: every block plus a one-cell face halo (edges and corners unused, left 0)"""
    vel = np.asarray(vel, dtype=F32)
    nb = vel.shape[3]
    nt = np.asarray(neighbor_table).reshape(nb, 27).astype(np.int64)
    p = np.zeros((B + 2, B + 2, B + 2, nb, 3), dtype=F32)
    p[1:-1, 1:-1, 1:-1] = vel
    own = np.arange(nb)
    for axis in range(3):
        for up in (False, True):
            o = [0, 0, 0]
            o[axis] = 1 if up else -1
            nbr = nt[:, (o[0] + 1) + 3 * (o[1] + 1) + 9 * (o[2] + 1)]
            src_blk = np.where(nbr > 0, nbr - 1, own)
            # the neighbour's adjacent layer, or (no block there) the block's own edge layer: the own-value rule
            src = np.where(nbr > 0, 0 if up else B - 1, B - 1 if up else 0)
            vals = np.moveaxis(vel, axis, 0)[src, :, :, src_blk, :]      # [nb, 8, 8, 3]
            np.moveaxis(p, axis, 0)[B + 1 if up else 0, 1:-1, 1:-1] = vals.transpose(1, 2, 0, 3)
    return p


def gradient_tensor(vel: np.ndarray, neighbor_table: np.ndarray, scale) -> np.ndarray:
    """g [3,3] of arrays [8,8,8,nb]: g[i][j] = du_i/dx_j as the device evaluates it"""
    p = padded_velocity(vel, neighbor_table)
    s, h = F32(scale), F32(0.5)
    c = slice(1, -1)
    g = [[None] * 3 for _ in range(3)]
    for j in range(3):
        hi = [c, c, c]
        lo = [c, c, c]
        hi[j] = slice(2, None)
        lo[j] = slice(0, -2)
        for i in range(3):
            g[i][j] = (h * (p[tuple(hi) + (slice(None), i)] - p[tuple(lo) + (slice(None), i)])) * s
    return g


def gradient_fields(vel: np.ndarray, neighbor_table: np.ndarray, obstacle: np.ndarray, scale):
    """(vorticity [8,8,8,nb,3], Q [8,8,8,nb]) float32, the device's rule"""
    g = gradient_tensor(vel, neighbor_table, scale)
    (g11, g12, g13), (g21, g22, g23), (g31, g32, g33) = g
    w = np.stack([g32 - g23, g13 - g31, g21 - g12], axis=-1)
    q = F32(-0.5) * (((g11 * g11 + g22 * g22) + g33 * g33) + F32(2.0) * ((g12 * g21 + g13 * g31) + g23 * g32))
    solid = np.asarray(obstacle).astype(bool)
    w = np.where(solid[..., None], F32(0), w).astype(F32)
    q = np.where(solid, F32(0), q).astype(F32)
    return np.asfortranarray(w), np.asfortranarray(q)


def neighbor_value(vel, neighbor_table, x, y, z, b, dx, dy, dz):
    """get_velocity_neighbor (src/physics_utils.jl:44-67) for one cell, 0-based x, y, z, b: the slow, literal form"""
    nt = np.asarray(neighbor_table).reshape(vel.shape[3], 27)
    nx, ny, nz = x + dx, y + dy, z + dz
    if 0 <= nx < B and 0 <= ny < B and 0 <= nz < B:
        return vel[nx, ny, nz, b]
    ox = -1 if nx < 0 else (1 if nx >= B else 0)
    oy = -1 if ny < 0 else (1 if ny >= B else 0)
    oz = -1 if nz < 0 else (1 if nz >= B else 0)
    nbr = int(nt[b, (ox + 1) + 3 * (oy + 1) + 9 * (oz + 1)])
    if nbr > 0:
        return vel[nx % B, ny % B, nz % B, nbr - 1]
    return vel[x, y, z, b]
