"""A plain numpy restatement of ONE coarse step, written from the reference's Julia alone (test infrastructure).

Independent of oracle/ludwig_oracle.c and of the HIP kernels: another structure (whole-level array operations instead of a loop
over cells), another operand order (numpy's pairwise sums and matrix products for the moments), ordinary `np.power` / `np.log`,
and a working float type that is a parameter - float64 for reference values, float32 to calibrate how much float32 rounding of
this very operation moves the result (`e_ref`, below). It never writes to its inputs.

What it restates (file:line of the reference):
  src/solver_control.jl:21-165      recursion, A/B parity of t_sub, copy_to_old! before a level with children steps, children at
                                    2 t_sub (weight 0) and 2 t_sub + 1 (weight 0.5)
  src/physics_v2.jl:26-97           per-level call: global extent nx * 2^(level-1), seed t_sub % 10^6, post-collision store, Bouzidi
  src/physics_kernels.jl:62-149     pull through the neighbour table; edge conditions in the written priority: inlet (with
                                    gradient_noise), outlet, y mirror (symmetric or not: the same statement), z mirror, interface, w_k
  src/physics_kernels.jl:154-166    obstacle bounce-back
  src/physics_kernels.jl:172-199    rho clamp, sponge (moments, optionally populations)
  src/physics_kernels.jl:206-236    wall-model force
  src/physics_kernels.jl:251-300    WALE from the previous sub-step's velocity (own value where a neighbour is missing), omega floor
  src/physics_kernels.jl:305-354    regularised collision with the force term
  src/physics_interpolation.jl      coarse -> fine: temporal blend, invalid corners, trilinear, rescaling of f_neq by the tau ratio
  src/physics_utils.jl:17-28, 45-83 noise hash, velocity neighbours
  src/bouzidi_kernel.jl:29-91       Bouzidi correction: q range, q < 1/2 with the cell behind (own value if missing), q >= 1/2

Constants and literals keep their Float32 VALUES (0.01f0, KAPPA = 0.41f0, CS2 = 1f0/3f0, the lattice weights ...): they are part of
the operation's definition, not of its rounding. Arithmetic on them happens in the working type.

Tolerances (measured; see tests/test_step_reference_host.py and DESIGN.md section 5)
-----------------------------------------------------------------------------------
e_ref = |ref32 - ref64| / scale with scale = w_k max(rho, 1) for populations, max(|u|_inf of the step, u_inlet, 1e-3) for the
velocity and 1 for rho: float32 rounding of this operation in a different operand order, independent of the code under test.
MAX_E_REF is its maximum over the case table of tests/_step_ref_cases.py; the asserted bound for oracle-vs-ref64 and
HIP-vs-ref64 is MARGIN * MAX_E_REF per field class. The constants come from the host run named in DESIGN.md section 5.
"""
from __future__ import annotations

import weakref
from typing import Dict, List, Optional

import numpy as np

B = 8                                            # src/blocks.jl:14

# ---- branch record: one uint16 per cell and sub-step --------------------------------------------------------------------------
RHO_CLAMP = 1 << 0        # sum of the pulled populations below 0.01
SPONGE = 1 << 1           # sp > 0
WM_DIST = 1 << 2          # 0 < wall distance < 10
WM_UMAG = 1 << 3          # |u| > 1e-6 and nu > 1e-10
WM_YPLUS = 1 << 4         # y+ > 11.81
WM_LAW = 1 << 5           # u+ of the log law > 0.1
WM_FORCE = 1 << 6         # tau_wall > tau_res
WALE_OP1 = 1 << 7         # OP1 > 1e-12
WALE_DENOM = 1 << 8       # denom > 1e-12
WALE_EDDY = 1 << 9        # nu_eddy above the background value
OMEGA_FLOOR = 1 << 10     # tau_turb below 0.500001
BZ_IN_RANGE = 1 << 11     # a listed cell with a link q_min < q <= 1
BZ_OUT_OF_RANGE = 1 << 12 # a listed cell with a link 0 < q <= q_min or q > 1 (left alone)
BZ_LT_HALF = 1 << 13      # a corrected link with q < 1/2
BZ_GE_HALF = 1 << 14      # a corrected link with q >= 1/2
BZ_NO_BEHIND = 1 << 15    # a q < 1/2 link whose cell behind lies in a missing block (own value used)
BRANCH_NAMES = {RHO_CLAMP: "rho_clamp", SPONGE: "sponge", WM_DIST: "wm_dist", WM_UMAG: "wm_umag", WM_YPLUS: "wm_yplus", WM_LAW: "wm_law",
                WM_FORCE: "wm_force", WALE_OP1: "wale_op1", WALE_DENOM: "wale_denom", WALE_EDDY: "wale_eddy", OMEGA_FLOOR: "omega_floor",
                BZ_IN_RANGE: "bz_in_range", BZ_OUT_OF_RANGE: "bz_out_of_range", BZ_LT_HALF: "bz_lt_half", BZ_GE_HALF: "bz_ge_half",
                BZ_NO_BEHIND: "bz_no_behind"}

# ---- measured tolerances (CPU host run of tests/test_step_reference_host.py, printed by its census test) ----
# measured max e_ref over the table: f 2.091e-06, vel 2.125e-06, rho 4.332e-07; recorded with < 10 % on top, since numpy's pairwise
# sums group differently from one CPU's vector width to another's
MAX_E_REF = {"f": 2.3e-6, "vel": 2.3e-6, "rho": 4.7e-7}
# the oracle's own max error against ref64, same scales and cells: about 0.25 of the bound, so the margin stays at 4
ORACLE_MAX_ERR = {"f": 2.273e-6, "vel": 2.398e-6, "rho": 4.769e-7}
MARGIN = 4.0                                              # n-ary sums of 27 terms in another association
NORTH_STAR = 1e-5                                         # BASELINE.json: rho, u within 1e-5 relative
MAX_EXCLUDED_SHARE = 0.005                                # per case and level, of that level's fluid cells


def bound(kind: str) -> float:
    return MARGIN * MAX_E_REF[kind]


# ---- lattice (src/physics_v2.jl:99-117), 0-based tables -------------------------------------------------------------------------
def _lattice():
    c = np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], dtype=np.int64)
    d2 = (c * c).sum(axis=1)
    num = np.where(d2 == 0, 8, np.where(d2 == 1, 2, 1)).astype(np.float32)
    den = np.where(d2 <= 1, 27, np.where(d2 == 2, 54, 216)).astype(np.float32)
    w = num / den                                                              # Float32 quotients, as the reference builds them
    find = lambda s: np.array([int(np.nonzero((c == c[i] * s).all(axis=1))[0][0]) for i in range(27)])
    return c, w, find(np.array([-1, -1, -1])), find(np.array([1, -1, 1])), find(np.array([1, 1, -1]))


C_K, W32, OPP, MIRROR_Y, MIRROR_Z = _lattice()

_PRESENT, _INLET, _OUTLET, _YMIR, _ZMIR, _IFACE, _WEIGHT = range(7)


def gradient_noise(a, b, c, seed):
    """src/physics_utils.jl:17-28 on integer arrays: Int32 wrap-around products, then the three-round hash, 16 low bits -> [-1, 1)"""
    M = np.uint64(0xFFFFFFFF)
    a, b, c = (np.asarray(v, dtype=np.int64) for v in (a, b, c))
    h = ((a * 374761393 + b * 668265263 + c * 1274126177 + int(seed)) & 0xFFFFFFFF).astype(np.uint64)
    h = ((h ^ (h >> np.uint64(16))) * np.uint64(0x85EBCA6B)) & M
    h = ((h ^ (h >> np.uint64(13))) * np.uint64(0xC2B2AE35)) & M
    h = h ^ (h >> np.uint64(16))
    return (h & np.uint64(0xFFFF)).astype(np.float64) / 32768.0 - 1.0             # exact in Float32 as well


class _Geom:
    """Static addressing of one level: where cell + d lives, and what stands in for a missing pull source."""

    def __init__(self, level, params):
        self.nb = nb = level.n_blocks
        self.scale = 1 << (level.level_id - 1)
        self.n_glob = tuple(int(n) * self.scale for n in (params.domain_nx, params.domain_ny, params.domain_nz))
        self.table = np.asarray(level.neighbor_table).astype(np.int64) - 1           # -1 = missing
        loc = np.arange(B)
        self.lx, self.ly, self.lz = loc[:, None, None, None], loc[None, :, None, None], loc[None, None, :, None]
        self.blk = np.arange(nb)[None, None, None, :]
        m = [np.asarray(a).astype(np.int64)[None, None, None, :] for a in (level.map_x, level.map_y, level.map_z)]
        self.g = [(m[0] - 1) * B + self.lx + 1, (m[1] - 1) * B + self.ly + 1, (m[2] - 1) * B + self.lz + 1]   # 1-based global
        self.first_level = level.level_id == 1
        self._nbr: Dict[tuple, tuple] = {}
        self._code: Dict[int, np.ndarray] = {}

    def neighbour(self, d):
        """(ix, iy, iz, block, present) of cell + d; block is 0 where absent"""
        d = tuple(int(v) for v in d)
        if d not in self._nbr:
            n = [self.lx + d[0], self.ly + d[1], self.lz + d[2]]
            off = [np.where(v < 0, -1, np.where(v >= B, 1, 0)) for v in n]
            direction = (off[0] + 1) + 3 * (off[1] + 1) + 9 * (off[2] + 1)
            inside = direction == 13
            blk = np.where(inside, self.blk, self.table[self.blk, direction])
            blk = np.broadcast_to(blk, (B, B, B, self.nb))
            present = blk >= 0
            self._nbr[d] = (n[0] % B, n[1] % B, n[2] % B, np.where(present, blk, 0).astype(np.int32), present)
        return self._nbr[d]

    def code(self, k):
        """what population k of each cell is pulled from (src/physics_kernels.jl:92-140, in that priority)"""
        if k not in self._code:
            present = self.neighbour(-C_K[k])[4]
            s = [np.broadcast_to(self.g[a] - C_K[k][a], present.shape) for a in range(3)]
            y_out = (s[1] < 1) | (s[1] > self.n_glob[1])
            z_out = (s[2] < 1) | (s[2] > self.n_glob[2])
            code = np.select([present, s[0] < 1, s[0] > self.n_glob[0], y_out, z_out],
                             [_PRESENT, _INLET, _OUTLET, _YMIR, _ZMIR], _WEIGHT if self.first_level else _IFACE)
            self._code[k] = code.astype(np.int8)
        return self._code[k]


_geoms: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def geometry(level, params) -> _Geom:
    per = _geoms.setdefault(level, {})
    key = (params.domain_nx, params.domain_ny, params.domain_nz, level.n_blocks)
    if key not in per:
        per[key] = _Geom(level, params)
    return per[key]


def _equilibrium(T, rho, ux, uy, uz, k):
    c = C_K[k]
    cu = T(c[0]) * ux + T(c[1]) * uy + T(c[2]) * uz
    return rho * T(W32[k]) * (T(1) + T(3) * cu + T(4.5) * cu * cu - T(1.5) * (ux * ux + uy * uy + uz * uz))


class _Parent:
    def __init__(self, level, st, f_name, vel_name):
        self.ptr = np.asarray(level.block_pointer).astype(np.int64)
        self.tau = level.tau
        self.new = (st[f_name], st["rho"], st[vel_name])
        self.old = (st["f_old"], st["rho_old"], st["vel_old"])


def _interpolate(T, geom, parent, k, cells, tau_fine, weight, temporal):
    """src/physics_interpolation.jl:16-138 for population k at the listed cells (index arrays x, y, z, b)"""
    x, y, z, b = cells
    src = [np.broadcast_to(geom.g[a], (B, B, B, geom.nb))[x, y, z, b] - C_K[k][a] for a in range(3)]
    cont = [(s.astype(T) - T(0.5)) * T(0.5) for s in src]
    lo = [np.floor(c).astype(np.int64) for c in cont]
    frac = [c - l.astype(T) for c, l in zip(cont, lo)]
    hi = [l + 1 for l in lo]
    lo = [np.maximum(1, l) for l in lo]
    blend = bool(temporal) and np.float32(weight) < np.float32(0.99)
    tw = T(np.float32(weight))
    dims = parent.ptr.shape

    def corner(px, py, pz):
        p = (px, py, pz)
        pb = [(v - 1) // B + 1 for v in p]                        # v >= 1 here: truncation and floor agree
        ok = np.ones(px.shape, dtype=bool)
        for a in range(3):
            ok &= (pb[a] >= 1) & (pb[a] <= dims[a])
        idx = np.where(ok, parent.ptr[tuple(np.clip(pb[a], 1, dims[a]) - 1 for a in range(3))], 0)
        ok &= idx > 0
        idx = np.where(ok, idx - 1, 0)
        l = [(v - 1) % B for v in p]
        f_new, rho_new, vel_new = parent.new
        vals = [f_new[l[0], l[1], l[2], idx, k], rho_new[l[0], l[1], l[2], idx]] + [vel_new[l[0], l[1], l[2], idx, a] for a in range(3)]
        if blend:
            f_old, rho_old, vel_old = parent.old
            olds = [f_old[l[0], l[1], l[2], idx, k], rho_old[l[0], l[1], l[2], idx]] + [vel_old[l[0], l[1], l[2], idx, a] for a in range(3)]
            vals = [o * (T(1) - tw) + n * tw for o, n in zip(olds, vals)]
        fill = [T(W32[k]), T(1), T(0), T(0), T(0)]
        return [np.where(ok, v, fv) for v, fv in zip(vals, fill)], ok

    assert all((l >= 1).all() for l in lo)
    base, _ = corner(lo[0], lo[1], lo[2])
    v = {}
    for i in (0, 1):
        for j in (0, 1):
            for m in (0, 1):
                if (i, j, m) == (0, 0, 0):
                    v[i, j, m] = base
                    continue
                vals, ok = corner(hi[0] if i else lo[0], hi[1] if j else lo[1], hi[2] if m else lo[2])
                v[i, j, m] = [np.where(ok, a, b0) for a, b0 in zip(vals, base)]
    wx, wy, wz = frac
    out = []
    for q in range(5):
        c00 = v[0, 0, 0][q] * (T(1) - wx) + v[1, 0, 0][q] * wx
        c01 = v[0, 0, 1][q] * (T(1) - wx) + v[1, 0, 1][q] * wx
        c10 = v[0, 1, 0][q] * (T(1) - wx) + v[1, 1, 0][q] * wx
        c11 = v[0, 1, 1][q] * (T(1) - wx) + v[1, 1, 1][q] * wx
        c0 = c00 * (T(1) - wy) + c10 * wy
        c1 = c01 * (T(1) - wy) + c11 * wy
        out.append(c0 * (T(1) - wz) + c1 * wz)
    f_int, rho_int, ux, uy, uz = out
    feq = _equilibrium(T, rho_int, ux, uy, uz, k)
    tau_c = T(np.float32(parent.tau)) - T(0.5)
    tau_f = T(np.float32(tau_fine)) - T(0.5)
    ratio = min(max(tau_f / tau_c, T(np.float32(0.01))), T(100)) if tau_c > T(np.float32(1e-6)) else T(1)
    return feq + (f_int - feq) * ratio


def _interface_parent_cells(geom, k, cells, dims, ptr):
    """flat parent cell indices (x, y, z, b) the interpolation of population k at `cells` may read (all 8 corners), for the taint pass"""
    x, y, z, b = cells
    src = [np.broadcast_to(geom.g[a], (B, B, B, geom.nb))[x, y, z, b] - C_K[k][a] for a in range(3)]
    lo = [np.floor((s - 0.5) * 0.5).astype(np.int64) for s in src]
    hi = [l + 1 for l in lo]
    lo = [np.maximum(1, l) for l in lo]
    out = []
    for i in (0, 1):
        for j in (0, 1):
            for m in (0, 1):
                p = (hi[0] if i else lo[0], hi[1] if j else lo[1], hi[2] if m else lo[2])
                pb = [(v - 1) // B + 1 for v in p]
                ok = np.ones(p[0].shape, dtype=bool)
                for a in range(3):
                    ok &= (pb[a] >= 1) & (pb[a] <= dims[a])
                idx = np.where(ok, ptr[tuple(np.clip(pb[a], 1, dims[a]) - 1 for a in range(3))], 0)
                ok &= idx > 0
                out.append(((p[0] - 1) % B, (p[1] - 1) % B, (p[2] - 1) % B, np.where(ok, idx - 1, 0), ok))
    return out


def bouzidi_arm(T, level, geom, params, post, f_out, br=None):
    """apply_bouzidi_correction! (src/bouzidi_kernel.jl:29-91) in the working type T: corrects f_out in place from the post-collision
    state `post`, ORs the branch bits into br (if given) and returns the cells whose post-collision state was read. The one statement of
    the arm: _level_step calls it, and so does the device test of the correction alone (tests/test_gpu_setup_reference.py)."""
    shape = post.shape[:4]
    if br is None:
        br = np.zeros(shape, dtype=np.uint16)
    cb = np.asarray(level.bouzidi_cell_block).astype(np.int64) - 1
    x, y, z = (np.asarray(a).astype(np.int64) - 1 for a in (level.bouzidi_cell_x, level.bouzidi_cell_y, level.bouzidi_cell_z))
    q_min = np.float32(params.q_min_threshold)
    q_all = np.asarray(level.bouzidi_q_map)[x, y, z, cb, :].astype(np.float32)
    read = np.zeros(shape, dtype=bool)
    for k in range(27):
        q32 = q_all[:, k]
        ok = (q32 > q_min) & (q32 <= np.float32(1))
        br[x, y, z, cb] |= np.where(ok, np.uint16(BZ_IN_RANGE), np.uint16(0))
        br[x, y, z, cb] |= np.where(~ok & (q32 != 0), np.uint16(BZ_OUT_OF_RANGE), np.uint16(0))
        if not ok.any():
            continue
        xs, ys, zs, bs, q = x[ok], y[ok], z[ok], cb[ok], q32[ok].astype(T)
        f_k = post[xs, ys, zs, bs, k]
        read[xs, ys, zs, bs] = True
        ix, iy, iz, blk, present = geom.neighbour(C_K[OPP[k]])
        ix, iy, iz = (np.broadcast_to(a, shape)[xs, ys, zs, bs] for a in (ix, iy, iz))
        blk, present = blk[xs, ys, zs, bs], present[xs, ys, zs, bs]
        low = q < T(0.5)
        behind = np.where(present, post[ix, iy, iz, blk, k], f_k)
        read[ix[low & present], iy[low & present], iz[low & present], blk[low & present]] = True
        near_wall = T(2) * q * f_k + (T(1) - T(2) * q) * behind
        inv = T(1) / (T(2) * q)
        far_wall = inv * f_k + (T(2) * q - T(1)) * inv * post[xs, ys, zs, bs, OPP[k]]
        f_out[xs, ys, zs, bs, OPP[k]] = np.where(low, near_wall, far_wall)
        br[xs, ys, zs, bs] |= np.where(low, np.uint16(BZ_LT_HALF), np.uint16(BZ_GE_HALF))
        br[xs, ys, zs, bs] |= np.where(low & ~present, np.uint16(BZ_NO_BEHIND), np.uint16(0))
    return read


def _level_step(T, level, geom, st, f_in_name, f_out_name, vel_in_name, vel_out_name, parent: Optional[_Parent], t_sub, weight, u_curr, params):
    """perform_timestep_v2! for one level: stream-collide, then Bouzidi. Returns the branch record [8,8,8,nb] uint16."""
    nb = level.n_blocks
    shape = (B, B, B, nb)
    f_in, vel_in = st[f_in_name], st[vel_in_name]
    u_in = T(np.float32(u_curr))
    w = W32.astype(T)
    cf = C_K.astype(T)
    store_post = bool(level.bouzidi_enabled) and level.n_boundary_cells > 0
    turb = np.float32(params.inlet_turbulence)
    if turb > 0:
        seed = int(t_sub) % 1000000
        noise = gradient_noise(np.broadcast_to(geom.g[1], shape), np.broadcast_to(geom.g[2], shape), seed, 1234).astype(T)
        u_inst = u_in + noise * T(turb) * u_in
    else:
        u_inst = np.full(shape, u_in, dtype=T)

    # ---- pull ----
    pulled = np.empty(shape + (27,), dtype=T)
    for k in range(27):
        ix, iy, iz, blk, present = geom.neighbour(-C_K[k])
        val = f_in[ix, iy, iz, blk, k]
        if not present.all():
            code = geom.code(k)
            cu = cf[k, 0] * u_inst
            inlet = w[k] * (T(1) + T(3) * cu + T(4.5) * cu * cu - T(1.5) * u_inst * u_inst)
            cu_o = cf[k, 0] * u_in
            outlet = w[k] * (T(1) + T(3) * cu_o + T(4.5) * cu_o * cu_o - T(1.5) * u_in * u_in)
            val = np.select([code == _PRESENT, code == _INLET, code == _OUTLET, code == _YMIR, code == _ZMIR],
                            [val, inlet, outlet, f_in[..., MIRROR_Y[k]], f_in[..., MIRROR_Z[k]]], w[k])
            cells = np.nonzero(code == _IFACE)
            if cells[0].size:
                assert parent is not None
                val[cells] = _interpolate(T, geom, parent, k, cells, level.tau, weight, params.use_temporal_interp)
        pulled[..., k] = val

    with np.errstate(all="ignore"):
        rho_sum = pulled.sum(axis=-1)
        j = pulled @ cf                                                  # [..., 3]
        br = np.zeros(shape, dtype=np.uint16)

        def flag(cond, bit):
            br[...] |= np.where(cond, np.uint16(bit), np.uint16(0))

        flag(rho_sum < T(np.float32(0.01)), RHO_CLAMP)
        rho = np.maximum(rho_sum, T(np.float32(0.01)))
        inv_rho = T(1) / rho
        u = j * inv_rho[..., None]
        sp = np.asarray(level.sponge).astype(T)
        in_sponge = sp > 0
        flag(in_sponge, SPONGE)
        keep = T(1) - sp
        rho = np.where(in_sponge, rho * keep + sp, rho)
        u_target = np.zeros(3, dtype=T)
        u_target[0] = u_in
        u = np.where(in_sponge[..., None], u * keep[..., None] + u_target * sp[..., None], u)
        if params.sponge_blend_dist:
            feq_t = np.stack([_equilibrium(T, T(1), u_in, T(0), T(0), k) for k in range(27)]).astype(T)
            blended = np.where(in_sponge[..., None], pulled * keep[..., None] + feq_t * sp[..., None], pulled)
        else:
            blended = pulled

        # ---- wall-model force ----
        force = np.zeros(shape + (3,), dtype=T)
        if params.wall_model_active:
            d = np.asarray(level.wall_dist).astype(T)
            near = (d > 0) & (d < T(10))
            flag(near, WM_DIST)
            u_mag = np.sqrt((u * u).sum(axis=-1))
            nu = (T(np.float32(level.tau)) - T(0.5)) / T(3)
            moving = near & (u_mag > T(np.float32(1e-6))) & (nu > T(np.float32(1e-10)))
            flag(moving, WM_UMAG)
            power_law = u_mag * np.power(nu / (d * u_mag + T(np.float32(1e-10))), T(1) / T(7)) * np.power(T(2) * T(np.float32(8.3)), -T(1) / T(7))
            u_tau = np.maximum(power_law, T(np.float32(1e-6)))
            y_plus = u_tau * d / nu
            outer = moving & (y_plus > T(np.float32(11.81)))
            flag(outer, WM_YPLUS)
            law = (T(1) / T(np.float32(0.41))) * np.log(y_plus) + T(np.float32(5.2))
            use_law = outer & (law > T(np.float32(0.1)))
            flag(use_law, WM_LAW)
            u_tau = np.where(use_law, np.maximum(u_tau * ((u_mag / u_tau) / law), T(np.float32(1e-6))), u_tau)
            tau_wall = rho * u_tau * u_tau
            tau_res = rho * nu * (u_mag / d)
            push = moving & (tau_wall > tau_res)
            flag(push, WM_FORCE)
            mag = (tau_wall - tau_res) / d
            force = np.where(push[..., None], -mag[..., None] * u / u_mag[..., None], T(0)).astype(T)
        u_eq = u + T(0.5) * force * inv_rho[..., None]          # inv_rho of the clamped sum, before the sponge (as written)
        usq_eq = (u_eq * u_eq).sum(axis=-1)

        # ---- WALE ----
        grad = np.empty(shape + (3, 3), dtype=T)                    # grad[..., i, j] = d u_i / d x_j
        for axis in range(3):
            d = np.zeros(3, dtype=np.int64)
            d[axis] = 1
            sides = []
            for sgn in (1, -1):
                ix, iy, iz, blk, present = geom.neighbour(sgn * d)
                v = vel_in[ix, iy, iz, blk, :]
                sides.append(np.where(present[..., None], v, vel_in))
            grad[..., :, axis] = T(0.5) * (sides[0] - sides[1])
        gsq = grad @ grad
        tr = (gsq[..., 0, 0] + gsq[..., 1, 1] + gsq[..., 2, 2]) / T(3)
        sd = T(0.5) * (gsq + np.swapaxes(gsq, -1, -2))
        for a in range(3):
            sd[..., a, a] = gsq[..., a, a] - tr
        strain = T(0.5) * (grad + np.swapaxes(grad, -1, -2))
        op1 = (sd * sd).sum(axis=(-1, -2))
        op2 = (strain * strain).sum(axis=(-1, -2))
        tiny = T(np.float32(1e-12))
        big1 = op1 > tiny
        flag(big1, WALE_OP1)
        denom = op2 * op2 * np.sqrt(np.maximum(op2, tiny)) + op1 * np.sqrt(np.sqrt(np.maximum(op1, tiny)))
        big2 = big1 & (denom > tiny)
        flag(big2, WALE_DENOM)
        c_w = T(np.float32(params.c_wale))
        nu_eddy = np.where(big2, (c_w * c_w) * (op1 * np.sqrt(op1)) / denom, T(0))
        bg = T(np.float32(params.nu_sgs_bg))
        flag(nu_eddy > bg, WALE_EDDY)
        nu_eddy = np.maximum(nu_eddy, bg)
        tau_turb = T(np.float32(level.tau)) + nu_eddy * T(3)
        floor = T(np.float32(0.500001))
        flag(tau_turb < floor, OMEGA_FLOOR)
        omega = T(1) / np.maximum(tau_turb, floor)

        # ---- regularised collision ----
        cu = u_eq @ cf.T                                                  # [..., 27]
        feq = rho[..., None] * w * (T(1) + T(3) * cu + T(4.5) * cu * cu - T(1.5) * usq_eq[..., None])
        fneq = blended - feq
        cc = cf[:, :, None] * cf[:, None, :]                              # [27, 3, 3]
        pi = np.einsum("...k,kij->...ij", fneq, cc)
        q_t = cc - T(np.float32(1.0) / np.float32(3.0)) * np.eye(3, dtype=T)
        reg = w * T(4.5) * np.einsum("...ij,kij->...k", pi, q_t)
        # force term: the bare u in (c - u), u_eq inside cu
        c_dot_f = force @ cf.T
        f_term = w * T(3) * (c_dot_f * (T(1) + T(3) * cu) - (u * force).sum(axis=-1)[..., None])
        coll = feq + (T(1) - omega)[..., None] * reg + (T(1) - T(0.5) * omega)[..., None] * f_term

        obs = np.asarray(level.obstacle).astype(bool)
        out = np.where(obs[..., None], pulled[..., OPP], coll).astype(T)
        br[obs] = 0
        st[f_out_name] = out
        st[vel_out_name] = np.where(obs[..., None], T(0), u).astype(T)
        st["rho"] = np.where(obs, T(1), rho).astype(T)
        if store_post:
            st["f_post_collision"] = out.copy()

    # ---- Bouzidi ----
    if store_post:
        st["post_read"] = bouzidi_arm(T, level, geom, params, st["f_post_collision"], st[f_out_name], br)
    return br


# ---- the coarse step (src/solver_control.jl) ------------------------------------------------------------------------------------
_STATE = ("f", "f_temp", "vel", "vel_temp", "rho", "f_old", "rho_old", "vel_old")


def _buffers(t_sub):
    """iseven(t_sub): read f / vel, write f_temp / vel_temp; else the other way round"""
    return ("f", "f_temp", "vel", "vel_temp") if t_sub % 2 == 0 else ("f_temp", "f", "vel_temp", "vel")


class LevelResult:
    """New state of one level after the coarse step, in the working type.
    f / vel: the buffers written last (named f_name / vel_name), rho, f_post_collision and post_read (the cells where the Bouzidi
    pass read it; None without Bouzidi), old = (f_old, rho_old, vel_old) as saved last (None for a level without children or
    without temporal storage), branches = one uint16 record per sub-step of this level."""

    def __init__(self):
        self.f_name = self.vel_name = None
        self.f = self.vel = self.rho = self.f_post_collision = self.post_read = self.old = None
        self.branches: List[np.ndarray] = []


def coarse_step(grids, params, t: int, u_curr, dtype=np.float64) -> List[LevelResult]:
    """One pass of the loop body of execute_timestep_batch! at coarse step t over host BlockLevels. Inputs are left untouched."""
    T = np.dtype(dtype).type
    n = len(grids)
    states = [{name: np.asarray(getattr(g, name)).astype(T) for name in _STATE} for g in grids]
    results = [LevelResult() for _ in grids]

    def rec(lv, t_sub, parent, weight):
        if lv >= n:
            return
        g, st, res = grids[lv], states[lv], results[lv]
        fi, fo, vi, vo = _buffers(t_sub)
        has_children = lv + 1 < n
        if has_children and params.use_temporal_interp:
            if g.f_old.size <= 27:
                raise ValueError("temporal interpolation without temporal storage reads out of bounds in the reference")
            st["f_old"], st["rho_old"], st["vel_old"] = st[fi].copy(), st["rho"].copy(), st[vi].copy()
            res.old = (st["f_old"], st["rho_old"], st["vel_old"])
        if g.n_blocks:
            res.branches.append(_level_step(T, g, geometry(g, params), st, fi, fo, vi, vo, parent, t_sub, weight, u_curr, params))
        res.f_name, res.vel_name = fo, vo
        if has_children:
            me = _Parent(g, st, fo, vo)
            rec(lv + 1, 2 * t_sub, me, 0.0)
            rec(lv + 1, 2 * t_sub + 1, me, 0.5)

    rec(0, int(t), None, 0.0)
    for st, res in zip(states, results):
        res.f, res.vel, res.rho = st[res.f_name], st[res.vel_name], st["rho"]
        res.f_post_collision, res.post_read = st.get("f_post_collision"), st.get("post_read")
    return results


def tainted_cells(grids, params, t: int, run_a: List[LevelResult], run_b: List[LevelResult]):
    """Cells whose value two runs of the restatement (float32 and float64) cannot be compared at: a cell where they took different
    branches in some sub-step, and every cell that read such a cell's output later in the same coarse step - through its pulled
    set, its gradient stencil, an interface interpolation from the parent, or the Bouzidi cell behind.
    Returns per level (newest, old): bool [8,8,8,nb] for the newest buffers and for the saved old state."""
    n = len(grids)
    taint = [{name: np.zeros((B, B, B, g.n_blocks), dtype=bool) for name in ("f", "f_temp", "rho", "old")} for g in grids]
    sub = [0] * n

    def rec(lv, t_sub, parent_lv, parent_out):
        if lv >= n:
            return
        g, tn = grids[lv], taint[lv]
        geom = geometry(g, params)
        fi, fo, _, _ = _buffers(t_sub)
        has_children = lv + 1 < n
        if has_children and params.use_temporal_interp:
            tn["old"] = tn[fi].copy()
        bad_in = tn[fi]
        bad = run_a[lv].branches[sub[lv]] != run_b[lv].branches[sub[lv]]
        sub[lv] += 1
        for k in range(27):
            ix, iy, iz, blk, present = geom.neighbour(-C_K[k])
            bad |= np.where(present, bad_in[ix, iy, iz, blk], False)
            code = geom.code(k)
            bad |= ((code == _YMIR) | (code == _ZMIR)) & bad_in
            cells = np.nonzero(code == _IFACE)
            if cells[0].size:
                p, pt = grids[parent_lv], taint[parent_lv]
                src = pt[parent_out] | pt["rho"] | pt["old"]
                hit = np.zeros(cells[0].shape, dtype=bool)
                for px, py, pz, pb, ok in _interface_parent_cells(geom, k, cells, p.block_pointer.shape, np.asarray(p.block_pointer).astype(np.int64)):
                    hit |= ok & src[px, py, pz, pb]
                bad[cells] |= hit
        if g.bouzidi_enabled and g.n_boundary_cells > 0:
            collided = bad.copy()
            cb = np.asarray(g.bouzidi_cell_block).astype(np.int64) - 1
            x, y, z = (np.asarray(a).astype(np.int64) - 1 for a in (g.bouzidi_cell_x, g.bouzidi_cell_y, g.bouzidi_cell_z))
            for k in range(27):
                ix, iy, iz, blk, present = geom.neighbour(C_K[OPP[k]])
                ix, iy, iz = (np.broadcast_to(a, bad.shape)[x, y, z, cb] for a in (ix, iy, iz))
                bad[x, y, z, cb] |= present[x, y, z, cb] & collided[ix, iy, iz, blk[x, y, z, cb]]
        tn[fo] = bad
        tn["rho"] = bad
        if has_children:
            rec(lv + 1, 2 * t_sub, lv, fo)
            rec(lv + 1, 2 * t_sub + 1, lv, fo)

    rec(0, int(t), None, None)
    return [(taint[lv][run_a[lv].f_name], taint[lv]["old"]) for lv in range(n)]


def errors(got_f, got_vel, got_rho, ref: LevelResult, u_scale, cells=None):
    """max |got - ref| / scale per field class over `cells` (bool [8,8,8,nb]; default all): the scales of the module docstring"""
    sel = np.ones(ref.rho.shape, dtype=bool) if cells is None else cells
    if not sel.any():
        return {"f": 0.0, "vel": 0.0, "rho": 0.0}
    r = np.maximum(ref.rho.astype(np.float64), 1.0)
    ef = np.abs(got_f.astype(np.float64) - ref.f) / (W32.astype(np.float64) * r[..., None])
    ev = np.abs(got_vel.astype(np.float64) - ref.vel) / u_scale
    er = np.abs(got_rho.astype(np.float64) - ref.rho)
    out = {"f": ef[sel].max(), "vel": ev[sel].max(), "rho": er[sel].max()}
    return {k: (float(v) if np.isfinite(v) else float("inf")) for k, v in out.items()}


def velocity_scale(ref: List[LevelResult], u_curr) -> float:
    return max(max(float(np.abs(r.vel).max()) for r in ref if r.vel.size), float(u_curr), 1e-3)
