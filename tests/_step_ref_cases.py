"""The case table of the float64 step reference (tests/_step_ref.py), shared by the host and the device test.

Every case is at most 8 x 4 x 4 coarse blocks and runs 4 coarse steps (even and odd t). The oracle only ADVANCES the state from one
snapshot to the next; expected values come from the restatement alone.

Tunnel table: pairwise coverage of (levels, temporal, sponge blend, symmetric, wall model at tau 0.5003, inlet noise, Bouzidi);
test_tunnel_table_is_pairwise checks it. Levels 3 uses the smallest tunnel that nests twice, levels 1 the widest.
"""
from collections import namedtuple

import numpy as np

import _step_ref as sr
from open_ludwig_amd import cases

Case = namedtuple("Case", "build u steps smooth wall")

#              levels temporal blend symmetric wall noise bouzidi
TUNNEL_TABLE = [(3, 0, 0, 1, 1, 1, 0),
                (3, 1, 1, 0, 0, 0, 1),
                (2, 0, 0, 0, 0, 1, 1),
                (2, 1, 1, 1, 1, 0, 0),
                (1, 0, 1, 1, 0, 0, 1),
                (1, 1, 0, 0, 1, 0, 1),
                (1, 1, 1, 0, 0, 1, 0)]
TUNNEL_SIZE = {1: (6, 4, 4), 2: (5, 3, 2), 3: (4, 2, 2)}
U_TUNNEL = 0.05
U_FAST = 0.12


def _tunnel(size, levels, temporal, blend, symmetric, wall, noise, bouzidi, seed=7, q_min=0.001):
    def build():
        grids, params = cases.tunnel_with_sphere(size, tau=0.5003 if wall else 0.5006, levels=levels, wall_model=bool(wall),
                                                 bouzidi=bool(bouzidi), sponge_blend=bool(blend), symmetric=bool(symmetric),
                                                 inlet_turbulence=0.01 if noise else 0.0, seed=seed, temporal=bool(temporal))
        params.q_min_threshold = q_min
        return grids, params
    return build


def _box(width, rough, tau=0.5006, nu_bg=None, u0=0.03):
    def build():
        grids, params = cases.periodic_box((width, 2, 2), tau=tau, u0=u0)
        if rough:
            cases.init_perturbed(grids[0], 5)
        if nu_bg is not None:
            params.nu_sgs_bg = nu_bg
        return grids, params
    return build


def _tunnel_at_rest():
    """wall model with the fluid at rest: |u| <= 1e-6 next to the wall until the inlet's wave arrives"""
    grids, params = cases.tunnel_with_sphere((4, 2, 2), tau=0.5003, levels=1, wall_model=True, inlet_turbulence=0.0)
    cases.set_state(grids[0], np.float32(1), np.float32(0), np.float32(0), np.float32(0))
    return grids, params


def _tunnel_strong_wall_force():
    """wall distances a tenth of the sphere's and a fast stream: the wall-model force reaches 1e-2, where its second-order part (u_eq, not u, inside
    the force term's c.u; the 1 - omega/2 factor) stands clear of float32 rounding - at the sphere's own distances it is below 1e-9"""
    grids, params = cases.tunnel_with_sphere((4, 2, 2), tau=0.5003, levels=1, wall_model=True, inlet_turbulence=0.0)
    near = grids[0].wall_dist < np.float32(100)
    grids[0].wall_dist[near] *= np.float32(0.1)
    cases.init_perturbed(grids[0], 7, u_mean=U_FAST)
    return grids, params


def _clamped_box():
    """a rough periodic box with two cells emptied: their pullers' density sum falls below the clamp"""
    grids, params = cases.periodic_box((3, 2, 2))
    cases.init_perturbed(grids[0], 11)
    for name in ("f", "f_temp"):
        getattr(grids[0], name)[3, 4, 5, 2, :] = 0
        getattr(grids[0], name)[2:5, 3:6, 4:7, 7, :] *= np.float32(1e-3)
    return grids, params


STEPS = (1, 2, 3, 4)
CASES = {}
for _w in (3, 5, 8):
    CASES[f"box{_w}_smooth"] = Case(_box(_w, False), 0.0, STEPS, True, False)
    CASES[f"box{_w}_rough"] = Case(_box(_w, True), 0.0, STEPS, False, False)
for _row in TUNNEL_TABLE:
    CASES["tunnel_L%d_t%d_b%d_s%d_w%d_n%d_z%d" % _row] = Case(_tunnel(TUNNEL_SIZE[_row[0]], *_row), U_TUNNEL, STEPS, False, bool(_row[4]))
# the noise seed t_sub % 10^6 wraps between the 2nd and the 3rd of these steps
CASES["noise_seed_wrap"] = Case(_tunnel((4, 2, 2), 1, 0, 1, 0, 0, 1, 1), U_TUNNEL, (999998, 999999, 1000000, 1000001), False, False)
# one block thick: cells at a y and a z mirror at once, inlet x mirror x mirror corners, Bouzidi cells with no block behind them
CASES["thin_y"] = Case(_tunnel((4, 1, 2), 1, 0, 1, 0, 0, 1, 1), U_TUNNEL, STEPS, False, False)
CASES["thin_z"] = Case(_tunnel((4, 2, 1), 1, 0, 0, 0, 1, 1, 1), U_TUNNEL, STEPS, False, True)
CASES["thin_yz"] = Case(_tunnel((4, 1, 1), 1, 0, 1, 1, 0, 1, 1, q_min=0.1), U_TUNNEL, STEPS, False, False)
# the refined region lies against the y-min plane (and the inlet): interface and mirror compete for the same population
CASES["interface_at_ymin"] = Case(_tunnel((4, 2, 2), 2, 1, 0, 1, 0, 1, 1), U_TUNNEL, STEPS, False, False)
# branches the tunnels leave empty
CASES["wall_at_rest"] = Case(_tunnel_at_rest, U_TUNNEL, STEPS, False, True)
CASES["wall_strong_force"] = Case(_tunnel_strong_wall_force, U_FAST, STEPS, False, True)
CASES["omega_floor"] = Case(_box(3, False, tau=0.5000005, nu_bg=0.0), 0.0, STEPS, True, False)
CASES["density_clamp"] = Case(_clamped_box, 0.0, STEPS, False, False)

# device test subsets: the Python recursion and 64-bit addressing
SUBSET = ("box5_rough", "tunnel_L2_t1_b1_s1_w1_n0_z0", "thin_yz", "interface_at_ymin")


def fluid_cells(level):
    return int((~np.asarray(level.obstacle).astype(bool)).sum())


class StepCheck:
    """What one coarse step of one case is judged by: ref64, the comparable cells, the velocity scale, e_ref"""

    def __init__(self, grids, params, t, u):
        self.t = t
        self.ref = sr.coarse_step(grids, params, t, u, np.float64)
        r32 = sr.coarse_step(grids, params, t, u, np.float32)
        self.tainted = sr.tainted_cells(grids, params, t, r32, self.ref)
        self.u_scale = sr.velocity_scale(self.ref, u)
        self.e_ref = {"f": 0.0, "vel": 0.0, "rho": 0.0}
        for lv, (a, b) in enumerate(zip(r32, self.ref)):
            e = sr.errors(a.f, a.vel, a.rho, b, self.u_scale, ~self.tainted[lv][0])
            for k in e:
                self.e_ref[k] = max(self.e_ref[k], e[k])
        self.excluded_share = [float(tn[0].sum()) / max(1, fluid_cells(g)) for g, tn in zip(grids, self.tainted)]
        self.branch_diff = [sum(int((x != y).sum()) for x, y in zip(a.branches, b.branches)) for a, b in zip(r32, self.ref)]

    def compare(self, lv, level, got, label, report=None):
        """got: name -> array of level lv after the step (f / vel under their buffer names, rho, optionally f_post_collision, f_old,
        rho_old, vel_old). Asserts the bounds of tests/_step_ref.py; returns the measured errors at the comparable cells."""
        ref = self.ref[lv]
        bad, bad_old = self.tainted[lv]
        fluid = ~np.asarray(level.obstacle).astype(bool)
        f, vel, rho = got[ref.f_name], got[ref.vel_name], got["rho"]
        for name, a in (("f", f), ("vel", vel), ("rho", rho)):
            assert np.isfinite(a).all(), f"{label} level {lv + 1} {name}: not finite"
        err = sr.errors(f, vel, rho, ref, self.u_scale, ~bad)
        if report is not None:
            report(lv, err)
        for kind in ("f", "vel", "rho"):
            assert err[kind] <= sr.bound(kind), (f"{label} level {lv + 1} {kind}: error {err[kind]:.3e} over the bound {sr.bound(kind):.3e} "
                                                 f"(ratio {err[kind] / sr.bound(kind):.2f})")
        # north star, its own hard bound: rho at every cell (excluded ones too), u at the comparable ones
        rel_rho = np.abs(rho.astype(np.float64) - ref.rho) / np.abs(ref.rho)
        assert rel_rho.max() <= sr.NORTH_STAR, f"{label} level {lv + 1}: rho off by {rel_rho.max():.3e} relative"
        ok = ~bad & fluid
        if ok.any():
            rel_u = (np.abs(vel.astype(np.float64) - ref.vel) / self.u_scale)[ok].max()
            assert rel_u <= sr.NORTH_STAR, f"{label} level {lv + 1}: u off by {rel_u:.3e} of {self.u_scale:.3e}"
        if "f_post_collision" in got and ref.post_read is not None:
            cells = ref.post_read & ~bad
            scale = sr.W32.astype(np.float64) * np.maximum(ref.rho, 1.0)[..., None]
            e = (np.abs(got["f_post_collision"].astype(np.float64) - ref.f_post_collision) / scale)[cells]
            assert e.size and e.max() <= sr.bound("f"), f"{label} level {lv + 1} f_post_collision: {e.max():.3e}"
        if "f_old" in got and ref.old is not None:
            # the state the level read in its last sub-step: the snapshot itself on level 1, a computed sub-step below it
            f_old, rho_old, vel_old = ref.old
            e = [np.abs(got["f_old"] - f_old) / (sr.W32.astype(np.float64) * np.maximum(rho_old, 1.0)[..., None]),
                 np.abs(got["vel_old"] - vel_old) / self.u_scale, np.abs(got["rho_old"] - rho_old)]
            for name, a, kind in zip(("f_old", "vel_old", "rho_old"), e, ("f", "vel", "rho")):
                worst = a[~bad_old].max()
                assert worst <= (0.0 if lv == 0 else sr.bound(kind)), f"{label} level {lv + 1} {name}: {worst:.3e} off the state the level read"
        return err
