"""Block topologies the step's addressing can go wrong at, shared by the host test (tests/test_step_topologies_host.py) and the device
test (tests/test_gpu_step_topologies.py).

The step library derives three things from the neighbour table alone: the work list (x-runs of 4, leftover chains of 1-3, link bits,
the two launch classes), the LDS face hand-over with the dummy-block-then-patch path of the GENERAL kernel, and the priority chain
that picks the stand-in for a missing pull source. The cases of tests/_step_ref_cases.py are full rectangular level 1 grids with
box-shaped nests; the ones here are not: periodic boxes one block wide (a block is its own neighbour), tables periodic along some
axes only, a level 1 with holes (the w_k arm), L-shaped, disjoint and one-block-thick refinement patches on every domain face, and
a seeded random generator.

Every level holds at most 64 blocks and every case at most 3 levels; states are cases.init_perturbed, the inlet speed is 0.05, and
coarse steps 1-4 give both A/B parities and both child sub-step weights.

Two things follow from the 64-block cap. A block has all 26 neighbours only inside a 3 x 3 x 3 cube of blocks, which on a refined
level spans 2 x 2 x 2 parents = 64 blocks: a fine level with all-neighbour blocks is exactly that cube, so `nest_with_body` has it
(the raggedness the other nests have is left to them) and sits in a 7 x 3 x 3 level 1, whose interior row of 5 all-neighbour blocks
is one x-run of 4 and one lone block. And a random seed whose level 2 or 3 would exceed the cap is replaced by the next integer,
like one that misses a condition of the host test.
"""
from collections import namedtuple

import numpy as np

from open_ludwig_amd import cases
from open_ludwig_amd.physics import SolverParams

Case = namedtuple("Case", "build u steps")
U = 0.05
# mean speed of the start states. The float32 rounding of a cell's momentum sum is absolute (about 1.5e-7 at rho = 1) while the
# velocity bound of tests/_step_ref.py is relative to the step's largest speed: at cases.init_perturbed's default mean of 0.04
# three-level nests here put the velocity e_ref above the recorded MAX_E_REF, at 0.06 none of the table does
U_MEAN = 0.06
STEPS = (1, 2, 3, 4)
MAX_BLOCKS = 64
MAX_LEVELS = 3
TAU = 0.5006


def children(parents):
    """the 8 child blocks of every listed parent block (child = 2 * parent - 1 + {0, 1}, src/domain.jl:100-108)"""
    return sorted({(2 * bx - 1 + (d & 1), 2 * by - 1 + ((d >> 1) & 1), 2 * bz - 1 + ((d >> 2) & 1)) for bx, by, bz in parents for d in range(8)})


def _level(level_id, coords, dims, tau=TAU, periodic=(False, False, False), temporal=True):
    """level `level_id` of a domain of `dims` level-1 blocks; tau - 1/2 halves per level (src/physics_scaling.jl:139-143)"""
    s = 2 ** (level_id - 1)
    return cases.make_level(level_id, coords, tuple(d * s for d in dims), 0.5 + (tau - 0.5) / s, periodic=periodic, temporal=temporal)


def _params(dims, temporal, noise=0.0, wall=False, blend=False, symmetric=False):
    return SolverParams(domain_nx=dims[0] * 8, domain_ny=dims[1] * 8, domain_nz=dims[2] * 8, wall_model_active=wall, c_wale=0.5,
                        nu_sgs_bg=0.0005, inlet_turbulence=noise, use_temporal_interp=temporal, sponge_blend_dist=blend,
                        symmetric_analysis=symmetric, q_min_threshold=0.001)


def _finish(grids, dims, seed, sponge):
    for i, g in enumerate(grids):
        assert 0 < g.n_blocks <= MAX_BLOCKS, (g.level_id, g.n_blocks)
        if sponge:
            cases.add_sponge(g, dims[0] * 8 * 2 ** i)
        cases.init_perturbed(g, seed + i, u_mean=U_MEAN)
    assert len(grids) <= MAX_LEVELS
    return grids


def _periodic(dims, periodic=(True, True, True), seed=21):
    def build():
        g = _level(1, cases.full_box_coords(*dims), dims, periodic=periodic, temporal=False)
        return _finish([g], dims, seed, sponge=not periodic[0]), _params(dims, False)
    return build


HOLES_DIMS = (6, 3, 3)
# one interior block; two x-adjacent blocks of one row; the inlet-side and the outlet-side corner. Rows are cut to chains of
# 3 + 2 (by, bz = 2, 2), 1 + 3 (3, 1), 5 (1, 1) and 5 (3, 3); the other rows keep 6
HOLES = ((4, 2, 2), (2, 3, 1), (3, 3, 1), (1, 1, 1), (6, 3, 3))


def _level1_holes():
    coords = [c for c in cases.full_box_coords(*HOLES_DIMS) if c not in HOLES]
    g = _level(1, coords, HOLES_DIMS)
    return _finish([g], HOLES_DIMS, 31, sponge=True), _params(HOLES_DIMS, True, noise=0.01, blend=True)


RAGGED_DIMS = (5, 3, 3)
# level-2 parents: an L in the z = 1 plane from the inlet along y-min, then up to y-max; a single block in the outlet / y-max / z-max
# corner; a single block at the inlet under z-max. Together they touch all six domain faces.
RAGGED_L2_PARENTS = ((1, 1, 1), (2, 1, 1), (3, 1, 1), (3, 2, 1), (3, 3, 1), (5, 3, 3), (1, 2, 3))
# level-3 parents (level-2 blocks): two x-adjacent siblings, a block of the parent next door (an L across a parent boundary), and
# the outermost block of the corner patch, whose children lie against the outlet, y-max and z-max at once. None has all its siblings.
RAGGED_L3_PARENTS = ((5, 3, 1), (6, 3, 1), (5, 2, 1), (10, 6, 6))


def _ragged_nest():
    d = RAGGED_DIMS
    grids = [_level(1, cases.full_box_coords(*d), d), _level(2, children(RAGGED_L2_PARENTS), d), _level(3, children(RAGGED_L3_PARENTS), d)]
    assert set(RAGGED_L3_PARENTS) <= set(grids[1].active_block_coords)
    return _finish(grids, d, 41, sponge=True), _params(d, True, noise=0.01)


SLAB_DIMS = (6, 3, 2)


def _slab_nest():
    """level 2 one parent thick in y and z, 5 parents long: 10 x 2 x 2 fine blocks, all with a missing neighbour"""
    d = SLAB_DIMS
    grids = [_level(1, cases.full_box_coords(*d), d, temporal=False), _level(2, children([(x, 2, 1) for x in range(1, 6)]), d, temporal=False)]
    return _finish(grids, d, 51, sponge=True), _params(d, False, blend=True)


BODY_DIMS = (7, 3, 3)
BODY_CENTRE, BODY_RADIUS = (32.3, 16.7, 32.2), 10.4          # fine cells


def _nest_with_body():
    d = BODY_DIMS
    tau = 0.5003
    parents = [(x, y, z) for x in (2, 3) for y in (1, 2) for z in (2, 3)]          # against y-min and z-max
    grids = [_level(1, cases.full_box_coords(*d), d, tau=tau), _level(2, children(parents), d, tau=tau)]
    _finish(grids, d, 61, sponge=True)
    # the nest covers fine cells 17..48 x 1..32 x 17..48 of 112 x 48 x 48, its 8 all-neighbour blocks 25..40 x 9..24 x 25..40. The body
    # spans about 22..43 x 6..27 x 22..43: its surface crosses from the all-neighbour blocks into the general ones around them, and
    # it, the cells behind its links and the 4-cell wall-distance band stay inside the nest and off every domain face
    cases.add_sphere(grids[1], BODY_CENTRE, BODY_RADIUS, bouzidi=True, wall_dist=True)
    return grids, _params(d, True, noise=0.01, wall=True, blend=True)


def random_topology(seed, three_levels):
    """level-1 dimensions from 4..6 x 2..3 x 2..3; 0-15 % of the blocks dropped; 20-40 % of the rest refined; with three_levels 10-25 %
    of the level-2 blocks refined again; temporal, symmetric_analysis and the inlet noise drawn per seed.
    -> (dims, level-1 coords, level-2 parents, level-3 parents, flags), or None where a level would exceed MAX_BLOCKS"""
    rng = np.random.default_rng(seed)
    dims = (int(rng.integers(4, 7)), int(rng.integers(2, 4)), int(rng.integers(2, 4)))
    full = cases.full_box_coords(*dims)
    keep = sorted(rng.permutation(len(full))[int(round(rng.uniform(0.0, 0.15) * len(full))):].tolist())
    l1 = [full[i] for i in keep]
    n2 = int(round(rng.uniform(0.20, 0.40) * len(l1)))
    p2 = sorted(l1[i] for i in rng.permutation(len(l1))[:n2].tolist())
    l2 = children(p2)
    p3 = []
    if three_levels:
        n3 = max(1, int(round(rng.uniform(0.10, 0.25) * len(l2))))
        p3 = sorted(l2[i] for i in rng.permutation(len(l2))[:n3].tolist())
    flags = dict(temporal=bool(rng.integers(0, 2)), symmetric=bool(rng.integers(0, 2)), noise=0.01 * float(rng.integers(0, 2)))
    if len(l2) > MAX_BLOCKS or 8 * len(p3) > MAX_BLOCKS:
        return None
    return dims, l1, p2, p3, flags


def _random(seed, three_levels):
    def build():
        dims, l1, p2, p3, fl = random_topology(seed, three_levels)
        grids = [_level(1, l1, dims, temporal=fl["temporal"]), _level(2, children(p2), dims, temporal=fl["temporal"])]
        if p3:
            grids.append(_level(3, children(p3), dims, temporal=fl["temporal"]))
        return _finish(grids, dims, 100 + 10 * seed, sponge=True), _params(dims, fl["temporal"], noise=fl["noise"], symmetric=fl["symmetric"])
    return build


# seed -> three levels (half of them). Seeds are taken from 1 upward, two and three levels in turn; a seed whose draw puts a level
# over MAX_BLOCKS, or whose case misses a condition of the host test, is replaced by the next integer. The cap turns most draws
# down (a level 1 of 6 x 3 x 3 can never pass: 20 % of 46 blocks are 9 parents), which is why the seeds are sparse and the
# level-1 grids small; the host test asserts that the six still differ in temporal, symmetric_analysis and inlet noise.
RANDOM_SEEDS = {2: False, 3: True, 8: False, 19: True, 21: False, 25: True}

CASES = {
    "periodic_1x1x2": Case(_periodic((1, 1, 2)), U, STEPS),
    "periodic_2x1x1": Case(_periodic((2, 1, 1)), U, STEPS),
    "periodic_1x3x1": Case(_periodic((1, 3, 1)), U, STEPS),
    "periodic_2x2x1": Case(_periodic((2, 2, 1)), U, STEPS),
    "periodic_y_only": Case(_periodic((3, 2, 2), (False, True, False)), U, STEPS),
    "periodic_xz": Case(_periodic((2, 2, 1), (True, False, True)), U, STEPS),
    "level1_holes": Case(_level1_holes, U, STEPS),
    "ragged_nest": Case(_ragged_nest, U, STEPS),
    "slab_nest": Case(_slab_nest, U, STEPS),
    "nest_with_body": Case(_nest_with_body, U, STEPS),
}
for _seed, _three in RANDOM_SEEDS.items():
    CASES[f"random_{_seed}"] = Case(_random(_seed, _three), U, STEPS)

# device test subsets
OTHER_PATHS = ("level1_holes", "ragged_nest", "nest_with_body", "periodic_2x1x1")
DIRECT = ("level1_holes", "slab_nest")
OBSERVED = ("level1_holes", "periodic_1x3x1", "ragged_nest")


def direction(dx, dy, dz):
    """column of neighbor_table for the block offset (src/domain_topology.jl:135-160)"""
    return (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1)


def all_neighbour_blocks(level):
    """bool [n_blocks]: all 26 neighbours present - the blocks the library steps without edge or interface patching"""
    return (np.asarray(level.neighbor_table) > 0).all(axis=1)


def x_chains(level):
    """the maximal chains of x-consecutive blocks of one kind (all-neighbour or not) in every (by, bz) row, as lists of 0-based
    block indices: what the default work list cuts into x-runs of 4 and leftovers of 1-3"""
    table = np.asarray(level.neighbor_table)
    kind = all_neighbour_blocks(level)
    order = sorted(range(level.n_blocks), key=lambda b: (level.map_y[b], level.map_z[b], level.map_x[b]))
    chains = []
    for b in order:
        last = chains[-1][-1] if chains else None
        if (last is not None and level.map_y[last] == level.map_y[b] and level.map_z[last] == level.map_z[b] and kind[last] == kind[b]
                and table[last, direction(1, 0, 0)] == b + 1):
            chains[-1].append(b)
        else:
            chains.append([b])
    return chains
