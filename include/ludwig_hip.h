/*
 * ludwig_hip.h - C ABI of libludwig_hip.so, the MI355X (gfx950) collide-and-stream engine
 * that drops in under OPEN_Ludwig's per-level time-step API.
 *
 * Every entry point names the reference interface it replaces (paths are relative to the
 * reference repository root). The reference is Julia; the binding a maintainer adds is a
 * `ccall` wrapper, shown in INTEGRATION.md and julia/LudwigHIP.jl.
 *
 * Conventions
 *   - plain pointers and sizes only; host arrays are borrowed for the duration of the call.
 *   - host arrays use the reference's memory layout (src/blocks.jl:118-150): Julia
 *     column-major A[x,y,z,b,k] -> linear (x-1) + 8(y-1) + 64(z-1) + 512(b-1) + 512*n_blocks*(k-1);
 *     index tables keep the reference's 1-based values with 0 = absent.
 *   - every function returns LUDWIG_OK (0) or a negative LUDWIG_ERR_* code and never throws;
 *     the message is available from ludwig_last_error() (thread-local). One positive status exists,
 *     LUDWIG_ISO_REFUSED of ludwig_level_isosurface_extract: no error, a surface over the caller's cap.
 *   - a LudwigLevel is not re-entrant; calls are asynchronous on the level's HIP stream and
 *     ordered by it; ludwig_sync() is the reference's KernelAbstractions.synchronize.
 *   - lattice tables (c, w, opp, mirror_y, mirror_z of src/physics_v2.jl:99-117) are compile-time
 *     constants inside the library: k = (cx+1) + 3(cy+1) + 9(cz+1) (+1 in the reference).
 */
#ifndef LUDWIG_HIP_H
#define LUDWIG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LUDWIG_ABI_VERSION 1

#define LUDWIG_OK              0
#define LUDWIG_ERR_INVALID    -1   /* bad argument / inconsistent sizes          */
#define LUDWIG_ERR_HIP        -2   /* a HIP runtime call failed                  */
#define LUDWIG_ERR_NO_DEVICE  -3   /* no usable gfx950 device                    */
#define LUDWIG_ERR_ALLOC      -4   /* device or host allocation failed           */
#define LUDWIG_ERR_STATE      -5   /* call not valid for this level's storage    */

/* Fields of BlockLevel (src/blocks.jl:16-65) addressable through upload/download/field_ptr. */
enum LudwigField {
    LUDWIG_F = 0,            /* f                 [8,8,8,nb,27] f32 */
    LUDWIG_F_TEMP = 1,       /* f_temp            [8,8,8,nb,27] f32 */
    LUDWIG_F_POST = 2,       /* f_post_collision  [8,8,8,nb,27] f32 (only if n_boundary_cells > 0) */
    LUDWIG_F_OLD = 3,        /* f_old             [8,8,8,nb,27] f32 (only if temporal storage)     */
    LUDWIG_RHO = 4,          /* rho               [8,8,8,nb]    f32 */
    LUDWIG_RHO_OLD = 5,
    LUDWIG_VEL = 6,          /* vel               [8,8,8,nb,3]  f32 */
    LUDWIG_VEL_TEMP = 7,
    LUDWIG_VEL_OLD = 8,
    LUDWIG_OBSTACLE = 9,     /* obstacle          [8,8,8,nb]    u8 (Bool) */
    LUDWIG_SPONGE = 10,      /* sponge            [8,8,8,nb]    f32 */
    LUDWIG_WALL_DIST = 11,   /* wall_dist         [8,8,8,nb]    f32 */
    LUDWIG_FIELD_COUNT = 12
};

/* Which blocks of a level a launch covers (multi-GPU overlap of halo exchange and interior work). */
enum LudwigPart {
    LUDWIG_PART_ALL = 0,
    LUDWIG_PART_BOUNDARY = 1,   /* owned blocks flagged in LudwigLevelHost.comm_boundary */
    LUDWIG_PART_INTERIOR = 2    /* the other owned blocks                                  */
};

typedef struct LudwigLevel LudwigLevel;   /* opaque; owns all device memory of one BlockLevel */

/*
 * Host description of one BlockLevel, consumed by ludwig_level_create, which replaces
 * `adapt(backend, level)` (src/blocks.jl:67-87, called at src/main.jl:98).
 * Optional pointers may be NULL: the constructor defaults of src/blocks.jl:118-150 apply
 * (rho = 1, vel = 0, f = 0, obstacle = false, sponge = 0, wall_dist = 100).
 */
typedef struct LudwigLevelHost {
    int32_t level_id;              /* 1-based, BlockLevel.level_id                                  */
    int32_t n_blocks;              /* blocks in the arrays = owned blocks followed by ghost blocks  */
    int32_t n_owned;               /* blocks this device steps; 0 means n_blocks (single device),
                                      < 0 means none (the level only holds ghost copies here)        */
    float   tau;                   /* BlockLevel.tau                                                */
    int32_t grid_dim_x, grid_dim_y, grid_dim_z;   /* size(block_pointer)                            */
    const int32_t *block_pointer;  /* [dim_x,dim_y,dim_z], 1-based, 0 = absent (src/blocks.jl:111-114) */
    const int32_t *neighbor_table; /* [n_blocks,27], 1-based, 0 = absent (src/domain_topology.jl:135-160) */
    const int32_t *map_x, *map_y, *map_z;         /* [n_blocks] 1-based block coords                */
    const uint8_t *obstacle;       /* optional */
    const float   *sponge;         /* optional */
    const float   *wall_dist;      /* optional */
    int32_t enable_temporal_interpolation;        /* allocate f_old/rho_old/vel_old (src/blocks.jl:123-142) */
    int32_t n_boundary_cells;      /* > 0 with a q map enables Bouzidi (src/blocks.jl:152); < 0: no cells here, but allocate and
                                      store f_post_collision anyway (multi-GPU: a peer's Bouzidi cells read this rank's face layer) -
                                      in every block, until ludwig_level_add_post_collision_readers says where it is read */
    const uint16_t *bouzidi_q_map; /* Float16 bits [8,8,8,nb,27]; optional                          */
    const int32_t  *bouzidi_cell_block;           /* [n_boundary_cells] 1-based                     */
    const int8_t   *bouzidi_cell_x, *bouzidi_cell_y, *bouzidi_cell_z;   /* 1-based local coords     */
    const uint8_t  *comm_boundary; /* optional [n_blocks]: 1 = owned block adjacent to a ghost block */
    int32_t store_post_collision_everywhere;      /* 0: f_post_collision is written only where it has a reader (the reference writes
                                      it for every cell, src/physics_kernels.jl:350-352, and reads it only in the Bouzidi kernel,
                                      src/bouzidi_kernel.jl:44-77): the x-rows of 8 cells that hold a listed Bouzidi cell with a link
                                      q > 0 or the cell one step behind such a link; whole blocks that hold or touch a listed cell
                                      when the step's q_min_threshold is negative (every direction is a link then) or with
                                      LUDWIG_POST_ROWS=0. The rest of the array keeps what it held (zeros after create).
                                      1: every block, as the reference (multi-GPU: a peer's cells read this rank's blocks)  */
} LudwigLevelHost;

/*
 * Scalar arguments of perform_timestep_v2! (src/physics_v2.jl:26-38) that are constant over a run,
 * plus the globals it reads (SYMMETRIC_ANALYSIS src/physics_v2.jl:71, Q_MIN_THRESHOLD :93).
 */
typedef struct LudwigStepFlags {
    int32_t domain_nx, domain_ny, domain_nz;   /* coarse (level-1) cell dims                 */
    int32_t is_symmetric;
    int32_t wall_model_active;
    int32_t use_temporal_interp;
    int32_t sponge_blend_distributions;
    float   c_wale;
    float   nu_sgs_background;
    float   inlet_turbulence;
    float   q_min_threshold;
} LudwigStepFlags;

/* ---- library ---- */
int         ludwig_abi_version(void);
const char *ludwig_last_error(void);
int         ludwig_device_count(int *count);

/* ---- level life cycle: adapt(backend, BlockLevel) src/blocks.jl:67-87 ---- */
int  ludwig_level_create(const LudwigLevelHost *host, int device, LudwigLevel **out);
void ludwig_level_destroy(LudwigLevel *level);

/* HIP stream (hipStream_t) all later calls on this level are queued on; NULL = the null stream. */
int  ludwig_level_set_stream(LudwigLevel *level, void *hip_stream);

/* Multi-GPU, Bouzidi levels: name the f_post_collision elements somebody OUTSIDE this level's own cell list reads - a peer rank's
 * Bouzidi links reach one cell across a cut (src/bouzidi_kernel.jl:47-58), i.e. exactly the elements of this rank's group-2 send
 * lists (ludwig_halo_plan_create). offsets: element offsets into f_post_collision in the reference layout [8,8,8,n_blocks,27], like the
 * halo index lists. The library adds their x-rows to the rows the stream-collide step stores (store_post_collision_everywhere above);
 * a level created with n_boundary_cells < 0 stops storing every block from the first call on (n = 0 is a valid call: nobody reads).
 * No effect on a level created with store_post_collision_everywhere = 1. May be called again; the sets add up. Synchronizes the stream. */
int  ludwig_level_add_post_collision_readers(LudwigLevel *level, const int64_t *offsets, int64_t n);

/*
 * A HIP stream whose kernels may use every compute unit of `device` except `reserved_cus` of them (0 = an ordinary stream).
 * For the multi-GPU schedule: the interior blocks of step t + 1 run while the halo of step t travels (ludwig_halo_pack, RCCL
 * send/recv, ludwig_halo_unpack on other streams). A stream-collide launch fills every CU, and a send/recv kernel queued beside
 * it - even on a high-priority stream - is handed its workgroups only as the launch drains (measured: 20 us alone, 470 us beside
 * it). Compute units the stepping stream never uses are free the moment the exchange needs them; the step is HBM-bound and does
 * not miss them. The reserved CUs are spread evenly over the XCDs AND over the four shader engines of every XCD (an unbalanced mask costs the
 * step more than a larger balanced one): on a 256-CU device the request is rounded up to a multiple of 32. No reference counterpart (single GPU);
 * hipStream_t in *stream_out.
 */
int  ludwig_stream_create(int device, int reserved_cus, void **stream_out);
int  ludwig_stream_destroy(int device, void *hip_stream);

/*
 * Launch order of the stream-collide kernel. One item per WAVE: items[i] = (block0 << 3) | z with block0 0-based
 * and z in 0..7 = the 8x8 z-plane of that block the wave steps; a negative item is an idle wave. Every
 * (block, plane) of the part must appear exactly once. Purely a performance knob (L2 / Infinity-Cache
 * locality); results do not depend on it. Default: x-runs, plane-per-XCD, see DESIGN.md.
 * What the library makes of the list: 4 consecutive items form one workgroup, and workgroup
 * g is expected on XCD g % 8. A group of 4 items whose blocks are all of one kind (all 26 neighbours present, or all
 * with a missing neighbour) keeps its composition and its slot; items of mixed or incomplete groups are re-packed behind
 * them. Neighbouring items of a group that hold x-adjacent blocks at the same plane exchange their face column through
 * LDS. Levels below 8 192 owned blocks step both kinds in one launch (LUDWIG_MERGE_CLASSES overrides).
 */
int  ludwig_level_set_order(LudwigLevel *level, int part, const int32_t *items, int64_t n_items);

/* Array(level.field) / copyto!(level.field, host) */
int  ludwig_level_upload(LudwigLevel *level, int field, const void *host, size_t bytes);
int  ludwig_level_download(const LudwigLevel *level, int field, void *host, size_t bytes);
/* The device arrays hold the blocks in the library's own order (x-consecutive blocks consecutive in memory), not in the
 * reference's. Every entry point that takes or returns arrays, block ids or element offsets speaks the REFERENCE order and
 * translates; only raw pointers (below) expose the internal one: element (cell, block b, component k) of a field lives at
 * cell + 512 * ref_to_internal[b] + 512 * n_blocks * k. ref_to_internal: [n_blocks], filled by this call (identity when the
 * environment variable LUDWIG_REFERENCE_BLOCK_ORDER is set). */
int  ludwig_level_block_order(const LudwigLevel *level, int32_t *ref_to_internal);

/* Raw device pointer of a field (e.g. to let RCCL receive straight into it); blocks in the internal order, see above. The pointer stays valid for the life of the
 * level and the caller may write through it whenever the level's stream is idle. Because the library cannot see such writes,
 * a level that has handed out a pointer to a state field gives up three internal shortcuts from then on (results are the
 * same, it is only slower): copy_to_old! really copies, the interface values of its children are no longer computed one
 * sub-step ahead, rho is stored by every step. Geometry fields (obstacle, sponge, wall_dist) must be changed with
 * ludwig_level_upload, which also refreshes the per-block flags derived from them. */
int  ludwig_level_field_ptr(const LudwigLevel *level, int field, void **device_ptr, size_t *bytes);
/* Layout of a device array, for raw pointers: the device arrays are BLOCK-major - element (cell, block b, component k) of a field
 * with K components lives at cell + component_stride * k + block_stride * ref_to_internal[b], with component_stride = 512 and
 * block_stride = 512 K (the 27 populations of a block are one contiguous 54-KiB piece), whereas every array passed through the ABI
 * keeps the reference's [8,8,8,n_blocks,K] (src/blocks.jl:118-150: components 512 n_blocks apart). Why: 27 + 27 concurrent streams
 * n_blocks x 2 KiB apart load MI355X's memory system unevenly at distances that depend on nothing but n_blocks.
 * Strides in ELEMENTS; any output pointer may be NULL. */
int  ludwig_level_field_layout(const LudwigLevel *level, int field, int32_t *components, int64_t *block_stride, int64_t *component_stride);

/* init_eq! (src/main.jl:109-134): f = f_temp = (f_old) = w_k, rho_old = 1, vel_old = 0 */
int  ludwig_init_equilibrium(LudwigLevel *level);

/* ---- stepping ---- */
/*
 * perform_timestep_v2! (src/physics_v2.jl:26-97) with the A/B roles of src/solver_control.jl:35-41
 * derived from t_sub: iseven(t_sub) -> in = f/vel, out = f_temp/vel_temp, else swapped.
 * parent == NULL <=> level 1 (parent_f === nothing). For a child, the parent's newest state is the
 * output of the parent's step t_sub >> 1 (src/solver_control.jl:63-83) and is selected the same way.
 * Runs stream-collide, then the Bouzidi correction if the level has boundary cells.
 */
int  ludwig_step(LudwigLevel *level, const LudwigLevel *parent, int64_t t_sub,
                 float u_curr, float parent_tau, float temporal_weight,
                 const LudwigStepFlags *flags);

/* The two kernels of perform_timestep_v2! separately (src/physics_v2.jl:58-83 and :87-96), so that a
 * multi-GPU caller can exchange halos in between and overlap interior work. `part` is a LudwigPart. */
int  ludwig_stream_collide(LudwigLevel *level, const LudwigLevel *parent, int64_t t_sub,
                           float u_curr, float parent_tau, float temporal_weight,
                           const LudwigStepFlags *flags, int part);
/* apply_bouzidi_correction! (src/bouzidi_kernel.jl:99-123) on the output buffer of step t_sub */
int  ludwig_bouzidi_correction(LudwigLevel *level, int64_t t_sub, float q_min_threshold);

/* copy_to_old!(level, f_in, vel_in) (src/blocks.jl:199-205) for the step t_sub about to run */
int  ludwig_save_old(LudwigLevel *level, int64_t t_sub);

/*
 * execute_timestep_batch! (src/solver_control.jl:145-165) in one call: for t = t_start .. t_start+batch_size-1 run
 * recursive_step!(grids, 1, t, ...) - per level: A/B roles from t_sub parity, copy_to_old! when the level has children
 * and temporal interpolation is on, perform_timestep_v2!, then the child level twice (2 t_sub with temporal weight 0.0,
 * 2 t_sub + 1 with 0.5) - and synchronize at the end like the reference. levels[0] is level 1; all on one device.
 */
int  ludwig_execute_timestep_batch(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size,
                                   float u_curr, const LudwigStepFlags *flags);

/* What a batch observes while it steps: a list of tagged entries, each a set (made by ludwig_probes_create, ludwig_surface_stats_create,
 * ludwig_force_series_create, ludwig_tracers_create, ludwig_flux_planes_create or ludwig_modes_create, below) observed at coarse steps
 * start_step + k interval, k >= 0. */
enum { LUDWIG_OBSERVE_PROBES = 0, LUDWIG_OBSERVE_SURFACE = 1, LUDWIG_OBSERVE_FORCES = 2, LUDWIG_OBSERVE_TRACERS = 3,
       LUDWIG_OBSERVE_FLUXES = 4, LUDWIG_OBSERVE_MODES = 5 };
typedef struct LudwigBatchObserver {
    int32_t kind;        /* LUDWIG_OBSERVE_* */
    void   *set;         /* LudwigProbes* / LudwigSurfaceStats* / LudwigForceSeries* / LudwigTracers* / LudwigFluxPlanes* / LudwigModes*; NULL: ignored */
    int64_t start_step;  /* observed at coarse steps start_step + k interval, k >= 0 */
    int32_t interval;
} LudwigBatchObserver;
/* ludwig_execute_timestep_batch with the sets of `observers` observed inside the batch, in any order, at most one per kind.
 * n_observers = 0 (observers may then be NULL) is ludwig_execute_timestep_batch itself; an entry with a null set is skipped, its
 * start_step and interval unread. Probes, the surface set and the force series: one launch (the force series: its reduction tree) per
 * level concerned on that level's own stream, right after its last sub-step of an observed coarse step; the probes' ring slot is opened
 * only then. Tracers: one advance behind an observed coarse step, when the host has issued every launch of that step and none of the
 * next; with level streams the first level's stream waits for all the others, runs the advance, and all the others wait for it (ordering
 * only). Everything is refused before anything is stepped, in this order: the levels; LUDWIG_ERR_INVALID with "observer" in the message
 * for n_observers < 0, observers NULL with n_observers > 0, an unknown kind, or two non-null entries of one kind; then per set
 * LUDWIG_ERR_INVALID for interval < 1, probes or tracers not made over exactly these levels (same handles, same order), a surface or
 * force set whose level is not in `levels`, and LUDWIG_ERR_STATE if the batch's probe samples or force records would overflow the free
 * ring. Flux planes (checked last): the ring slot is opened when an observed coarse step begins, every level that holds points launches
 * its reduction on its own stream right after its last sub-step of that step - no stream join, no host synchronisation;
 * LUDWIG_ERR_INVALID for interval < 1 or a set not made over exactly these levels, LUDWIG_ERR_STATE if the batch's records would
 * overflow the free ring. Modes (checked after the flux planes): at an observed coarse step t the table row is ((t - start_step) /
 * interval) % n_rows; every level with owned blocks launches its sample on its own stream right after its last sub-step of that step -
 * no stream join, no event, no host synchronisation; LUDWIG_ERR_INVALID for interval < 1 or a set not made over exactly these levels,
 * LUDWIG_ERR_STATE unless the batch's observed steps give exactly the rows count, count + 1, ... of every level (count: its samples
 * since the last reset) and all of them are below n_rows: a batch never runs past the end of a window, the caller cuts there. */
int  ludwig_execute_timestep_batch_observed(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size,
                                            float u_curr, const LudwigStepFlags *flags, const LudwigBatchObserver *observers,
                                            int32_t n_observers);

/* KernelAbstractions.synchronize(backend) (src/solver_control.jl:164) */
int  ludwig_sync(const LudwigLevel *level);

/* ---- surface stresses for the force diagnostics (the caller of the path on the output side) ----
 * map_stresses_kernel! (src/forces/surface.jl:138-266, launched at :406-420): for every triangle the nearest fluid cell
 * of the level (shells of radius 0..search_radius around the cell holding the triangle centre, scan order dz, dy, dx, the
 * first strictly smaller distance wins, the search stops after a shell of radius > 1 once a cell was found), then
 * p = (rho - 1) / 3 * pressure_scale and tau = rho * nu * u_t / d * stress_scale (compute_stress_from_cell :32-76).
 * centers / normals: HOST [n_triangles * 3] Float32 (x, y, z per triangle, mesh coordinates: the offset is added here);
 * outputs: HOST [n_triangles] Float32 each. vel_field: LUDWIG_VEL (what the reference reads, :412) or LUDWIG_VEL_TEMP.
 * The integration (integrate_forces_kernel! :282-366) stays with the caller: it is a sum over these four arrays. */
typedef struct LudwigSurfaceParams {
    float   dx;                 /* level.dx                                  */
    float   tau;                /* level.tau                                 */
    float   offset_x, offset_y, offset_z;   /* params.mesh_offset            */
    float   pressure_scale, stress_scale;
    int32_t search_radius;      /* reference: 5 (src/main.jl:197)            */
} LudwigSurfaceParams;

int  ludwig_map_surface_stresses(const LudwigLevel *level, int vel_field, int32_t n_triangles, const float *centers,
                                 const float *normals, const LudwigSurfaceParams *sp,
                                 float *pressure, float *shear_x, float *shear_y, float *shear_z);

/* compute_flow_stats (src/diagnostics.jl:56-94, CUDA branch), the rho_min column of the run log: minimum of rho over the
 * non-obstacle cells of the blocks this device owns, reduced on the device (+inf for a level without owned blocks). A
 * multi-GPU caller takes the minimum over ranks (one all-reduce MIN). */
int  ludwig_level_rho_min(const LudwigLevel *level, float *rho_min);

/* rho store policy. perform_timestep_v2!'s kernel writes rho for every cell on every step (src/physics_kernels.jl:243-246). By
 * default a level nobody reads rho of between two steps skips that store and reproduces the array on demand, bit for bit (every
 * reader inside the library asks for it). every_step = 1 restores the reference's store pattern on this level
 * (LUDWIG_EAGER_RHO=1 in the environment does it for every level), 0 lets the library elide again. Results never depend on it. */
int  ludwig_level_set_rho_store(LudwigLevel *level, int every_step);

/* ---- record step (no reference counterpart; DESIGN.md section 3.1 "Record step") ----
 * The post-collision state of a plain cell is a function of 11 floats (rho, u, the six components of the non-equilibrium stress and
 * 1 - omega). A level every cell of which is plain keeps those between steps instead of f, vel and rho - 44 B written and 44 B read per
 * cell update against 240 - and turns them back into populations, bit for bit, before anything reads, hands out or writes f, vel or rho.
 * Results never depend on it; LUDWIG_RECORD_STEP=0 in the environment turns it off.
 *
 * ludwig_record_step_rule: the rule, as a function of what a level is (no device needed). 1 = such a level steps by records: every
 * block is owned (n_owned == n_blocks > 0: one rank, no ghost blocks), the level has no parent, no saved state for temporal
 * interpolation, no f_post_collision and no wall model, and every block's flags word (LUDWIG internal: bit 0 all 26 neighbours present,
 * bit 1 obstacle, bit 2 sponge, bit 3 near-wall, bit 4 post-collision readers) is exactly 1. 0 = f path; -1 = bad arguments. On top of it
 * a step goes by records only as a whole-level launch (LUDWIG_PART_ALL) outside batches that run in-batch observers or several levels,
 * and never once a writable pointer into the level was handed out, a halo plan was made for it or another level used it as its parent. */
int  ludwig_record_step_rule(const int32_t *block_flags, int32_t n_blocks, int32_t n_owned, int32_t has_parent,
                             int32_t has_temporal_storage, int32_t has_post_collision, int32_t wall_model_active);
/* how many of the level's steps so far went by records (0 on a level the rule excludes) */
int  ludwig_level_record_steps(const LudwigLevel *level, int64_t *n_steps);

/* ---- time-averaged statistics (no reference counterpart) ----
 * Per cell of the blocks this device owns, in double precision: S_rho += rho, S_u[i] += u_i, S_uu[m] += u_i u_j (m = xx, yy, zz, xy,
 * yz, xz: VTK's symmetric-tensor order). Each sum is a plain sequential addition in sample order, so a float64 replay on the host
 * reproduces it bit for bit. The accumulators (80 B per cell) are allocated by the first reset; a level that never resets allocates
 * and launches nothing. A level created with n_owned < 0 accepts every call and does nothing. */
enum LudwigStat { LUDWIG_STAT_RHO = 0, LUDWIG_STAT_VEL = 1, LUDWIG_STAT_VEL2 = 2 };   /* K = 1, 3, 6 components */
/* allocate on the first call, zero the sums, n = 0 (queued on the level's stream) */
int  ludwig_level_stats_reset(LudwigLevel *level);
/* add one sample: rho as ludwig_level_download(LUDWIG_RHO) would return it now (an elided store is replayed first) and the velocity
 * buffer sub-step t_sub wrote (vel_temp if t_sub is even, vel if odd). Queued on the level's stream, no host synchronisation.
 * LUDWIG_ERR_STATE before the first reset. */
int  ludwig_level_stats_accumulate(LudwigLevel *level, int64_t t_sub);
/* the sums of one statistic in the reference layout [8,8,8,n_blocks,K] Float64, reference block order, ghost blocks zero; bytes =
 * 4096 n_blocks K; *n_samples (may be NULL) = samples since the last reset. Synchronizes the stream. LUDWIG_ERR_STATE before the first reset. */
int  ludwig_level_stats_download(const LudwigLevel *level, int stat, double *host, size_t bytes, int64_t *n_samples);

/* ---- flow monitor: compute_flow_stats of a level plus where (src/diagnostics.jl:56-94; the locations, the non-finite count and
 * the fixed summation order have no reference counterpart) ----
 * One record from one pass over the blocks this device owns: rho as ludwig_level_download(LUDWIG_RHO) would return it now (an elided
 * store is replayed first), the velocity buffer sub-step t_sub wrote (vel_temp if t_sub is even, vel if odd) and obstacle. Per
 * non-obstacle cell v2 = (ux ux + uy uy) + uz uz in float32; the cell is counted iff rho, ux, uy, uz and v2 are all finite, else bad.
 *   counts[2]    non-obstacle cells, bad cells
 *   extremes[3]  min rho, max rho, max v2 over the counted cells (IEEE < and >); +inf, -inf, -inf without a counted cell
 *   cells[4][4]  (bx, by, bz, x + 8 y + 64 z) of the min-rho, max-rho, max-v2 cell - among equal values the lowest in
 *                (bx, by, bz, z, y, x) order, whatever the block order - and of the lowest bad cell; -1 four times where absent.
 *                Block coordinates are the level's map_x/y/z (at most 2^18 - 1 per axis, LUDWIG_ERR_INVALID otherwise)
 *   sums[2]      Float64 sums of rho and of rho v2 over the counted cells (every other cell adds +0.0) in one fixed balanced tree:
 *                adjacent pairs halved, x = x[0::2] + x[1::2], over the 512 cells of a block in cell order, then over the per-block
 *                results in the caller's block order with +0.0 appended wherever a length is odd.
 * The per-block scratch (80 B per owned block) is allocated by the first call; a level never monitored allocates and launches nothing.
 * Runs on the level's stream: one small download, one synchronisation. A level created with n_owned < 0 returns the empty record. */
int  ludwig_level_monitor(LudwigLevel *level, int64_t t_sub, int64_t *counts, int64_t *cells, float *extremes, double *sums);

/* ---- wall diagnostics: what the wall model does in its own range (no reference counterpart: the reference reads y_plus_target and
 * never computes a y+) ----
 * The wall-model state of a cell is what perform_timestep_v2!'s kernel passes through on its way to the wall force
 * (src/physics_kernels.jl:206-236), restated operation by operation in float32 from (wall_dist, the level's tau, rho, |u| =
 * sqrt(ux ux + uy uy + uz uz)): u_tau, y_plus = u_tau wall_dist / nu - the FINAL u_tau, not the provisional one that picks the branch -
 * and a code: 0 not near the wall (!(0 < wall_dist < 10)) or an obstacle cell, 1 near the wall but the model is skipped (|u| <= 1e-6 or
 * nu <= 1e-10), 2 the power law's u_tau is kept (y_p <= 11.81 or u_plus_law <= 0.1), 3 the log law replaced it; 4 is or-ed in where the
 * step applies a force (tau_wall > tau_res). Codes 0 and 1 give u_tau = y_plus = 0. The step stores rho and u after the sponge and before
 * the force, so the state sub-step t_sub wrote is exactly what that sub-step's wall model saw.
 *
 * ludwig_level_wall_census: one all-integer record from one pass over the blocks this device owns (blocks without a near-wall cell are
 * skipped): rho as ludwig_level_download(LUDWIG_RHO) would return it now (an elided store is replayed first), the velocity buffer sub-step
 * t_sub wrote (vel_temp if t_sub is even, vel if odd), the level's wall_dist, obstacle and tau.
 *   near_cells   non-obstacle cells with 0 < wall_dist < 10
 *   evaluated    of those, the cells with code >= 2 whose y_plus and wall shear rho u_tau u_tau are both finite
 *   log_law, forced   of the evaluated cells, those with code 3 / with the force bit
 *   non_finite   cells with code >= 2 whose y_plus or wall shear is not finite; they count here and in near_cells only
 *   min_bits, max_bits   the float32 bits of the least / greatest y_plus over the evaluated cells (positive floats order as unsigned
 *                integers); 0xFFFFFFFF / 0 when there is none
 *   hist         the evaluated cells by y_plus, eight bins per octave from the bits alone: with e8 = bits >> 20 (the exponent and the top
 *                three mantissa bits) bin 0 if e8 < 936 (y_plus < 2^-10), bin 1 + (e8 - 936) for 936 <= e8 < 1128, bin 193 if e8 >= 1128
 *                (2^14 and above); the lower edge of bin j in 1..193 is the float with bits (935 + j) << 20
 * Integer sums commute, so the record depends on neither the block order nor on how the level is cut over ranks: the records of the
 * ranks add up (min / max of the bits) to one device's. The 1.6-KB device record is made by the first call; a level never asked
 * allocates and launches nothing. Runs on the level's stream: one small download, one synchronisation. A level created with
 * n_owned < 0 returns the empty record. */
#define LUDWIG_WALL_BINS 194
typedef struct LudwigWallCensus {
    uint64_t near_cells, evaluated, log_law, forced, non_finite;
    uint32_t min_bits, max_bits;
    uint64_t hist[LUDWIG_WALL_BINS];
} LudwigWallCensus;
int  ludwig_level_wall_census(LudwigLevel *level, int64_t t_sub, LudwigWallCensus *out);

/* A wall-surface set lives on one level (the finest). Triangle i reads its nearest fluid cell (reference block index blocks[i], 0-based,
 * -1 = none found; cell cells[i] = x + 8 y + 64 z) and has the normal normals[3i + 0..2]. A compute evaluates seven float32 values per
 * triangle, [7][n_tri]: p exactly as ludwig_map_surface_stresses does for that cell; tau_model_x, y, z = (rho u_tau u_tau) stress_scale
 * along the tangential velocity u - (u.n) n (that call's direction), zero where |u_t| <= 1e-10 or code < 2; u_tau; y_plus; the code as
 * a float. The wall distance of the model is the LEVEL's wall_dist at the cell - the one the step used - and tau the level's own; of sp
 * only pressure_scale and stress_scale are read. A triangle without a cell gives the p of rho = 1 and zeros. n_tri = 0 is allowed (a rank
 * that owns none of the triangles). The level may hold at most 2^31 / 512 blocks. */
typedef struct LudwigWallSurface LudwigWallSurface;   /* opaque */
int  ludwig_wall_surface_create(LudwigLevel *level, int32_t n_tri, const int32_t *blocks, const int32_t *cells, const float *normals,
                                const LudwigSurfaceParams *sp, LudwigWallSurface **out);
/* frees the set, not the level; it does not touch the level, so it may come before or after its destruction */
void ludwig_wall_surface_destroy(LudwigWallSurface *set);
/* evaluate the state sub-step t_sub wrote (vel_temp if t_sub is even, vel if odd; rho as a download would return it), queued on the
 * level's stream, no host synchronisation */
int  ludwig_wall_surface_compute(LudwigWallSurface *set, int64_t t_sub);
/* the last computed values [7][n_tri] in the caller's triangle order (bytes must be 7 * n_tri * 4); synchronizes the level's stream.
 * LUDWIG_ERR_STATE before the first compute. */
int  ludwig_wall_surface_download(LudwigWallSurface *set, float *values, size_t bytes);

/* ---- velocity-gradient fields (no reference counterpart for the output; the gradient is compute_velocity_gradients,
 * src/physics_utils.jl:44-82, the one WALE uses) ----
 * Per cell of the blocks this device owns, from one velocity buffer u: g_ij = (0.5f (u_i(+e_j) - u_i(-e_j))) * scale with the
 * neighbour value of get_velocity_neighbor (across a block face through the neighbour table; no block there: the cell's own
 * value), vorticity = (g32 - g23, g13 - g31, g21 - g12) and Q = -0.5f (((g11 g11 + g22 g22) + g33 g33) + 2 ((g12 g21 + g13 g31)
 * + g23 g32)), float32 in this order; obstacle cells 0. The output buffer (16 B per cell) is allocated by the first compute; a
 * level that never computes allocates and launches nothing. A level created with n_owned < 0 accepts every call and does nothing. */
enum LudwigGradField { LUDWIG_GRAD_VORTICITY = 0 /* K = 3 */, LUDWIG_GRAD_Q = 1 /* K = 1 */ };
/* vel_field: LUDWIG_VEL or LUDWIG_VEL_TEMP; scale: finite, non-zero (1/dx for derivatives per unit length). Reads vel, obstacle and
 * the neighbour table only; queued on the level's stream, no host synchronisation. */
int  ludwig_level_gradient_fields_compute(LudwigLevel *level, int vel_field, float scale);
/* the last computed field in the reference layout [8,8,8,n_blocks,K] Float32, reference block order, ghost blocks zero; bytes =
 * 2048 n_blocks K. Synchronizes the stream. LUDWIG_ERR_STATE before the first compute. */
int  ludwig_level_gradient_fields_download(const LudwigLevel *level, int which, float *host, size_t bytes);

/* ---- iso-surfaces: the triangles of s = value on one level, extracted on the device (no reference counterpart) ----
 * s per cell: LUDWIG_ISO_DENSITY rho as a download would return it; LUDWIG_ISO_VELOCITY_MAGNITUDE sqrtf((ux ux + uy uy) + uz uz) of
 * vel_field; LUDWIG_ISO_Q_CRITERION / LUDWIG_ISO_VORTICITY_MAGNITUDE Q / sqrtf((wx wx + wy wy) + wz wz) of
 * ludwig_level_gradient_fields_compute(level, vel_field, scale), which the call performs (the gradient fields then hold that result).
 * Surfaces live on the dual grid: a cube is anchored at a cell (x, y, z) of a block, its corner c = dx + 2 dy + 4 dz is the cell
 * (x + dx, y + dy, z + dz), through the anchor block's neighbour row where it lies beyond the block (a periodic entry continues the
 * surface unwrapped). A cube is live iff its anchor block is owned and skip[block] == 0, its anchor's global cell coordinates
 * (8 (map - 1) + x, ...) lie in [cell_lo, cell_hi) per axis, all eight corner blocks exist, no corner is an obstacle cell and all
 * eight s are finite. Each live cube is split into the tetrahedra (0,1,3,7) (0,3,2,7) (0,2,6,7) (0,6,4,7) (0,4,5,7) (0,5,1,7); a corner is
 * inside iff s >= value; 1 or 3 inside corners of a tetrahedron give one triangle, 2 give two, wound (by an integer table) so that the
 * normal points from the inside corners to the outside ones. A vertex on the edge (a, b), a < b as cube corner numbers:
 * t = fminf(fmaxf((value - s_a) / (s_b - s_a), 0), 1); position g_a + t (b - a) in cell units of the level, g_a the anchor's global cell
 * coordinates plus a's offset; attributes rho, ux, uy, uz = q_a + t (q_b - q_a) (rho and vel_field); key = 512 block + cell of a and of
 * b, reference block order (the level must hold fewer than 2^31 / 512 blocks). Float32, no contraction: every cube that shares an edge
 * gives its vertex the same bits. Triangles are ordered by anchor block (reference order), anchor cell x + 8 y + 64 z, tetrahedron,
 * first / second triangle - whatever the internal block order or the scheduling.
 * The buffers belong to the level, are allocated by the first extraction and grow when needed; a level that never extracts allocates
 * and launches nothing. A level created with n_owned < 0 accepts every call and does nothing (0 triangles). */
enum LudwigIsoScalar { LUDWIG_ISO_DENSITY = 0, LUDWIG_ISO_VELOCITY_MAGNITUDE = 1, LUDWIG_ISO_Q_CRITERION = 2,
                       LUDWIG_ISO_VORTICITY_MAGNITUDE = 3 };
#define LUDWIG_ISO_REFUSED     1   /* not an error: more than max_triangles, nothing was emitted */
/* vel_field: LUDWIG_VEL or LUDWIG_VEL_TEMP; scale, value: finite (scale non-zero where the gradient is used); skip: n_blocks bytes in
 * the reference block order, or NULL for none; cell_lo, cell_hi: 3 ints each, cell_lo <= cell_hi; max_triangles >= 0. Counts on the
 * level's stream, brings the per-block counts to the host (one synchronisation), then queues the emission. *n_triangles = the count;
 * when it exceeds max_triangles nothing is emitted, the call returns LUDWIG_ISO_REFUSED and a download gives 0 triangles. */
int  ludwig_level_isosurface_extract(LudwigLevel *level, int which, int vel_field, float scale, float value, const uint8_t *skip,
                                     const int32_t *cell_lo, const int32_t *cell_hi, int64_t max_triangles, int64_t *n_triangles);
/* the last extraction of n triangles: positions [n][3][3] and attributes [n][3][4] floats, keys [n][3][2] int32; the byte counts must
 * be 36 n, 48 n, 24 n. Synchronizes the stream. LUDWIG_ERR_STATE before the first extraction. */
int  ludwig_level_isosurface_download(LudwigLevel *level, float *positions, size_t position_bytes, float *attributes,
                                      size_t attribute_bytes, int32_t *keys, size_t key_bytes);

/* ---- probes: time series of rho and u at points (no reference counterpart) ----
 * A probe set is made over a level array (the batch's). Probe p lives on level level_index[p] (0-based) and has 8 stencil corners
 * c = dx + 2 dy + 4 dz: (reference block index blocks[8p + c], cell cells[8p + c] = x + 8 y + 64 z) - the caller has replaced every
 * corner that is no fluid cell of the level by the base cell - and the weights weights[3p + 0..2] along x, y, z in [0, 1]. A sample
 * of a probe is rho, ux, uy, uz of the level's newest state, trilinear in float32 in one fixed order: x first (corners 0-1, 2-3,
 * 4-5, 6-7), then y, then z, each lerp (1 - w) a + w b. Samples go to a device ring [capacity][n_probes][4] float32, one slot per
 * sampled coarse step. Creating the set makes every probed level store rho after every step (+4 of 216 B per cell where a level
 * elided that store); destroying the set leaves that setting as it is (ludwig_level_set_rho_store(level, 0) undoes it). Entries of
 * `levels` no probe refers to may be null. A probed level may hold at most 2^31 / 512 blocks (32-bit cell indices). */
typedef struct LudwigProbes LudwigProbes;   /* opaque */
int  ludwig_probes_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_probes, const int32_t *level_index,
                          const int32_t *blocks, const int32_t *cells, const float *weights, int32_t capacity, LudwigProbes **out);
/* frees the set, not the levels; it does not touch them, so it may come before or after their destruction */
void ludwig_probes_destroy(LudwigProbes *probes);
/* sample the probes of level level_index after its sub-step t_sub (vel_temp if t_sub is even, vel if odd; rho as a download would
 * return it: an elided store is replayed first), queued on the level's stream. The slot is that of coarse step t_sub >> level_index:
 * the newest slot if it is for that step and this level has not written it, else a new one (its other probes NaN until written).
 * All probed levels must be on one stream here (the NaN fill and the writes of every level are ordered by it): LUDWIG_ERR_STATE
 * otherwise, and when the ring is full. */
int  ludwig_probes_sample(LudwigProbes *probes, int32_t level_index, int64_t t_sub);
/* the samples taken since the last download, oldest first: values [n][n_probes][4], steps [n] (coarse steps); *n_samples = n.
 * Synchronizes the streams of the probed levels, then empties the ring. LUDWIG_ERR_INVALID when n > max_samples. */
int  ludwig_probes_download(LudwigProbes *probes, float *values, int64_t *steps, int32_t max_samples, int32_t *n_samples);
/* ludwig_execute_timestep_batch_observed with one LUDWIG_OBSERVE_PROBES entry (probes, start_step, interval) */
int  ludwig_execute_timestep_batch_probes(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size,
                                          float u_curr, const LudwigStepFlags *flags, LudwigProbes *probes, int64_t start_step,
                                          int32_t interval);

/* ---- surface statistics: time-averaged wall loads per triangle (no reference counterpart) ----
 * A surface set lives on one level (the finest). Triangle i reads its nearest fluid cell (reference block index blocks[i], 0-based,
 * -1 = none found; cell cells[i] = x + 8 y + 64 z), with wall distance wall_dist[i] in lattice units and normal normals[3i + 0..2].
 * A sample evaluates p, tau_x, tau_y, tau_z exactly as ludwig_map_surface_stresses does for that cell (sp->tau, pressure_scale,
 * stress_scale; the other fields of sp are ignored), |tau| = sqrt((tau_x^2 + tau_y^2) + tau_z^2) in float32, and adds to 7 float64
 * sums per triangle, [7][n_tri]: S_p, S_pp, S_tau_x, S_tau_y, S_tau_z, S_|tau|, S_|tau|^2 - each a plain sequential addition of the
 * float32 value (squares of it, exact in float64) in sample order. A triangle with no cell adds zeros. The sums start at zero.
 * Creating the set makes the level store rho after every step (see ludwig_level_set_rho_store). n_tri = 0 is allowed (a rank that
 * owns none of the triangles): samples are counted, nothing is launched. The level may hold at most 2^31 / 512 blocks. */
typedef struct LudwigSurfaceStats LudwigSurfaceStats;   /* opaque */
int  ludwig_surface_stats_create(LudwigLevel *level, int32_t n_tri, const int32_t *blocks, const int32_t *cells, const float *wall_dist,
                                 const float *normals, const LudwigSurfaceParams *sp, LudwigSurfaceStats **out);
/* frees the set, not the level; it does not touch the level, so it may come before or after its destruction */
void ludwig_surface_stats_destroy(LudwigSurfaceStats *stats);
/* zero the sums and the sample count, queued on the level's stream */
int  ludwig_surface_stats_reset(LudwigSurfaceStats *stats);
/* one sample of the state sub-step t_sub wrote (vel_temp if t_sub is even, vel if odd; rho as a download would return it), queued on
 * the level's stream, no host synchronisation */
int  ludwig_surface_stats_accumulate(LudwigSurfaceStats *stats, int64_t t_sub);
/* the sums [7][n_tri] in the caller's triangle order (bytes must be 7 * n_tri * 8) and the number of samples; synchronizes the
 * level's stream */
int  ludwig_surface_stats_download(LudwigSurfaceStats *stats, double *sums, size_t bytes, int64_t *n_samples);

/* a probes and a surface entry of ludwig_execute_timestep_batch_observed, as the three calls below take them */
typedef struct LudwigBatchSamplers {
    LudwigProbes       *probes;
    int64_t             probes_start_step;
    int32_t             probes_interval;
    LudwigSurfaceStats *surface;
    int64_t             surface_start_step;
    int32_t             surface_interval;
} LudwigBatchSamplers;
/* ludwig_execute_timestep_batch_observed with the LUDWIG_OBSERVE_PROBES and LUDWIG_OBSERVE_SURFACE entries of s (s may be NULL) */
int  ludwig_execute_timestep_batch_sampled(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size,
                                           float u_curr, const LudwigStepFlags *flags, const LudwigBatchSamplers *s);

/* ---- force series: the integrated surface loads per sampled coarse step (no reference counterpart) ----
 * A force-series set lives on one level (the finest). Triangle i has the cell, wall distance and normal of a surface set (above), an
 * area area[i] and a moment arm arm[a * n_tri + i] (a = 0..2: centre + offset - moment centre, formed by the caller in float32).
 * A sample evaluates per triangle, in float32 without contraction: p, tau as ludwig_map_surface_stresses does for the cell (zeros
 * without one; sp->tau, pressure_scale, stress_scale, the other fields of sp are ignored), dFp_j = ((-p) n_j) A, dFv_j = tau_j A,
 * dF = dFp + dFv, dM = (ry dF_z - rz dF_y, rz dF_x - rx dF_z, rx dF_y - ry dF_x), covered = |p| > 1e-10f. The nine values Fp(3), Fv(3),
 * M(3) are widened to float64 and added in one fixed balanced tree over the triangles in the caller's order: adjacent pairs halved,
 * +0.0 appended wherever a length is odd, until one value is left (the tree over the triangles zero-padded to the next power of two).
 * The count of covered triangles is an integer sum. No atomics: a record depends on nothing but the state and the triangle order.
 * One record = 9 float64 + 1 int64, kept in a device ring of `capacity` records until it is downloaded.
 * Creating the set makes the level store rho after every step (see ludwig_level_set_rho_store). n_tri = 0 is allowed (a rank that
 * owns none of the triangles): its records are zeros and nothing is launched. The level may hold at most 2^31 / 512 blocks. */
typedef struct LudwigForceSeries LudwigForceSeries;   /* opaque */
int  ludwig_force_series_create(LudwigLevel *level, int32_t n_tri, const int32_t *blocks, const int32_t *cells, const float *wall_dist,
                                const float *normals, const float *area, const float *arm, const LudwigSurfaceParams *sp,
                                int32_t capacity, LudwigForceSeries **out);
/* frees the set, not the level; it does not touch the level, so it may come before or after its destruction */
void ludwig_force_series_destroy(LudwigForceSeries *set);
/* one record of the state sub-step t_sub wrote (vel_temp if t_sub is even, vel if odd; rho as a download would return it), filed
 * under coarse step t_coarse; queued on the level's stream, no host synchronisation. LUDWIG_ERR_STATE when the ring is full. */
int  ludwig_force_series_sample(LudwigForceSeries *set, int64_t t_sub, int64_t t_coarse);
/* the n records taken since the last download, oldest first: sums[9 i + 0..8], covered[i], steps[i]. Synchronizes the level's stream,
 * then empties the ring. LUDWIG_ERR_INVALID when n > max_samples. */
int  ludwig_force_series_download(LudwigForceSeries *set, double *sums, int64_t *covered, int64_t *steps, int32_t max_samples,
                                  int32_t *n_samples);
/* ludwig_execute_timestep_batch_observed with the entries of s (may be NULL) and a LUDWIG_OBSERVE_FORCES entry (fs, start_step, interval) */
int  ludwig_execute_timestep_batch_loads(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size,
                                         float u_curr, const LudwigStepFlags *flags, const LudwigBatchSamplers *s,
                                         LudwigForceSeries *fs, int64_t start_step, int32_t interval);

/* ---- flux planes: integrals over axis-aligned planes per sampled coarse step (no reference counterpart) ----
 * A set is made over a level array. Plane k has the normal axis normal[k] (0, 1, 2: x, y, z) and the points plane_start[k] ..
 * plane_start[k + 1] - 1 (plane_start[0] = 0), in its point order. Point p with valid[p] != 0 lives on level level_index[p] (0-based)
 * and has the probes' stencil: 8 corners c = dx + 2 dy + 4 dz (reference block index blocks[8p + c], cell cells[8p + c] = x + 8 y +
 * 64 z), every corner that is no fluid cell of the level already replaced by the base cell, and weights[3p + 0..2] in [0, 1]. A point
 * with valid[p] == 0 is skipped and its other entries are unread.
 * A sample of a valid point is rho, ux, uy, uz by the probes' trilinear rule (x, then y, then z, every lerp (1 - w) a + w b) in float32
 * without contraction, read from the level's newest state after the coarse step (vel_temp after an even sub-step, vel after an odd
 * one; rho as a download would return it). Its integrands, float32 without contraction, in exactly this operand order:
 *     un = u[normal]   m = rho * un   q = (ux*ux + uy*uy) + uz*uz   c[0..7] = rho, un, m, m*ux, m*uy, m*uz, rho*q, m*q
 * For every (plane, level) pair the valid points of that plane on that level, in point order, are reduced per row: widened to float64
 * and added in the force series' balanced tree (adjacent pairs halved, +0.0 appended wherever a length is odd, no addition once one
 * value is left); the count of points is an int64 sum. A plane's record is the float64 left-to-right sum of its per-level records
 * from the coarsest level to the finest, skipping levels that hold none of its points (counts added as integers); a plane without a
 * valid point gives +0.0 and 0. No atomics: a record depends on nothing but the state and the point order. Each level reduces its own
 * points on its own stream, so no level waits for another. Lattice units throughout: the area element, the plane's direction and every
 * physical scale are the caller's.
 * Per-level records wait in a device ring [capacity][n_planes][n_levels] until they are downloaded. Creating the set makes every level
 * that holds a point store rho after every step (see ludwig_level_set_rho_store). n_planes = 0, or no valid point, is allowed and
 * launches nothing. A level may hold at most 2^31 / 512 blocks; entries of `levels` that no valid point refers to may be NULL. */
typedef struct LudwigFluxPlanes LudwigFluxPlanes;   /* opaque */
int  ludwig_flux_planes_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_planes, const int32_t *plane_start,
                               const int32_t *normal, const int32_t *level_index, const int32_t *blocks, const int32_t *cells,
                               const float *weights, const uint8_t *valid, int32_t capacity, LudwigFluxPlanes **out);
/* frees the set, not the levels; it does not touch them, so it may come before or after their destruction */
void ludwig_flux_planes_destroy(LudwigFluxPlanes *set);
/* between batches: one ring slot filed under coarse step t_coarse; every level that holds points reduces them, as left by its last
 * sub-step of that step ((t_coarse + 1) 2^level_index - 1), on its stream; no host synchronisation. LUDWIG_ERR_STATE when the ring is
 * full. */
int  ludwig_flux_planes_sample(LudwigFluxPlanes *set, int64_t t_coarse);
/* the n samples taken since the last download, oldest first: sums[(i n_planes + k) 8 + 0..7], counts[i n_planes + k], steps[i].
 * Synchronizes the streams of the levels that hold points, adds each plane's levels in order, then empties the ring.
 * LUDWIG_ERR_INVALID when n > max_samples. */
int  ludwig_flux_planes_download(LudwigFluxPlanes *set, double *sums, int64_t *counts, int64_t *steps, int32_t max_samples,
                                 int32_t *n_samples);

/* ---- Fourier modes: weighted running sums of rho and u per cell, for an on-the-fly DFT (no reference counterpart) ----
 * The library knows only a weight table W[n_rows][n_columns] of Float64 (row-major: W[r][m] = weights[r n_columns + m]), copied to the
 * device once; what the columns mean - a window, cosines and sines of chosen frequencies - is the caller's (open_ludwig_amd/modes.py).
 * A set is made over a level array, all of it. Per level with owned blocks it holds 4 n_columns Float64 sums per cell (32 n_columns B):
 * rho, ux, uy, uz per column. One sample of a level with table row r does, per cell of every owned block and every column m,
 *     S[m][q] = S[m][q] + W[r][m] * double(v_q)
 * - one float64 multiply, then one float64 add, never fused - with rho as ludwig_level_download(LUDWIG_RHO) would return it and the
 * velocity buffer sub-step t_sub wrote (vel_temp if t_sub is even, vel if odd): the conventions of ludwig_level_stats_accumulate.
 * Obstacle cells are accumulated like any other, non-finite values propagate by IEEE rules, so acc = acc + W[r][m] * double(v) on the
 * host reproduces every bit. Creating the set makes every level store rho after every step (see ludwig_level_set_rho_store). A level
 * created with n_owned < 0, or without owned blocks, is accepted, counts its samples and does nothing. */
typedef struct LudwigModes LudwigModes;   /* opaque */
/* 1 <= n_columns <= 33, 1 <= n_rows <= 65 536, no null level, one device: LUDWIG_ERR_INVALID otherwise. Everything is checked before
 * anything is allocated, and the set is made for every level or not at all; a failed allocation names the bytes asked for. The sums
 * start at zero. */
int  ludwig_modes_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_columns, int32_t n_rows, const double *weights,
                         LudwigModes **out);
/* frees the set, not the levels */
void ludwig_modes_destroy(LudwigModes *set);
/* zero the sums (queued on each level's stream) and every level's sample count */
int  ludwig_modes_reset(LudwigModes *set);
/* one sample of level level_index (0-based) after its sub-step t_sub with table row `row`, queued on the level's stream, no host
 * synchronisation. Rows come in order with none skipped: row must equal the level's sample count since the last reset
 * (LUDWIG_ERR_STATE, naming both); row < 0 or row >= n_rows: LUDWIG_ERR_INVALID. */
int  ludwig_modes_accumulate(LudwigModes *set, int32_t level_index, int64_t t_sub, int32_t row);
/* the four sums of one column in the reference layout [8,8,8,n_blocks,4] Float64 (rho, ux, uy, uz), reference block order, ghost
 * blocks zero; bytes = 4096 n_blocks 4; *n_samples (may be NULL) = the level's samples since the last reset. Synchronizes the level's
 * stream. */
int  ludwig_modes_download(LudwigModes *set, int32_t level_index, int32_t column, double *host, size_t bytes, int32_t *n_samples);

/* ---- slices: planar grids of points sampled after a coarse step (no reference counterpart) ----
 * A slice set is made over a level array. Point p with valid[p] != 0 lives on level level_index[p] (0-based) and has the probes'
 * stencil: 8 corners c = dx + 2 dy + 4 dz (reference block index blocks[8p + c], cell cells[8p + c] = x + 8 y + 64 z), corner 0 the
 * base cell, every corner that is no fluid cell of the level already replaced by the base cell, and weights[3p + 0..2] in [0, 1].
 * The base cell's block must be owned (its neighbour row reaches every cell a point reads: the corners and their face neighbours).
 * Points with valid[p] == 0 are not read and sample as 0. A sample is rows [n_rows][n_points] floats: rho, ux, uy, uz, |u| =
 * sqrt((ux^2 + uy^2) + uz^2), and with LUDWIG_SLICE_GRADIENT in flags vorticity x, y, z and Q - the trilinear interpolation of the
 * cell values ludwig_level_gradient_fields_compute gives with scales[level]. Interpolation is ludwig_probes_*'s, bit for bit.
 * Entries of `levels` no valid point refers to may be null. */
typedef struct LudwigSlices LudwigSlices;   /* opaque */
enum { LUDWIG_SLICE_GRADIENT = 1 };
int  ludwig_slices_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_points, const int32_t *level_index,
                          const int32_t *blocks, const int32_t *cells, const float *weights, const uint8_t *valid,
                          const float *scales, int32_t flags, LudwigSlices **out);
/* frees the set, not the levels */
void ludwig_slices_destroy(LudwigSlices *slices);
/* sample every point on its level's newest state after coarse step t_coarse: level index li has then finished sub-step
 * t_sub = 2^li (t_coarse + 1) - 1, whose velocity is vel_temp if t_sub is even, vel if odd. One launch per level, on its stream. */
int  ludwig_slices_sample(LudwigSlices *slices, int64_t t_coarse);
/* the last sample: bytes = n_rows * n_points * 4 (n_rows 5, or 9 with LUDWIG_SLICE_GRADIENT). Synchronizes the levels' streams. */
int  ludwig_slices_download(LudwigSlices *slices, float *values, size_t bytes);

/* ---- streamlines: lines traced through the level hierarchy on the device (no reference counterpart) ----
 * A streamline set is made over a level array, all of it: every level must have been created with block_pointer, hold no ghost blocks
 * and lie on one device. The kernel locates a moving point on the hierarchy itself, through each level's dense block_pointer. Float32,
 * no contraction; open_ludwig_amd/streamlines.py (trace_host) restates every bit.
 * A position P is three floats in cell units of level index 0, domain frame (a point of the flow file divided by that level's dx). On
 * level index li the cell coordinate is g = P 2^li - 0.5f. sample(P): from the finest level down, the level holds P iff every g_a is
 * finite, 0 <= g_a and floorf(g_a) <= 8 grid_dim_a - 1 (tested in float), and block_pointer[floorf(g) / 8] > 0; the finest such level
 * is chosen, none: code 1 (a periodic neighbour is not followed). Base cell i0 = floorf(g); an obstacle cell: code 2. Weights
 * g - floorf(g); corners i0 + {0,1}^3, c = dx + 2 dy + 4 dz, each found through block_pointer; a corner outside the grid, in an absent
 * block or in an obstacle cell is replaced by the base cell; rho, ux, uy, uz trilinear as ludwig_probes_* (x, then y, then z).
 * A line from seed P with sign s: k = 0; loop: (rho, u, li) = sample(P), on failure the line ends with that code and P is no vertex;
 * vertex k = (P, rho, u, li); k == max_steps: code 0; m = sqrtf((ux ux + uy uy) + uz uz), !(m >= min_speed): code 3;
 * h = step 2^-li; Pm = P + (0.5f h) (s u / m) per component (divide, times s, times 0.5f h, add); um = sample(Pm) (its code ends the
 * line), mm likewise, !(mm >= min_speed): code 3; P = P + h (s um / mm); k += 1. A line has 0 .. max_steps + 1 vertices. */
typedef struct LudwigStreamlines LudwigStreamlines;   /* opaque */
enum { LUDWIG_STREAM_END_STEPS = 0, LUDWIG_STREAM_END_OUTSIDE = 1, LUDWIG_STREAM_END_OBSTACLE = 2, LUDWIG_STREAM_END_SLOW = 3 };
/* seeds: 3 n_lines floats; sign: n_lines floats, each 1 or -1; step > 0 in cells of the level a step starts on; max_steps >= 0.
 * Uploads every level's block_pointer (in the library's block order) and allocates [n_lines][max_steps + 1] records of 8 floats
 * (x, y, z, rho, ux, uy, uz, level index as a float), counts and codes. n_lines = 0 is allowed (seeds, sign may be NULL) and never
 * launches. LUDWIG_ERR_STATE: a level without block_pointer or with ghost blocks, or levels on different devices; LUDWIG_ERR_INVALID:
 * step <= 0 or not finite, max_steps < 0, more than 2^31 - 1 records, a sign that is not +-1, n_levels not in 1..30. */
int  ludwig_streamlines_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_lines, const float *seeds, const float *sign,
                               float step, float min_speed, int32_t max_steps, LudwigStreamlines **out);
/* frees the set, not the levels */
void ludwig_streamlines_destroy(LudwigStreamlines *set);
/* trace every line through every level's newest state after coarse step t_coarse (level index li: sub-step 2^li (t_coarse + 1) - 1,
 * vel_temp if that is even, vel if odd; rho as a download would return it). One launch on the first level's stream, ordered after
 * everything queued on the other levels' streams, which in turn wait for it. Writes only the set's own buffers. */
int  ludwig_streamlines_trace(LudwigStreamlines *set, int64_t t_coarse);
/* the last trace: counts and codes [n_lines] int32, vertices [n_lines][max_steps + 1][8] floats of which the first max(count)
 * records of each line are brought down (the rest of the caller's array is left alone); bytes = the size of the whole vertex array.
 * Synchronizes. LUDWIG_ERR_STATE before the first trace. */
int  ludwig_streamlines_download(LudwigStreamlines *set, int32_t *counts, int32_t *codes, float *vertices, size_t bytes);

/* ---- volume images: rays marched through the level hierarchy on the device and composited (no reference counterpart) ----
 * A render set is made over a level array, all of it, under the streamline sets' conditions (block_pointer, no ghost blocks, one device).
 * Float32, no contraction, every product, sum, quotient and sqrtf rounded on its own; only + - x / sqrtf floorf, ldexpf (a scaling by
 * a power of two, exact), comparisons and int <-> float conversions; open_ludwig_amd/render.py (render_host) restates every bit. Positions are the streamlines' P.
 * Camera: eye, corner (the centre of pixel (0, 0), the top-left one), du, dv (the steps per pixel column and row), dir (a unit vector),
 * perspective (0 or 1), built by the host in float64 and cast once. Pixel (i, j), column i, row j: T_a = (corner_a + (float)i du_a) +
 * (float)j dv_a. Orthographic: O = T, D = dir. Perspective: O = eye, d = T - O, m = sqrtf((dx dx + dy dy) + dz dz), D = d / m; m not > 0
 * or not finite: code MISS.
 * Box: lo_a = 0, hi_a = (float)(8 grid_dim_a of level index 0) + 0.5f. t0 = 0, t1 = +inf; per axis x, y, z: D_a == 0: MISS unless
 * lo_a <= O_a <= hi_a; else a = (lo_a - O_a) / D_a, b = (hi_a - O_a) / D_a, t0 = fmaxf(t0, fminf(a, b)), t1 = fminf(t1, fmaxf(a, b)).
 * !(t0 < t1): MISS.
 * s(P) is the streamlines' sample(P) applied to one per-cell scalar of the chosen level: the finest level whose active blocks hold the
 * base cell (none: OUTSIDE), an obstacle base cell: OBSTACLE, weights g - floorf(g), a corner outside the grid, in an absent block or
 * in an obstacle cell takes the base cell's value, trilinear x, then y, then z, each lerp (1 - w) a + w b. The scalars are those of
 * LUDWIG_ISO_* from the same sources: rho; sqrtf((ux ux + uy uy) + uz uz) per cell, then interpolated; Q and sqrtf((wx wx + wy wy) +
 * wz wz) of ludwig_level_gradient_fields_compute on the level's newest velocity buffer with scales[level index].
 * March: t = t0, T = 1, (R, G, B) = 0, n = 0. Loop: !(t < t1): code EXIT; n == max_samples: code SAMPLES; P_a = O_a + t D_a;
 * (kind, s, li) = sample(P), n += 1, li = 0 when OUTSIDE; delta = step 2^-li; OBSTACLE: shade the body, code BODY; found and s == s:
 * x = fminf(fmaxf((s - lo) inv, 0), 1) with inv = 1.0f / (hi - lo) (fmaxf gives 0 for a NaN), e = table[(int)(x 255.0f + 0.5f)] =
 * (r, g, b, kappa), alpha = fminf(kappa delta, 1.0f), w = T alpha, R = R + w r (G, B alike), T = T - w, T < t_min: code OPAQUE;
 * t = t + delta. After the loop, unless BODY: R = R + T bg_r (G, B alike). A = 1 - T.
 * Body: o(e) = 1 if the base cell's face neighbour at e on its own level is an obstacle cell of an active block, else 0 (outside the
 * grid, absent block: 0); n_a = o(-e_a) - o(+e_a), nn = n.n; nn == 0: shade = 1, else c = -((n_x D_x + n_y D_y) + n_z D_z) /
 * sqrtf((float)nn), shade = 0.3f + 0.7f fmaxf(c, 0.0f). R = R + T (body_r shade) (G, B alike), then T = 0.
 * Per pixel: RGBA floats, an int32 end code and the int32 sample count n. A pixel is written by one lane: no atomics. */
typedef struct LudwigRender LudwigRender;   /* opaque */
enum { LUDWIG_RENDER_EXIT = 0, LUDWIG_RENDER_MISS = 1, LUDWIG_RENDER_BODY = 2, LUDWIG_RENDER_OPAQUE = 3, LUDWIG_RENDER_SAMPLES = 4 };
/* uploads every level's block_pointer (in the library's block order) and allocates the buffers of max_pixels pixels (24 bytes each).
 * Errors as ludwig_streamlines_create; max_pixels not in 1..2^31 - 1: LUDWIG_ERR_INVALID. */
int  ludwig_render_create(LudwigLevel *const *levels, int32_t n_levels, int64_t max_pixels, LudwigRender **out);
/* frees the set, not the levels */
void ludwig_render_destroy(LudwigRender *set);
/* one image of scalar `which` (enum LudwigIsoScalar) of every level's newest state after coarse step t_coarse (the buffers
 * ludwig_streamlines_trace reads). scales: n_levels floats, the gradient fields' scale per level (read for every scalar). camera: 16
 * floats - eye, corner, du, dv, dir, one unused. params: 10 floats - step, lo, hi, t_min, background r g b, body r g b. table: 256
 * entries r, g, b, kappa (extinction per coarse cell length). For Q and |omega| every level's gradient fields are computed first, on its
 * stream, into the level's own gradient buffers (as ludwig_level_isosurface_extract does); |u| and |omega| go into buffers of the set.
 * Then one launch on the first level's stream, ordered against the other levels' streams as ludwig_streamlines_trace is. Apart from
 * the gradient buffers only the set's own buffers are written. Refused before anything is launched, LUDWIG_ERR_INVALID: a null array,
 * t_coarse < 0, an unknown `which`, perspective not 0 or 1, width or height < 1 or width height > max_pixels, step, t_min or a scale
 * not finite or <= 0, hi not > lo, max_samples < 1. */
int  ludwig_render_image(LudwigRender *set, int64_t t_coarse, int which, const float *scales, const float *camera, int perspective,
                         int32_t width, int32_t height, const float *params, int32_t max_samples, const float *table);
/* the last image: rgba [height][width][4] floats, codes and samples [height][width] int32; bytes = the size of rgba. Synchronizes.
 * LUDWIG_ERR_STATE before the first image. */
int  ludwig_render_download(LudwigRender *set, float *rgba, int32_t *codes, int32_t *samples, size_t bytes);

/* ---- tracers: particles advected through the level hierarchy on the device, inside a batch (no reference counterpart) ----
 * A tracer set is made over a level array, all of it, under the streamline sets' conditions (block_pointer, no ghost blocks, one device).
 * Float32, no contraction; open_ludwig_amd/tracers.py (advance_host, snapshot_host) restates every bit. Positions are the streamlines' P.
 * sample_u(P) is the streamlines' sample(P) returning u and the level index only: rho is never read, and no level's rho policy changes.
 * The set holds n_seeds x generations slots; slot g n_seeds + s has P[3] and an int32 state: -1 empty, 0 alive, 1 outside, 2 obstacle
 * (the LUDWIG_STREAM_END_* codes), 3 non-finite. The set counts its advances k = 0, 1, ... on the host. Advance k behind coarse step t reads
 * every level's newest velocity after t (the buffer ludwig_streamlines_trace reads):
 *   if k % release_every == 0, generation (k / release_every) % generations is the released one;
 *   every alive slot not of the released generation: u = sample_u(P); Pm = P + (0.5f dt) u per component; um = sample_u(Pm); a failed
 *   sample: the state takes its code, P stays; Pn = P + dt um; a non-finite component: state 3, P stays; else P = Pn. A dead or empty
 *   slot is not touched;
 *   the released generation's slots get P = seed, state 0: overwritten whatever they held, not advanced and not sampled.
 * Snapshot (changes no state): rec[slot][8] = x, y, z, ux, uy, uz, level index, code. An alive slot is sampled at P: code 0 with values,
 * or zeros, level -1 and the failing code; any other slot: zeros, level -1, code = its state. The position is always written.
 * A slot is owned by one lane group: no atomics, no compaction, the result depends on no scheduling. */
typedef struct LudwigTracers LudwigTracers;   /* opaque */
enum { LUDWIG_TRACER_EMPTY = -1, LUDWIG_TRACER_ALIVE = 0, LUDWIG_TRACER_OUTSIDE = 1, LUDWIG_TRACER_OBSTACLE = 2, LUDWIG_TRACER_NONFINITE = 3 };
/* seeds: 3 n_seeds floats; generations >= 1, release_every >= 1 (in advances), dt > 0 and finite (coarse steps per advance, as a float).
 * n_seeds = 0 is allowed (seeds may be NULL) and never launches. Errors as ludwig_streamlines_create; more than 2^28 - 1 slots:
 * LUDWIG_ERR_INVALID. */
int  ludwig_tracers_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_seeds, const float *seeds, int32_t generations,
                           int32_t release_every, float dt, LudwigTracers **out);
/* frees the set, not the levels */
void ludwig_tracers_destroy(LudwigTracers *set);
/* one advance outside a batch, behind coarse step t_coarse: one launch on the first level's stream, ordered after everything queued on the
 * other levels' streams, which in turn wait for it. Writes only the set's own buffers. */
int  ludwig_tracers_advance(LudwigTracers *set, int64_t t_coarse);
/* snapshot on the newest velocity after coarse step t_coarse, ordered as an advance */
int  ludwig_tracers_snapshot(LudwigTracers *set, int64_t t_coarse);
/* the last snapshot: records [n_seeds generations][8] floats, bytes = their size; n_advances (may be NULL): advances so far.
 * Synchronizes. LUDWIG_ERR_STATE before the first snapshot. */
int  ludwig_tracers_download(LudwigTracers *set, float *records, size_t bytes, int64_t *n_advances);
/* ludwig_execute_timestep_batch_observed with the entries of samplers (may be NULL), a LUDWIG_OBSERVE_FORCES entry (forces,
 * force_start_step, force_interval) and a LUDWIG_OBSERVE_TRACERS entry (tracers, start_step, interval) */
int  ludwig_execute_timestep_batch_tracers(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size, float u_curr,
                                           const LudwigStepFlags *flags, const LudwigBatchSamplers *samplers, LudwigForceSeries *forces,
                                           int64_t force_start_step, int32_t force_interval, LudwigTracers *tracers, int64_t start_step,
                                           int32_t interval);

/* ---- warm start: a level filled from another hierarchy's flow, resampled on the device (no reference counterpart: the reference starts
 * every run from rest, init_eq! src/main.jl:109-134) ----
 * What is carried over is the macroscopic state, rho and u; the populations restart at their equilibrium, so the non-equilibrium part
 * (the viscous stress) is rebuilt by the first steps. A level initialised this way is NOT what a continued run would hold, not even on
 * an identical grid. A cell that a finer source level covers takes the finer level's interpolated value (sample(P) chooses the finest).
 *
 * A flow source is a level hierarchy reduced to what the streamlines' sample(P) reads: per level the grid dimensions, the dense 1-based
 * block_pointer, obstacle, rho and ONE velocity array, in device memory of its own (17 B per cell; no populations; no LudwigLevel).
 * Float32, no contraction; open_ludwig_amd/warm_start.py (init_host) restates every bit.
 *
 * ludwig_level_init_from_source: for every cell (x, y, z) of every block the level holds (ghost blocks included), with the global cell
 * coordinates gc_a = 8 (map_a - 1) + x_a of its block row: P_a = a_a ((float)gc_a + 0.5f) + b_a - the sum in brackets is exact (a level
 * with more than 2^23 cells per axis is refused), the product and the sum are rounded once each; map = a_x, a_y, a_z, b_x, b_y, b_z, so P
 * is a position in cell units of the source's level index 0. (code, q, li) = the streamlines' sample(P) on the source, with rho. If code
 * is 0 and all four q are finite, with s = vel_scale: rho' = 1.0f + (q_rho - 1.0f) (s s), u'_k = q_k s; otherwise rho', u' = fallback
 * (rho, ux, uy, uz). An obstacle cell of the level gets rho' = 1, u' = 0. Stored: rho = rho', vel = vel_temp = u', f = f_temp =
 * calculate_equilibrium(rho', u', w_k, c_k) (src/physics_utils.jl:34-39) for the 27 k; on a level with temporal storage f_old, rho_old and
 * vel_old get the same values. counts (may be NULL), over the non-obstacle cells of the level: [0] found, [1] outside the source, [2] in
 * a source obstacle cell, [3] found but not finite, then [4 + li] the found cells per source level - integer sums, whatever the order.
 * Afterwards the level is in the state ludwig_level_upload of these arrays would leave it in: nothing older survives in a record, an
 * elided rho store or an aliased saved state. Queued on the level's stream; with counts one small download and one synchronisation. A
 * level created with n_owned < 0 accepts the call and does nothing (counts zero). */
typedef struct LudwigFlowSource LudwigFlowSource;   /* opaque */
/* Host arrays per level, level index 0 first, in the reference layout and block order: grid_dims[3 li + a] blocks per axis,
 * block_pointer[li] [dim_x,dim_y,dim_z] 1-based with 0 = absent, obstacle[li] [8,8,8,nb] u8, rho[li] [8,8,8,nb] f32, vel[li] [8,8,8,nb,3]
 * f32 with nb = n_blocks[li]. LUDWIG_ERR_INVALID: a null array, n_levels not in 1..30, a block_pointer entry outside 0..nb, more than
 * 2^24 cells per axis. */
int  ludwig_flow_source_create(int device, int32_t n_levels, const int32_t *grid_dims, const int32_t *n_blocks,
                               const int32_t *const *block_pointer, const uint8_t *const *obstacle, const float *const *rho,
                               const float *const *vel, LudwigFlowSource **out);
/* A device-to-device copy of every level's newest state after coarse step t_coarse (level index li: sub-step 2^li (t_coarse + 1) - 1,
 * vel_temp if that is even, vel if odd; rho as a download would return it), under the streamline sets' conditions (block_pointer, no
 * ghost blocks, one device; errors as ludwig_streamlines_create). The copies are queued on the levels' streams behind their steps and
 * waited for; the source shares no memory with the levels, which may step on or be destroyed. */
int  ludwig_flow_source_from_levels(LudwigLevel *const *levels, int32_t n_levels, int64_t t_coarse, LudwigFlowSource **out);
/* frees the source; levels initialised from it keep what they got */
void ludwig_flow_source_destroy(LudwigFlowSource *src);
/* map: 6 floats, fallback: 4 floats, counts: 4 + (levels of the source) int64 or NULL. Refused before anything is launched or written,
 * LUDWIG_ERR_INVALID: a null level, source, map or fallback; a map or fallback entry that is not finite; a_a <= 0; vel_scale not finite
 * or <= 0; more than 2^23 cells per axis. LUDWIG_ERR_STATE: the source is on another device than the level. */
int  ludwig_level_init_from_source(LudwigLevel *level, const LudwigFlowSource *src, const float *map, float vel_scale,
                                   const float *fallback, int64_t *counts);

/* ---- subgrid model: the WALE eddy viscosity the step collides with, and its time-averaged measures (no reference counterpart for the
 * output; the model is perform_timestep_v2!'s, src/physics_kernels.jl:251-300) ----
 * Per cell of the blocks this device owns, from one velocity buffer u: the gradient in lattice units g_ij = 0.5f (u_i(+e_j) - u_i(-e_j))
 * with the neighbour value of get_velocity_neighbor (no block across a face: the cell's own value), then the step's WALE block restated
 * operation by operation in float32 up to nu_t = max(nu_model, nu_sgs_background), and |S|^2 = 2 OP2. Evaluated on the buffer sub-step
 * t_sub wrote, nu_t is bit for bit the value sub-step t_sub + 1 collides with. The code says which branch gave it: 0 OP1 <= 1e-12,
 * 1 denom <= 1e-12 (both: nu_t = nu_sgs_background), 2 the model is evaluated and the background floor wins, 3 the model is above the
 * floor. Obstacle cells give 0 and code 0 and add +0.0 to the sums.
 * c_wale and nu_sgs_background are not arguments: a level records the two values every step call gives it (LudwigStepFlags), and these
 * calls evaluate with them. LUDWIG_ERR_STATE on a level with owned blocks that has never been stepped.
 * The field buffer (8 B per cell) is allocated by the first compute, the sums (24 B per cell) by the first reset; a level that calls
 * neither allocates and launches nothing. A level created with n_owned < 0 accepts every call and does nothing. */
enum LudwigSubgridField { LUDWIG_SUBGRID_NU = 0, LUDWIG_SUBGRID_CODE = 1 };   /* nu_t; the code as a float */
/* vel_field: LUDWIG_VEL or LUDWIG_VEL_TEMP. Reads vel, obstacle and the neighbour table only; queued on the level's stream, no host
 * synchronisation. */
int  ludwig_level_subgrid_fields_compute(LudwigLevel *level, int vel_field);
/* the last computed field in the reference layout [8,8,8,n_blocks] Float32, reference block order, ghost blocks zero; bytes =
 * 2048 n_blocks. Synchronizes the stream. LUDWIG_ERR_STATE before the first compute. */
int  ludwig_level_subgrid_fields_download(const LudwigLevel *level, int which, float *host, size_t bytes);
/* Sums in double precision: S_nu += nu_t, S_nunu += nu_t nu_t, S_eps += nu_t |S|^2, the float32 values widened first (a product of two
 * floats is exact in double); each a plain sequential addition per cell in sample order, so a float64 replay reproduces every bit. */
enum LudwigSubgridSum { LUDWIG_SUBGRID_SUM_NU = 0, LUDWIG_SUBGRID_SUM_NUNU = 1, LUDWIG_SUBGRID_SUM_EPS = 2 };
/* allocate on the first call, zero the sums, n = 0 (queued on the level's stream) */
int  ludwig_level_subgrid_stats_reset(LudwigLevel *level);
/* add one sample from the velocity buffer sub-step t_sub wrote (vel_temp if t_sub is even, vel if odd). Queued on the level's stream, no
 * host synchronisation. LUDWIG_ERR_STATE before the first reset. */
int  ludwig_level_subgrid_stats_accumulate(LudwigLevel *level, int64_t t_sub);
/* one sum in the reference layout [8,8,8,n_blocks] Float64, reference block order, ghost blocks zero; bytes = 4096 n_blocks; *n_samples
 * (may be NULL) = samples since the last reset. Synchronizes the stream. LUDWIG_ERR_STATE before the first reset. */
int  ludwig_level_subgrid_stats_download(const LudwigLevel *level, int which, double *host, size_t bytes, int64_t *n_samples);

/* ---- halo exchange helpers (no reference counterpart: the reference is single-device) ---- */
/* dst[i] = field[index[i]] / field[index[i]] = src[i]; index, dst, src are DEVICE pointers, index holds element
 * offsets into the field in the reference layout. hip_stream: the stream to queue on (hipStream_t), NULL = the
 * level's stream - the exchange normally runs on its own stream so that it overlaps the interior update. */
int  ludwig_halo_pack(const LudwigLevel *level, int field, const int64_t *index_dev, int64_t n,
                      float *dst_dev, void *hip_stream);
int  ludwig_halo_unpack(LudwigLevel *level, int field, const int64_t *index_dev, int64_t n,
                        const float *src_dev, void *hip_stream);

/* ---- multi-GPU: communicator, halo plan, exchange, distributed step (no reference counterpart: the reference is single-device,
 * src/main.jl:75; its caller for this path is execute_timestep_batch!, src/solver_control.jl:145-165, which a multi-GPU host calls
 * once per rank) ----
 * One process per GPU. RCCL (ncclSend / ncclRecv, point-to-point over xGMI) is resolved at run time from the librccl already mapped
 * into the process (e.g. PyTorch's) so that two copies never coexist; otherwise librccl.so(.1) is opened from the loader's path
 * (LUDWIG_RCCL_LIB overrides). The library does not link against it: single-GPU users never load it. */
typedef struct LudwigComm LudwigComm;
#define LUDWIG_UNIQUE_ID_BYTES 128
/* ncclGetUniqueId: called by ONE rank; the host carries the 128 bytes to the others by its own means (MPI, a file, a socket). */
int  ludwig_comm_unique_id(void *id_out);
/* ncclCommInitRank on `device` (collective over the `world` ranks). */
int  ludwig_comm_create(const void *unique_id, int rank, int world, int device, LudwigComm **out);
void ludwig_comm_destroy(LudwigComm *comm);
/* in-place all-reduce of a few Float32 scalars over the communicator (diagnostics: rho_min, force sums); op: 0 sum, 2 max, 3 min;
 * buf is a HOST array. NaN in any rank's value gives NaN for min / max (the reference's minimum() propagates it). */
int  ludwig_comm_allreduce_f32(LudwigComm *comm, float *buf, int32_t n, int32_t op);

/* The ghost elements of one level this rank receives after a step and the owned elements it sends, per peer and per logical field
 * GROUP: 0 = populations (f or f_temp), 1 = velocity (vel or vel_temp), 2 = f_post_collision, 3 = rho. For every group the lists of
 * all peers are concatenated in peer order: index[count[0] + ... + count[p-1] ...] belongs to peer p. Element offsets are in the
 * REFERENCE layout of the level (cell + 512 b + 512 n_blocks k); a peer's receive list and the matching send list of that peer name
 * the same elements in the same order. Everything is translated and uploaded here, once: a step then costs three enqueue calls. */
#define LUDWIG_HALO_GROUPS 4
typedef struct LudwigHaloPlanDesc {
    int32_t n_peers;
    const int32_t *peer_ranks;                          /* [n_peers] rank in the communicator; this rank itself = a device copy   */
    const int64_t *send_count[LUDWIG_HALO_GROUPS];      /* [n_peers] each; NULL = the group is empty                              */
    const int64_t *recv_count[LUDWIG_HALO_GROUPS];
    const int64_t *send_index[LUDWIG_HALO_GROUPS];      /* HOST arrays, concatenated over peers                                   */
    const int64_t *recv_index[LUDWIG_HALO_GROUPS];
} LudwigHaloPlanDesc;
typedef struct LudwigHaloPlan LudwigHaloPlan;
/* comm may be NULL when every peer is this rank itself (periodic wrap onto the own brick; tests). */
int  ludwig_halo_plan_create(LudwigLevel *level, LudwigComm *comm, const LudwigHaloPlanDesc *desc, LudwigHaloPlan **out);
void ludwig_halo_plan_destroy(LudwigHaloPlan *plan);

/* One exchange: for i < n: group groups[i] of the plan moves field fields[i] (a LudwigField with as many components as the group).
 * Queued on the plan's own HIGH-priority stream behind everything queued on the level's stream so far: pack (one kernel per group)
 * -> ncclGroupStart, one ncclSend / ncclRecv per peer and group, ncclGroupEnd -> unpack. Returns at once; nothing queued on the
 * level's stream LATER waits for it until ludwig_halo_wait, so work that reads no ghost can run under it. */
int  ludwig_halo_exchange(LudwigHaloPlan *plan, int32_t n, const int32_t *groups, const int32_t *fields);
/* everything queued on the level's stream after this call runs after the plan's last exchange */
int  ludwig_halo_wait(LudwigHaloPlan *plan);
/* For hosts that carry the messages themselves (a transport other than RCCL; the one-GPU rehearsals over gloo): the two halves of an
 * exchange on `hip_stream` (NULL = the level's), and the message buffers (DEVICE pointers, Float32, peers concatenated as in the plan). */
int  ludwig_halo_plan_pack(LudwigHaloPlan *plan, int32_t group, int32_t field, void *hip_stream);
int  ludwig_halo_plan_unpack(LudwigHaloPlan *plan, int32_t group, int32_t field, void *hip_stream);
int  ludwig_halo_plan_buffers(const LudwigHaloPlan *plan, int32_t group, void **send_dev, int64_t *n_send, void **recv_dev, int64_t *n_recv);
/* In-stream mode: ludwig_halo_exchange queues pack, transfer and unpack on the LEVEL's stream instead of the plan's own - no overlap
 * with what the level launches next, and no cross-stream hand-over either (each costs the device tens of idle microseconds: more than
 * the whole exchange of a small level; nested levels take 2^(l-1) steps per coarse step). ludwig_halo_wait is then a no-op. The Python
 * host chooses it for levels below 8 192 owned blocks (LUDWIG_HALO_IN_STREAM_BELOW). Same messages, same bits. */
int  ludwig_halo_plan_in_stream(LudwigHaloPlan *plan, int enable);
/* Benchmarks: with timing on, every ludwig_halo_exchange is bracketed by events on the plan's stream (the span includes waiting beside
 * whatever the device is busy with); ludwig_halo_plan_exchange_ms returns the spans of the exchanges finished since the last call
 * (at most `max`, oldest first; call after a device synchronize). */
int  ludwig_halo_plan_timing(LudwigHaloPlan *plan, int enable);
int  ludwig_halo_plan_exchange_ms(LudwigHaloPlan *plan, float *ms_out, int32_t max, int32_t *n_out);

/* perform_timestep_v2! (src/physics_v2.jl:26-97) of a level whose blocks are spread over ranks, with the exchange hidden behind
 * compute: interior blocks of step t_sub (they read no ghost) -> wait for the exchange of the previous step -> boundary blocks
 * -> [f_post_collision halo of the links that reach across a cut, Bouzidi correction] -> exchange of this step's output (groups 0
 * and 1: the populations and velocity buffer step t_sub wrote), left in flight under the next call's interior blocks.
 * ludwig_halo_wait (or the next call) joins it; ludwig_sync waits for the device. Same arguments as ludwig_step. */
int  ludwig_step_distributed(LudwigLevel *level, LudwigHaloPlan *plan, const LudwigLevel *parent, int64_t t_sub, float u_curr,
                             float parent_tau, float temporal_weight, const LudwigStepFlags *flags);

/* ---- introspection for benchmarks ---- */
typedef struct LudwigLevelInfo {
    int32_t n_blocks, n_owned;
    int32_t n_fast_blocks;        /* owned blocks with all 26 neighbours present (no edge / interface patching)   */
    int32_t n_general_blocks;
    int32_t n_boundary_cells;
    int32_t has_temporal_storage, has_post_collision;
    int32_t n_xrun_blocks;        /* of the fast blocks: how many the current LUDWIG_PART_ALL order steps next to an x
                                     neighbour in the same workgroup (face column through LDS instead of global memory) */
    int64_t device_bytes;
} LudwigLevelInfo;
int  ludwig_level_info(const LudwigLevel *level, LudwigLevelInfo *info);

#ifdef __cplusplus
}
#endif
#endif /* LUDWIG_HIP_H */
