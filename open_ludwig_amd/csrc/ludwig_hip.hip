// libludwig_hip.so - C ABI (include/ludwig_hip.h) over the gfx950 kernels in kernels.hpp.
// Host side only: memory ownership, block classification, work lists, launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ludwig_hip.h"
#include "device_memory.hpp"
#include "kernels.hpp"

using namespace lw;

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define LW_HIP(call)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) return fail(LUDWIG_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Every release of device memory, events and streams in this file happens in these three policies (device_memory.hpp).
struct HipMem {
    static int alloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void release(void *p) { (void)hipFree(p); }
};
struct HipEventOps {
    static int create(hipEvent_t *ev, unsigned flags = hipEventDisableTiming) { return (int)hipEventCreateWithFlags(ev, flags); }
    static int destroy(hipEvent_t ev) { return (int)hipEventDestroy(ev); }
};
struct HipStreamOps {
    static int create(hipStream_t *st, unsigned flags, int priority = 0) { return (int)hipStreamCreateWithPriority(st, flags, priority); }
    static int destroy(hipStream_t st) { return (int)hipStreamDestroy(st); }
};
template <class T> using Dev = lw::DeviceArray<T, HipMem>;
using HipEvent = lw::DeviceHandle<hipEvent_t, HipEventOps>;
using HipStream = lw::DeviceHandle<hipStream_t, HipStreamOps>;

constexpr int N_PARTS = 3, N_CLASSES = 3;   // class 1 = blocks with a missing neighbour (GENERAL instantiation), 2 = all-neighbour blocks; 0 unused
constexpr int XRUN = 4, XRUN_MAX = 4;       // waves per workgroup = blocks of an x-run (8 and 16 were tried in rounds 1-2: slower)

// ---- switches: every getenv of this file. INTEGRATION.md ("Environment switches") lists exactly these names with the same read times ----------
namespace env {

bool is_set(const char *name) { return getenv(name) != nullptr; }
int flag(const char *name) { const char *e = getenv(name); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }      // 0 / 1, -1 = unset

// LUDWIG_MERGE_CLASSES=0/1: never / always one launch for both block classes (-1: by size). Per level creation and per set_order.
int merge_classes() { return flag("LUDWIG_MERGE_CLASSES"); }
// LUDWIG_REFERENCE_BLOCK_ORDER: device arrays keep the caller's block order. Per level creation.
bool reference_block_order() { return is_set("LUDWIG_REFERENCE_BLOCK_ORDER"); }
// LUDWIG_WIDE_ADDR: 64-bit per-lane addresses at any level size. Per level creation.
bool wide_addr() { return is_set("LUDWIG_WIDE_ADDR"); }
// LUDWIG_FULL_POST_COLLISION: f_post_collision stored in every block, as the reference. Per level creation.
bool full_post_collision() { return is_set("LUDWIG_FULL_POST_COLLISION"); }
// LUDWIG_POST_ROWS=0: f_post_collision stored in whole blocks with a reader, not by x-rows. Per level creation.
bool post_rows_off() { const char *e = getenv("LUDWIG_POST_ROWS"); return e && e[0] == '0'; }
// LUDWIG_EAGER_RHO: every step stores rho. Per process (first step).
bool eager_rho() { static const bool v = is_set("LUDWIG_EAGER_RHO"); return v; }
// LUDWIG_NO_IFACE_AHEAD: the child-side interface pass produces one sub-step's values at a time. Per call (every such pass).
bool no_iface_ahead() { return is_set("LUDWIG_NO_IFACE_AHEAD"); }
// LUDWIG_RHO_OLD_COPY: copy_to_old!'s rho copy stays a copy inside a batch (not fused into the step). Per call (every save in a batch).
bool rho_old_copy() { return is_set("LUDWIG_RHO_OLD_COPY"); }
// LUDWIG_BATCH_SERIAL: a batch keeps every level on the caller's stream. Per process (first batch of more than one level).
bool batch_serial() { static const bool v = is_set("LUDWIG_BATCH_SERIAL"); return v; }
// LUDWIG_CHILD_SIDE_IFACE: level streams run the interface pass on the child's stream, not the parent's. Per process (first batch).
bool child_side_iface() { static const bool v = is_set("LUDWIG_CHILD_SIDE_IFACE"); return v; }
// LUDWIG_IFACE_HOIST=0/1: a middle level's child-side pass never / always ahead of its wait (-1: by size). Per process (first hoist).
int iface_hoist() { static const int v = flag("LUDWIG_IFACE_HOIST"); return v; }
// LUDWIG_LEVEL_STREAM_PRIORITY=0/2: level streams all at one priority / graded (1, unset: the finest level highest). Per call (every batch).
int level_stream_priority() { const char *e = getenv("LUDWIG_LEVEL_STREAM_PRIORITY"); return e ? atoi(e) : 1; }
// LUDWIG_RCCL_LIB: path of the RCCL library, tried after one already mapped in the process. Per process (first communicator).
const char *rccl_lib() { return getenv("LUDWIG_RCCL_LIB"); }
// LUDWIG_HALO_SELF_VIA_RCCL: a rank's messages to itself go through RCCL too. Per halo plan created.
bool halo_self_via_rccl() { return is_set("LUDWIG_HALO_SELF_VIA_RCCL"); }
// LUDWIG_HALO_TRACE: host microseconds of every exchange call on stderr. Per process (first exchange).
bool halo_trace() { static const bool v = is_set("LUDWIG_HALO_TRACE"); return v; }
// LUDWIG_RECORD_STEP=0: plain levels step on the f path too (the record step off, same bits). Per call (every step).
bool record_step_off() { return flag("LUDWIG_RECORD_STEP") == 0; }
// LUDWIG_RECORD_ORDER=0/1: the record step launches in the f path's order / with the 8 planes of a run on one XCD (unset: 1). Per
// level, when its record work list is built (first record step after create or set_order).
int record_order() { const int v = flag("LUDWIG_RECORD_ORDER"); return v < 0 ? 1 : v; }

}  // namespace env

}  // namespace

struct LudwigLevel {
    int device = 0;
    hipStream_t stream = nullptr;         // borrowed: the caller's (ludwig_level_set_stream) or own_stream
    int level_id = 1, n_blocks = 0, n_owned = 0;
    float tau = 1.0f;
    int gdx = 0, gdy = 0, gdz = 0;
    // Storage. The caller's arrays are [8,8,8,n_blocks,K], population-major (reference src/blocks.jl:118-150); the device arrays are
    // BLOCK-major: element (cell, block b, component k) at ((b * K + k) * 512 + cell) - the 27 populations of a block are one
    // contiguous 54-KiB piece. With the reference's layout the step is 27 + 27 concurrent streams n_blocks x 2 KiB apart, and at
    // some distances - 64.5, 65.75, 68, 76-77 ... MiB for boxes around 256^3, far denser for the small levels of a nested case -
    // they load MI355X's memory system unevenly: 5-30 % of the step, decided by nothing but n_blocks (profiles/r03_stride_*).
    // Block-major storage has no such distance, and the step's data movement is 5-12 % faster than at the best stride.
    // Translated at the ABI like the block order; only raw pointers see it (ludwig_level_field_layout).
    int64_t sk = 0;        // cells of the level = 512 * n_blocks (the reference's population stride; here only a count)
    bool wide = false;     // 64-bit per-lane addresses: the level's f array is 4 GiB or more (>= 77 672 blocks), or LUDWIG_WIDE_ADDR
    Dev<float> f[2];                       // f, f_temp
    Dev<float> vel[2];                     // vel, vel_temp
    Dev<float> rho, f_post, f_old, rho_old, vel_old;
    Dev<uint8_t> obstacle;
    Dev<float> sponge, wall_dist;
    Dev<int32_t> meta;
    bool has_temporal = false, has_post = false, bouzidi_enabled = false;
    // copy_to_old! without the copies: a pull step never writes its input buffers, so after ludwig_save_old(t_sub) the saved
    // f / vel ARE f[in] / vel[in] until something else writes that buffer. old_alias = that buffer index, or -1 when the
    // saved state lives in f_old / vel_old (materialize_old() copies it there before any such write). rho is copied.
    int old_alias = -1;
    // ludwig_level_field_ptr handed out a WRITABLE device pointer (f, f_temp, vel, vel_temp, rho, ...): from then on the caller
    // may write into the level at any time without the library seeing it, so the three shortcuts that rely on seeing every
    // write are off for this level - saved state is copied (no aliasing), its children's interface values are not computed
    // ahead, rho is stored by every step.
    bool external_writer = false;
    int n_bc = 0;
    Dev<int4> bouzidi_links;            // every listed link with q > 0 (the q map is static): kernels.hpp BouzidiParams::links
    int n_bouzidi_links = 0;
    Dev<uint32_t> post_rows;            // [n_blocks][2] bits: the x-rows f_post_collision is read at by the links with q > 0 (SCParams::post_rows)
    std::vector<uint32_t> h_post_rows;  // host copy (ludwig_level_add_post_collision_readers ORs into it)
    int post_mode = 0;                  // 0: rows / blocks with a reader; 1: every block because asked to (flag, environment);
                                        // 2: every block because no cell list is owned and nobody has named the readers yet
    bool post_rows_used = false;        // the last stream-collide stored f_post_collision by rows (valid for q_min >= 0 only)
    Dev<_Float16> q_map;
    Dev<int32_t> cell_block;
    Dev<int8_t> cell_x, cell_y, cell_z;
    // Block order. The caller's arrays keep the reference's block order (sort of (bx,by,bz) tuples, src/domain.jl:171: bz fastest
    // in memory, x neighbours 2 MB apart at 256^3). The device arrays hold the blocks in the library's own order - owned blocks
    // first, each group sorted with bx FASTEST - so that the four x-consecutive blocks an x-run workgroup steps are consecutive
    // in memory and a sweep "x, then y, then z" reads and writes every population stream sequentially while x / y neighbours stay
    // close in time in one L2 (the block order's DRAM floor AND the x-run order's halo hits). Everything inside the
    // library uses internal ids; the ABI translates: create (tables, geometry, Bouzidi lists), upload / download (a block-permuting
    // copy through `scratch`, one population at a time), halo pack / unpack (offsets translated in the kernel), set_order.
    std::vector<int32_t> ref2int, int2ref;      // empty = the reference order is kept (LUDWIG_REFERENCE_BLOCK_ORDER, or <= 1 block)
    bool x_fastest_memory = false;              // known while the default launch order is built (before ref2int is attached)
    Dev<int32_t> d_ref2int;
    Dev<float> scratch;                         // one population in the reference order (sk floats), allocated on first use
    std::vector<int32_t> h_meta;
    std::vector<uint8_t> h_comm_boundary;
    Dev<int32_t> items[N_PARTS][N_CLASSES];
    int64_t n_items[N_PARTS][N_CLASSES] = {};
    // small levels step both kinds of blocks in ONE launch (merge_classes): the all-neighbour workgroups followed by the general ones,
    // through the GENERAL instantiation. The separate lists stay for the rho replay and for levels that are not merged.
    Dev<int32_t> items_merged[N_PARTS];
    int64_t n_items_merged[N_PARTS] = {};
    int n_fast_blocks = 0;
    bool general_in_runs[N_PARTS] = {};     // class-1 items are in x-run format (link bits, XRUN waves per workgroup)
    int64_t n_linked_items[N_PARTS] = {};   // class-2 waves that exchange a face column with a neighbouring wave
    int64_t device_bytes = 0;
    // coarse -> fine interface pass (levels >= 2): links per part, built lazily for the global box of the first step
    int n_iface_blocks = 0;
    Dev<float> f_iface;
    Dev<int4> links[N_PARTS];            // per link: (block << 9) | cell, (gbi << 5) | k, source index
    Dev<int4> sources[N_PARTS];         // per source cell: 8 parent-cell offsets of its trilinear stencil (-1 = absent), 2 x int4
    Dev<float4> source_w[N_PARTS];      // per source cell: interpolation weights wx, wy, wz
    Dev<float4> source_mac[N_PARTS];    // per source cell, rewritten every pass: interpolated rho, ux, uy, uz
    Dev<float4> source_mac2[N_PARTS];   // the same for the speculated weight of the next sub-step
    Dev<float> f_iface2;
    // What a set of interface values was computed from and for; every placement of the pass keeps its record in this one form, so a
    // key cannot be known to one and forgotten by another. The values hold while the parent was not written (parent_version) and
    // the question is asked for the same sub-step (or pair), weight, parent tau and blending mode.
    struct IfaceKey {
        bool valid = false;
        const LudwigLevel *parent = nullptr;      // borrowed
        uint64_t parent_version = 0;
        int64_t step = 0;             // the sub-step the values are for; pair_ready: the pair, t_sub >> 1
        float tw = 0.0f, tau_parent = 0.0f;
        int use_temporal = 0;
        int set = 0;                  // pair_ready only: which pair of side buffers holds the values
        void fill(const LudwigLevel *parent_, int64_t step_, float tw_, float tau_parent_, int use_temporal_)
        {
            valid = true; parent = parent_; parent_version = parent_->version; step = step_;
            tw = tw_; tau_parent = tau_parent_; use_temporal = use_temporal_;
        }
        bool matches(const LudwigLevel *parent_, int64_t step_, float tw_, float tau_parent_, int use_temporal_) const
        {
            return valid && parent == parent_ && parent_version == parent_->version && step == step_ && tw == tw_ &&
                   tau_parent == tau_parent_ && use_temporal == use_temporal_;
        }
    };
    // Interface values computed ahead for the second sub-step of a pair (reference src/solver_control.jl:63-83: the child
    // steps 2t with weight 0.0 and 2t+1 with 0.5 against the same parent buffers), in f_iface2.
    IfaceKey ahead[N_PARTS];
    // Interface values produced BEFORE the step that uses them (interface_prepass: level streams run a parent level's interface
    // pass ahead of its wait for the children, see recursive_step), in f_iface.
    IfaceKey prepared[N_PARTS];
    // Lazy rho. The step writes `rho` (4 of 244 B per cell update) for readers that mostly are not there: the next step
    // overwrites it unread unless a child level interpolates from it (every step), or a diagnostic / download / save asks
    // for it (now and then). A level nobody has read `rho` of in between therefore skips the store and remembers the
    // launch (rho_replay); ensure_rho() reproduces the array on demand with the RHO_ONLY instantiation, from the same
    // input buffers (a pull step never writes its inputs) - bit for bit what the step would have stored.
    // Only whole-level launches (LUDWIG_PART_ALL) elide the store. Boundary / interior part launches - the multi-GPU schedule, where
    // the next step's interior blocks start before this step's halo has landed - always store: a part's elided rho could no longer
    // be reproduced once another part's launch has reused its input buffer.
    bool rho_eager = false;             // a child reads rho after every step (or LUDWIG_EAGER_RHO): always store
    struct RhoReplay {
        bool stale = false;             // the launch left rho unwritten
        int64_t t_sub = -1;
        SCParams p;
    } rho_replay[N_PARTS];              // only [LUDWIG_PART_ALL] is ever stale
    int64_t step_count = 0, last_step_t = -1, last_replay_step = -10;   // a level asked for rho after two steps in a row turns eager
    // ludwig_execute_timestep_batch runs every level on a stream of its own (level_streams below): events that order them
    HipStream own_stream;
    hipEvent_t parent_wait = nullptr;   // borrowed; set by recursive_step: the parent's step this sub-step's interface pass has to wait for
    // rho_old in the step: copy_to_old!'s copy of rho (the one field a step overwrites in place) costs a launch and two transitions on
    // a parent level's stream per step. The batch driver leaves it to the step that follows: every cell saves its old rho before it
    // stores the new one (kernels.hpp rho_old_save). Only whole-level launches of a level without ghost blocks; anything that
    // would read rho_old or write rho in between performs the copy first (resolve_rho_old).
    bool rho_old_pending = false;
    // Parent-side interface pass (level streams, recursive_step): the PARENT's stream computes this level's interface values for
    // the pair of sub-steps 2t, 2t + 1 right after the parent's step t, into set t & 1 of a second pair of side buffers - while this
    // level is still stepping pair t - 1 out of the other set. This level's own stream then carries no interface kernels at all.
    Dev<float> f_iface_b, f_iface2_b;                              // set 1 (set 0 = f_iface, f_iface2)
    Dev<float4> mac_b, mac2_b;                                     // scratch of set 1's pass (LUDWIG_PART_ALL)
    IfaceKey pair_ready;                                           // step = the pair; tw = the first sub-step's weight, the second's is 0.5
    HipEvent ev_pair_done[2];                                      // recorded on THIS level's stream after the second sub-step of a pair
    bool pair_done_set[2] = {false, false};
    HipEvent ev_stepped;                // recorded on this level's stream after each of its steps (collision + Bouzidi)
    HipEvent ev_consumed;               // recorded on the CHILD's stream once its interface pass has read this level's buffers
    bool ev_consumed_set = false;
    uint64_t stepped_gen = 0;           // how often ev_stepped has been recorded
    const LudwigLevel *waited_parent = nullptr;   // borrowed: the parent step this level's stream has already been made to wait for
    uint64_t waited_gen = 0;
    uint64_t version = 0;               // bumped by everything that writes this level's fields
    const LudwigLevel *iface_parent = nullptr;    // borrowed
    std::vector<int32_t> h_block_pointer;   // [gdx,gdy,gdz] 1-based, 0 = absent (src/blocks.jl:111-114)
    int n_links[N_PARTS] = {};
    int n_sources[N_PARTS] = {};
    int iface_dims[3] = {-1, -1, -1};
    // time-averaged statistics (ludwig_level_stats_*): [n_blocks][STAT_COMPONENTS][512] doubles in the internal block order, allocated
    // by the first reset; only the owned blocks are ever accumulated, the ghost blocks stay zero
    Dev<double> stats;
    bool stats_ready = false;           // reset has been called
    int64_t stats_n = 0;                // samples accumulated since
    // velocity-gradient fields (ludwig_level_gradient_fields_*): [n_blocks][GRAD_COMPONENTS][512] floats in the internal block order,
    // allocated (and zeroed) by the first compute; only the owned blocks are ever written, the ghost blocks stay zero
    Dev<float> grad;
    bool grad_ready = false;            // compute has been called
    // subgrid model (ludwig_level_subgrid_*). The model constants are the step's own: every stream-collide launch of this level records
    // the c_wale and nu_sgs_background it was given, and the observers evaluate with those, so they cannot disagree with the step.
    // fields: [n_blocks][SUBGRID_FIELD_COMPONENTS][512] floats, allocated (and zeroed) by the first compute; sums: [n_blocks]
    // [SUBGRID_SUM_COMPONENTS][512] doubles, allocated by the first reset. Internal block order; the ghost blocks stay zero.
    bool wale_known = false;            // a step has run
    float c_wale = 0.0f, nu_bg = 0.0f;
    Dev<float> subgrid_fields;
    bool subgrid_fields_ready = false;  // compute has been called
    Dev<double> subgrid_sums;
    bool subgrid_stats_ready = false;   // reset has been called
    int64_t subgrid_n = 0;              // samples accumulated since
    // flow monitor (ludwig_level_monitor): one MonitorRecord per owned block in the reference block order, then the records of every
    // combine stage (512 -> 1) behind them; allocated by the first call
    Dev<MonitorRecord> monitor_slab;
    // wall diagnostics (ludwig_level_wall_census): the one device record, allocated by the first call
    Dev<WallCensusRecord> wall_census;
    // iso-surfaces (ludwig_level_isosurface_*): everything is allocated by the first extraction. iso_scalar: [n_blocks][512], the
    // magnitudes that are stored nowhere; counts / offsets / skip: one entry per owned block in the reference block order; the triangle
    // buffers hold iso_capacity triangles and grow when an extraction needs more.
    Dev<float> iso_scalar;
    Dev<int32_t> iso_counts;
    Dev<int64_t> iso_offsets;
    Dev<uint8_t> iso_skip;
    Dev<int32_t> d_int2ref;             // the internal -> reference block order on the device (a vertex key names reference blocks)
    Dev<float> iso_pos, iso_att;
    Dev<int32_t> iso_keys;
    int64_t iso_capacity = 0;
    int64_t iso_n = -1;                 // triangles of the last extraction (0 after a refusal); -1: none yet
    // Record step (kernels.hpp "Record step"). A plain level - record_eligible() - steps from 11-float collision records instead of
    // f / vel / rho: rec[q] plays the role of f[q] and vel[q]. Per parity q, f_valid[q] says f[q] / vel[q] hold what the f path would
    // hold there and rec_valid[q] the same for rec[q]; a record step into parity q makes rec[q] valid and f[q] / vel[q] stale, and
    // ensure_populations() brings them back with k_materialise before anything reads or hands them out. rho_in_rec = the parity
    // whose record holds the density `rho` should hold (the last record step's output), or -1 when `rho` itself is in charge.
    Dev<float> rec[2];                      // allocated by the first record step
    bool f_valid[2] = {true, true}, rec_valid[2] = {false, false};
    int rho_in_rec = -1;
    int rec_eligible = -1;                  // the level's part of the rule: -1 unknown (recomputed after set_items / upload_meta)
    bool rec_banned = false;                // another level reads this one, or the record buffers could not be allocated: f path for good
    bool rec_hold = false;                  // a batch with in-batch observers or several levels is running: f path meanwhile
    Dev<int32_t> rec_items;                 // the class-2 work list in the record path's order, see record_items()
    int64_t n_record_steps = 0;
};

namespace {

template <class T>
int dev_alloc(LudwigLevel *L, Dev<T> &p, size_t count)
{
    const int e = p.alloc(count);
    if (e) return fail(LUDWIG_ERR_ALLOC, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString((hipError_t)e));
    L->device_bytes += (int64_t)(count * sizeof(T));
    return LUDWIG_OK;
}

// A host table onto the device, unless an earlier table of the chain has failed already (e says so).
template <class T>
void upload_table(hipError_t &e, const std::vector<T> &h, Dev<T> &dev)
{
    if (e == hipSuccess) e = (hipError_t)dev.alloc(h.size());
    if (e == hipSuccess && !h.empty()) e = hipMemcpy(dev, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

// what ludwig_level_destroy and every ludwig_*_destroy of a set do: the object's device is current while its members release
template <class S>
void destroy_set(S *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

int fill(LudwigLevel *L, float *a, int64_t n, float v)
{
    if (n == 0) return LUDWIG_OK;
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, L->stream, a, n, v);
    LW_HIP(hipGetLastError());
    return LUDWIG_OK;
}

struct FieldDesc {
    void *ptr;
    size_t bytes;
    int comps = 1;     // K: components per cell
    int es = 4;        // element size in bytes
};

int ensure_rho(LudwigLevel *L);

// ---- record step: validity (LudwigLevel::rec) ----
// The ONE way back from records to populations: f[parity] / vel[parity] (and rho, where that parity's record holds it) are made what
// the f path would hold there. parity -1 = both. Called by whatever reads them, hands them out or writes into them; a no-op on a
// level that has taken no record step since.
int ensure_populations(LudwigLevel *L, int parity)
{
    for (int q = 0; q < 2; ++q) {
        if ((parity >= 0 && parity != q) || L->f_valid[q]) continue;
        LW_HIP(hipSetDevice(L->device));
        SCParams p{};
        p.rec_in = L->rec[q];
        p.f_out = L->f[q];
        p.vel_out = L->vel[q];
        p.rho = L->rho_in_rec == q ? L->rho : nullptr;      // only the last record step's density is the level's rho
        hipLaunchKernelGGL(k_materialise, dim3((unsigned)((L->sk + 255) / 256)), dim3(256), 0, L->stream, p, L->sk);
        LW_HIP(hipGetLastError());
        L->f_valid[q] = true;
        if (L->rho_in_rec == q) L->rho_in_rec = -1;
    }
    return LUDWIG_OK;
}

// f, vel and rho of both parities as the f path would hold them now (observers and diagnostics read them through raw pointers)
#define LW_ENSURE_POPULATIONS(L)                                                                          \
    do {                                                                                                  \
        const int rp_ = ensure_populations(const_cast<LudwigLevel *>(L), -1);                             \
        if (rp_) return rp_;                                                                              \
    } while (0)

int materialize_old(LudwigLevel *L)
{
    if (L->old_alias < 0) return LUDWIG_OK;
    ++L->version;
    const size_t c = (size_t)L->sk;
    const int a = L->old_alias;
    L->old_alias = -1;
    LW_HIP(hipSetDevice(L->device));
    LW_HIP(hipMemcpyAsync(L->f_old, L->f[a], c * Q * 4, hipMemcpyDeviceToDevice, L->stream));
    LW_HIP(hipMemcpyAsync(L->vel_old, L->vel[a], c * 3 * 4, hipMemcpyDeviceToDevice, L->stream));
    return LUDWIG_OK;
}

// call before anything but a stream-collide step writes `field` (upload, halo unpack, a raw pointer handed out)
int before_external_write(LudwigLevel *L, int field)
{
    {   // the write lands in populations: they are brought up to date first, and no record stands for them afterwards
        const int r = ensure_populations(L, -1);
        if (r) return r;
        L->rec_valid[0] = L->rec_valid[1] = false;
    }
    // an elided rho is recomputed from the input populations / sponge / obstacle of the last step: produce it before any
    // of them changes (a halo unpack into the OUTPUT buffer of that step, the usual case, does not touch them)
    bool feeds_rho = field == LUDWIG_SPONGE || field == LUDWIG_OBSTACLE || field == LUDWIG_RHO;
    for (int a = 0; a < N_PARTS; ++a)
        if (L->rho_replay[a].stale && (field == LUDWIG_F || field == LUDWIG_F_TEMP) && L->f[field == LUDWIG_F ? 0 : 1] == L->rho_replay[a].p.f_in) feeds_rho = true;
    if (feeds_rho) {
        const int r = ensure_rho(L);
        if (r) return r;
    }
    if (L->old_alias < 0) return LUDWIG_OK;
    const int a = L->old_alias;
    const bool hits = field == LUDWIG_F_OLD || field == LUDWIG_VEL_OLD || (field == LUDWIG_F && a == 0) || (field == LUDWIG_F_TEMP && a == 1) ||
                      (field == LUDWIG_VEL && a == 0) || (field == LUDWIG_VEL_TEMP && a == 1);
    return hits ? materialize_old(L) : LUDWIG_OK;
}

FieldDesc field_desc(const LudwigLevel *L, int field)
{
    const size_t c = (size_t)L->sk;
    if (L->old_alias >= 0) {          // readers of the saved state follow the alias
        if (field == LUDWIG_F_OLD) return {L->f[L->old_alias], L->has_temporal ? c * Q * 4 : 0, Q, 4};
        if (field == LUDWIG_VEL_OLD) return {L->vel[L->old_alias], L->has_temporal ? c * 3 * 4 : 0, 3, 4};
    }
    switch (field) {
    case LUDWIG_F: return {L->f[0], c * Q * 4, Q, 4};
    case LUDWIG_F_TEMP: return {L->f[1], c * Q * 4, Q, 4};
    case LUDWIG_F_POST: return {L->f_post, L->has_post ? c * Q * 4 : 0, Q, 4};
    case LUDWIG_F_OLD: return {L->f_old, L->has_temporal ? c * Q * 4 : 0, Q, 4};
    case LUDWIG_RHO: return {L->rho, c * 4, 1, 4};
    case LUDWIG_RHO_OLD: return {L->rho_old, L->has_temporal ? c * 4 : 0, 1, 4};
    case LUDWIG_VEL: return {L->vel[0], c * 3 * 4, 3, 4};
    case LUDWIG_VEL_TEMP: return {L->vel[1], c * 3 * 4, 3, 4};
    case LUDWIG_VEL_OLD: return {L->vel_old, L->has_temporal ? c * 3 * 4 : 0, 3, 4};
    case LUDWIG_OBSTACLE: return {L->obstacle, c, 1, 1};
    case LUDWIG_SPONGE: return {L->sponge, c * 4, 1, 4};
    case LUDWIG_WALL_DIST: return {L->wall_dist, c * 4, 1, 4};
    default: return {nullptr, 0, 1, 4};
    }
}

// per-block flags that let the kernel skip loads: recomputed whenever the host hands us the field
void scan_flags(LudwigLevel *L, int field, const void *host)
{
    const int flag = field == LUDWIG_OBSTACLE ? FLAG_HAS_OBSTACLE : field == LUDWIG_SPONGE ? FLAG_HAS_SPONGE : FLAG_HAS_NEAR_WALL;
    for (int b = 0; b < L->n_blocks; ++b) {
        bool any = false;
        if (host) {
            if (field == LUDWIG_OBSTACLE) {
                const uint8_t *o = (const uint8_t *)host + (size_t)b * CELLS;
                for (int i = 0; i < CELLS && !any; ++i) any = o[i] != 0;
            } else if (field == LUDWIG_SPONGE) {
                const float *s = (const float *)host + (size_t)b * CELLS;
                for (int i = 0; i < CELLS && !any; ++i) any = s[i] > 0.0f;
            } else {
                const float *d = (const float *)host + (size_t)b * CELLS;
                for (int i = 0; i < CELLS && !any; ++i) any = d[i] > 0.0f && d[i] < 10.0f;
            }
        }
        int32_t &fl = L->h_meta[(size_t)b * NBR_STRIDE + NBR_FLAGS];
        fl = any ? (fl | flag) : (fl & ~flag);
    }
}

int upload_meta(LudwigLevel *L)
{
    L->rec_eligible = -1;                     // the per-block flags are part of the record step's rule
    if (L->n_blocks == 0) return LUDWIG_OK;
    LW_HIP(hipMemcpyAsync(L->meta, L->h_meta.data(), L->h_meta.size() * 4, hipMemcpyHostToDevice, L->stream));
    LW_HIP(hipStreamSynchronize(L->stream));
    return LUDWIG_OK;
}

// h_post_rows onto the device: into the table the level has, or into a new one that becomes the level's once it is filled
int upload_post_rows(LudwigLevel *L)
{
    if (L->post_rows) {
        LW_HIP(hipMemcpy(L->post_rows, L->h_post_rows.data(), L->h_post_rows.size() * 4, hipMemcpyHostToDevice));
        return LUDWIG_OK;
    }
    hipError_t e = hipSuccess;
    Dev<uint32_t> rows;
    upload_table(e, L->h_post_rows, rows);
    if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "post-collision rows: %s", hipGetErrorString(e));
    L->post_rows = std::move(rows);
    return LUDWIG_OK;
}

bool block_in_part(const LudwigLevel *L, int b, int part)
{
    if (b >= L->n_owned) return false;
    if (part == LUDWIG_PART_ALL) return true;
    const bool bnd = !L->h_comm_boundary.empty() && L->h_comm_boundary[b] != 0;
    return part == LUDWIG_PART_BOUNDARY ? bnd : !bnd;
}

// LUDWIG_MERGE_CLASSES: 1 = always one launch per pass, 0 = never, unset = levels below MERGE_BELOW_BLOCKS owned blocks
constexpr int MERGE_BELOW_BLOCKS = 8192;      // 4.2 M cells: above that a pass is > 0.2 ms and the extra launch is noise
bool merge_classes(const LudwigLevel *L, const std::vector<int32_t> &general, const std::vector<int32_t> &fast)
{
    if (general.empty() || fast.empty()) return false;
    const int e = env::merge_classes();
    return e >= 0 ? e != 0 : L->n_owned < MERGE_BELOW_BLOCKS;
}

int set_items(LudwigLevel *L, int part, const int32_t *items, int64_t n)
{
    // one item per wave: (block << 3) | z, or -1 = idle wave. XRUN consecutive items form one workgroup.
    // class 2: all-neighbour blocks, class 1: blocks with a missing neighbour - both through the x-run kernel;
    // class 0 (wave-by-wave kernel) only with LUDWIG_NO_XRUN (diagnostics).
    std::vector<int32_t> cls[N_CLASSES];
    auto is_fast = [&](int b) { return (L->h_meta[(size_t)b * NBR_STRIDE + NBR_FLAGS] & FLAG_ALL_NEIGHBOURS) != 0; };
    for (int64_t i = 0; i < n; ++i) {
        if (items[i] >= 0) {
            const int b = items[i] >> 3;
            if (b < 0 || b >= L->n_owned) return fail(LUDWIG_ERR_INVALID, "work item %lld: block %d is not an owned block", (long long)i, b);
            if (!block_in_part(L, b, part)) return fail(LUDWIG_ERR_INVALID, "work item %lld: block %d is not in part %d", (long long)i, b, part);
        }
    }
    const bool use_xrun = true;
    int64_t n_linked = 0;
    {
        // All-neighbour blocks -> x-run kernel (class 2), XRUN waves per workgroup; a wave is LINKED to the next one when
        // that one holds its +x neighbour block at the same plane (then the face column travels through LDS). Workgroups
        // of the caller's order that hold only such blocks keep their composition (and with it their XCD slot); loose
        // all-neighbour items of mixed workgroups are re-packed at the end. Blocks with a missing neighbour -> class 1.
        std::vector<int32_t> loose[2];                     // [0] all-neighbour, [1] general items of mixed workgroups
        for (int64_t g = 0; g < n; g += XRUN) {
            const int64_t m = std::min<int64_t>(XRUN, n - g);
            int n_fast = 0, n_gen = 0;
            for (int64_t w = 0; w < m; ++w)
                if (items[g + w] >= 0) (is_fast(items[g + w] >> 3) ? n_fast : n_gen)++;
            const bool pure = m == XRUN && (n_fast == 0 || n_gen == 0);
            for (int64_t w = 0; w < m; ++w) {
                const int32_t it = items[g + w];
                if (pure) { if (n_fast + n_gen > 0) cls[n_gen > 0 ? 1 : 2].push_back(it); }
                else if (it >= 0) loose[is_fast(it >> 3) ? 0 : 1].push_back(it);
            }
        }
        for (int c = 1; c <= 2; ++c) {
            const std::vector<int32_t> &lo = loose[c == 2 ? 0 : 1];
            cls[c].insert(cls[c].end(), lo.begin(), lo.end());
            while (cls[c].size() % XRUN) cls[c].push_back(-1);
            for (size_t g = 0; g < cls[c].size(); g += XRUN)
                for (int w = 0; w + 1 < XRUN; ++w) {
                    const int32_t a = cls[c][g + w], d = cls[c][g + w + 1];
                    if (a < 0 || d < 0 || (a & 7) != (d & 7)) continue;
                    const int ba = (a & ITEM_ID_MASK) >> 3, bd = d >> 3;     // `a` may already carry its west link
                    if (ba == bd || L->h_meta[(size_t)ba * NBR_STRIDE + DIR(1, 0, 0)] != bd) continue;
                    cls[c][g + w] |= ITEM_LINK_E;
                    cls[c][g + w + 1] |= ITEM_LINK_W;
                }
        }
        for (int32_t it : cls[2])
            if (it >= 0 && (it & (ITEM_LINK_E | ITEM_LINK_W))) ++n_linked;
    }
    std::vector<int32_t> merged;
    if (use_xrun && merge_classes(L, cls[1], cls[2])) {
        // one launch for the whole pass: the all-neighbour workgroups ride along in the GENERAL instantiation (its patch
        // phase finds nothing to do for them) - on small levels a launch boundary costs more than that
        merged = cls[2];
        merged.insert(merged.end(), cls[1].begin(), cls[1].end());
    }
    // the new lists are made beside the level's; a failure leaves the level stepping on the lists it had
    hipError_t e = hipSuccess;
    Dev<int32_t> d_merged, d_cls[N_CLASSES];
    upload_table(e, merged, d_merged);
    for (int c = 0; c < N_CLASSES; ++c) {
        bool any = false;
        for (int32_t it : cls[c]) any = any || it >= 0;
        if (!any) cls[c].clear();
        while (cls[c].size() % XRUN) cls[c].push_back(-1);
        upload_table(e, cls[c], d_cls[c]);
    }
    if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "work lists of part %d: %s", part, hipGetErrorString(e));
    L->general_in_runs[part] = true;
    L->n_linked_items[part] = n_linked;
    L->items_merged[part] = std::move(d_merged);
    L->n_items_merged[part] = (int64_t)merged.size();
    for (int c = 0; c < N_CLASSES; ++c) {
        L->items[part][c] = std::move(d_cls[c]);
        L->n_items[part][c] = (int64_t)cls[c].size();
    }
    if (part == LUDWIG_PART_ALL) {            // the record step's work list is made from this part's: rebuilt on its next step
        L->rec_eligible = -1;
        L->rec_items.reset();
    }
    return LUDWIG_OK;
}

// Default launch order: x-runs, plane-per-XCD.
// A cache line of population k, z-plane p of a block is read only by waves working on plane p + cz(k): in the
// owning block and in its x/y neighbours (faces, edges); nothing is shared across different plane indices.
//  * workgroup = the same plane of 4 x-consecutive all-neighbour blocks -> the x-run kernel: aligned loads only,
//    x-face columns handed over in LDS (kernels.hpp). Runs are cut greedily along every (by,bz) row of blocks.
//  * MI355X deals workgroup g to XCD g % 8 (private L2 each): the 8 planes of a group occupy 8 consecutive slots,
//    plane z on XCD (z + bz) % 8, so a line is fetched by one XCD only; groups are swept y-fastest, then x, then z.
//  * chains shorter than a workgroup (leftovers, lone blocks) are packed several to a workgroup, same slot rule; a work
//    item's link bits say which lateral faces arrive through LDS. Blocks with a missing neighbour (domain edges,
//    refinement interfaces) are chained the same way among themselves and take the GENERAL instantiation.
// Measured at 256^3 against the alternatives with tools/order_sweep.py (DESIGN.md "Launch order").
int default_items(LudwigLevel *L, int part)
{
    struct Blk { int32_t bx, by, bz, b; };
    std::vector<Blk> blks;
    for (int b = 0; b < L->n_owned; ++b) {
        if (!block_in_part(L, b, part)) continue;
        const int32_t *row = &L->h_meta[(size_t)b * NBR_STRIDE];
        blks.push_back({row[NBR_BX], row[NBR_BY], row[NBR_BZ], b});
    }
    std::sort(blks.begin(), blks.end(), [](const Blk &a, const Blk &c) {
        if (a.by != c.by) return a.by < c.by;
        if (a.bz != c.bz) return a.bz < c.bz;
        return a.bx < c.bx;
    });
    auto fast = [&](int b) { return (L->h_meta[(size_t)b * NBR_STRIDE + NBR_FLAGS] & FLAG_ALL_NEIGHBOURS) != 0; };
    struct Group { int32_t by, bx0, bz; int32_t n; int32_t b[XRUN_MAX]; };
    // kind 0: all-neighbour blocks, kind 1: blocks with a missing neighbour. Chains never mix kinds (different kernels).
    std::vector<Group> runs[2], shorts[2];      // full runs of XRUN; leftover chains of 1 .. XRUN-1 blocks
    size_t i = 0;
    while (i < blks.size()) {
        // maximal chain of x-consecutive blocks of one kind starting at i (same by,bz row)
        size_t j = i;
        const int kind = fast(blks[i].b) ? 0 : 1;
        while (j + 1 < blks.size() && blks[j + 1].by == blks[i].by && blks[j + 1].bz == blks[i].bz && (fast(blks[j + 1].b) ? 0 : 1) == kind &&
               L->h_meta[(size_t)blks[j].b * NBR_STRIDE + DIR(1, 0, 0)] == blks[j + 1].b && blks[j + 1].b != blks[i].b)
            ++j;
        size_t k = i;
        for (; k + XRUN <= j + 1; k += XRUN) {
            Group g{blks[k].by, blks[k].bx, blks[k].bz, XRUN, {}};
            for (int w = 0; w < XRUN; ++w) g.b[w] = blks[k + w].b;
            runs[kind].push_back(g);
        }
        if (k <= j) {
            Group g{blks[k].by, blks[k].bx, blks[k].bz, (int32_t)(j + 1 - k), {}};
            for (size_t w = k; w <= j; ++w) g.b[w - k] = blks[w].b;
            shorts[kind].push_back(g);
        }
        i = j + 1;
    }
    // sweep. Internal block order (x fastest in memory): x fastest, then y, then z = memory order, every population stream is
    // read and written sequentially, and the x / y neighbour groups follow within a few workgroups on the same XCD.
    // Reference block order kept (LUDWIG_REFERENCE_BLOCK_ORDER): y fastest, then x, then z (round 1's choice for that layout).
    const bool x_fastest = L->x_fastest_memory;
    auto by_zxy = [x_fastest](const Group &a, const Group &c) {
        if (a.bz != c.bz) return a.bz < c.bz;
        if (x_fastest) {
            if (a.by != c.by) return a.by < c.by;
            return a.bx0 < c.bx0;
        }
        if (a.bx0 != c.bx0) return a.bx0 < c.bx0;
        return a.by < c.by;
    };
    // slot 8 * group + x runs on XCD x and steps plane z = (x - bz) mod 8: x/y neighbours (same bz, same plane) share an
    // XCD, and over bz every XCD sees every plane index, i.e. every value of address bits 8..10 (no L2-channel aliasing)
    std::vector<int32_t> seq;
    for (int kind = 0; kind < 2; ++kind) {
        std::sort(runs[kind].begin(), runs[kind].end(), by_zxy);
        std::sort(shorts[kind].begin(), shorts[kind].end(), by_zxy);
        for (const Group &g : runs[kind])
            for (int x = 0; x < 8; ++x) {
                const int z = ((x - g.bz) % 8 + 8) % 8;
                for (int w = 0; w < XRUN; ++w) seq.push_back((g.b[w] << 3) | z);
            }
        // leftover chains: whole chains packed into workgroups of XRUN waves (never split), same slot rule
        for (size_t s0 = 0; s0 < shorts[kind].size();) {
            int32_t wg[XRUN_MAX];
            int used = 0;
            const int bz0 = shorts[kind][s0].bz;
            while (s0 < shorts[kind].size() && used + shorts[kind][s0].n <= XRUN) {
                for (int w = 0; w < shorts[kind][s0].n; ++w) wg[used++] = shorts[kind][s0].b[w];
                ++s0;
            }
            for (int x = 0; x < 8; ++x) {
                const int z = ((x - bz0) % 8 + 8) % 8;
                for (int w = 0; w < XRUN; ++w) seq.push_back(w < used ? (wg[w] << 3) | z : -1);
            }
        }
    }
    return set_items(L, part, seq.data(), (int64_t)seq.size());
}

// Links (cell, population) of the interface blocks whose source block is missing and for which the reference's
// domain-edge chain (src/physics_kernels.jl:88-140) selects the parent interpolation: source inside the global box.
int build_interface_links(LudwigLevel *L, const LudwigLevel *parent, int nx_g, int ny_g, int nz_g)
{
    // Everything about a link that does not depend on the flow is fixed here, once: which (cell, population) pairs pull
    // from outside the level (reference src/physics_kernels.jl:122-137), and for each such source cell the 8 parent cells
    // of its trilinear stencil and the weights (reference src/physics_interpolation.jl:29-62: px_cont, floor, +1 before
    // the clamp to 1, block lookup through the parent's block_pointer).
    if (L->iface_parent == parent && L->iface_dims[0] == nx_g && L->iface_dims[1] == ny_g && L->iface_dims[2] == nz_g) return LUDWIG_OK;
    if (parent->h_block_pointer.size() != (size_t)parent->gdx * parent->gdy * parent->gdz)
        return fail(LUDWIG_ERR_STATE, "parent level %d was created without block_pointer: its children cannot interpolate", parent->level_id);
    LW_HIP(hipStreamSynchronize(L->stream));
    struct Link { int64_t key; int sx, sy, sz; int2 e; };
    std::vector<Link> raw[N_PARTS];
    // every table is made beside the level's and moved in at the end: a failure leaves the level with the tables it had
    struct Tables { Dev<int4> links, sources; Dev<float4> w, mac, mac2; int n_links = 0, n_sources = 0; } made[N_PARTS];
    hipError_t e = hipSuccess;
    for (int b = 0; b < L->n_owned; ++b) {
        const int32_t *row = &L->h_meta[(size_t)b * NBR_STRIDE];
        const int gbi = row[NBR_GBI];
        if (gbi < 0) continue;
        const bool bnd = !L->h_comm_boundary.empty() && L->h_comm_boundary[b] != 0;
        for (int cell = 0; cell < CELLS; ++cell) {
            const int x = cell & 7, y = (cell >> 3) & 7, z = cell >> 6;
            if (x > 0 && x < 7 && y > 0 && y < 7 && z > 0 && z < 7) continue;
            const int gx = (row[NBR_BX] - 1) * BS + x + 1, gy = (row[NBR_BY] - 1) * BS + y + 1, gz = (row[NBR_BZ] - 1) * BS + z + 1;
            for (int k = 0; k < Q; ++k) {
                const int sx = x - CX(k), sy = y - CY(k), sz = z - CZ(k);
                const int ox = sx < 0 ? -1 : (sx > 7 ? 1 : 0), oy = sy < 0 ? -1 : (sy > 7 ? 1 : 0), oz = sz < 0 ? -1 : (sz > 7 ? 1 : 0);
                if ((ox | oy | oz) == 0 || row[DIR(ox, oy, oz)] >= 0) continue;
                const int src_gx = gx - CX(k), src_gy = gy - CY(k), src_gz = gz - CZ(k);
                if (src_gx < 1 || src_gx > nx_g || src_gy < 1 || src_gy > ny_g || src_gz < 1 || src_gz > nz_g) continue;   // inlet / outlet / mirror win
                const Link l{((int64_t)src_gz * (ny_g + 2) + src_gy) * (nx_g + 2) + src_gx, src_gx, src_gy, src_gz, make_int2((b << 9) | cell, (gbi << 5) | k)};
                raw[LUDWIG_PART_ALL].push_back(l);
                raw[bnd ? LUDWIG_PART_BOUNDARY : LUDWIG_PART_INTERIOR].push_back(l);
            }
        }
    }
    for (int a2 = 0; a2 < N_PARTS; ++a2) {
        std::stable_sort(raw[a2].begin(), raw[a2].end(), [](const Link &u, const Link &v) { return u.key < v.key; });
        std::vector<int4> links;       // (block << 9) | cell, (gbi << 5) | k, source index, unused
        std::vector<int4> corners;     // 2 per source
        std::vector<float4> weights;
        for (size_t i = 0; i < raw[a2].size(); ++i) {
            const Link &l = raw[a2][i];
            if (i == 0 || l.key != raw[a2][i - 1].key) {
                const float pc[3] = {((float)l.sx - 0.5f) * 0.5f, ((float)l.sy - 0.5f) * 0.5f, ((float)l.sz - 0.5f) * 0.5f};
                int p0[3], p1[3];
                float w[3];
                for (int d = 0; d < 3; ++d) {
                    p0[d] = (int)floorf(pc[d]);
                    p1[d] = p0[d] + 1;
                    w[d] = pc[d] - (float)p0[d];
                    p0[d] = std::max(1, p0[d]);
                }
                int cc[8];
                for (int n = 0; n < 8; ++n) {        // corner order 000,100,010,110,001,101,011,111
                    const int pgx = (n & 1) ? p1[0] : p0[0], pgy = (n & 2) ? p1[1] : p0[1], pgz = (n & 4) ? p1[2] : p0[2];
                    const int pbx = (pgx - 1) / BS + 1, pby = (pgy - 1) / BS + 1, pbz = (pgz - 1) / BS + 1;
                    cc[n] = -1;
                    if (pbx >= 1 && pbx <= parent->gdx && pby >= 1 && pby <= parent->gdy && pbz >= 1 && pbz <= parent->gdz) {
                        const int32_t pb = parent->h_block_pointer[(size_t)(pbx - 1) + (size_t)parent->gdx * ((size_t)(pby - 1) + (size_t)parent->gdy * (pbz - 1))];
                        if (pb > 0) cc[n] = ((pgx - 1) % BS) + 8 * ((pgy - 1) % BS) + 64 * ((pgz - 1) % BS) + 512 * (pb - 1);
                    }
                }
                corners.push_back(make_int4(cc[0], cc[1], cc[2], cc[3]));
                corners.push_back(make_int4(cc[4], cc[5], cc[6], cc[7]));
                weights.push_back(make_float4(w[0], w[1], w[2], 0.0f));
            }
            links.push_back(make_int4(l.e.x, l.e.y, (int)weights.size() - 1, 0));
        }
        // launch order of the links: population by population, sources in (z, y, x) order inside. Neighbouring lanes then
        // read neighbouring parent cells of ONE population array (a few 128-B lines per wave-load instead of ~30) and
        // write neighbouring cells of f_iface.
        std::stable_sort(links.begin(), links.end(), [](const int4 &u, const int4 &v) { return (u.y & 31) < (v.y & 31); });
        Tables &t = made[a2];
        t.n_links = (int)links.size();
        t.n_sources = (int)weights.size();
        upload_table(e, links, t.links);
        upload_table(e, corners, t.sources);
        upload_table(e, weights, t.w);
        if (e == hipSuccess) e = (hipError_t)t.mac.alloc(weights.size());
        if (e == hipSuccess) e = (hipError_t)t.mac2.alloc(weights.size());
    }
    const bool first = !L->f_iface && L->n_iface_blocks > 0;      // the pair of side buffers is sized with the level: made once
    const size_t n_side = (size_t)L->n_iface_blocks * CELLS * Q;
    Dev<float> side, side2;
    if (first && e == hipSuccess) e = (hipError_t)side.alloc(n_side);
    if (first && e == hipSuccess) e = (hipError_t)side2.alloc(n_side);
    if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "interface links of level %d: %s", L->level_id, hipGetErrorString(e));
    for (int a2 = 0; a2 < N_PARTS; ++a2) {
        Tables &t = made[a2];
        L->ahead[a2].valid = false;
        L->links[a2] = std::move(t.links); L->sources[a2] = std::move(t.sources); L->source_w[a2] = std::move(t.w);
        L->source_mac[a2] = std::move(t.mac); L->source_mac2[a2] = std::move(t.mac2);
        L->n_links[a2] = t.n_links;
        L->n_sources[a2] = t.n_sources;
    }
    if (first) {
        L->f_iface = std::move(side);
        L->f_iface2 = std::move(side2);
        L->device_bytes += 2 * (int64_t)n_side * 4;
    }
    L->iface_parent = parent;
    L->iface_dims[0] = nx_g; L->iface_dims[1] = ny_g; L->iface_dims[2] = nz_g;
    return LUDWIG_OK;
}

// Everything of SCParams an interface pass reads, for the pass or the step of `L` at sub-step t_sub: the parent-side pointers, the
// two relaxation times, the temporal weight and blending mode, the global box. A step adds its own fields (launch_stream_collide).
static void fill_pass_params(SCParams &p, const LudwigLevel *L, const LudwigLevel *parent, int64_t t_sub, float parent_tau,
                             float temporal_weight, const LudwigStepFlags *fl)
{
    if (parent) {
        const int pout = ((t_sub >> 1) % 2 == 0) ? 1 : 0;   // output buffer of the parent's step t_sub >> 1
        p.pf_new = parent->f[pout];
        p.pvel_new = parent->vel[pout];
        p.prho_new = parent->rho;
        // without temporal storage the reference passes 1-element dummies that are never read
        // (use_temporal_interp is then false at every call site that matters); alias "new" to stay in bounds
        p.pf_old = parent->has_temporal ? (parent->old_alias >= 0 ? parent->f[parent->old_alias] : parent->f_old) : parent->f[pout];
        p.prho_old = parent->has_temporal ? parent->rho_old : parent->rho;
        p.pvel_old = parent->has_temporal ? (parent->old_alias >= 0 ? parent->vel[parent->old_alias] : parent->vel_old) : parent->vel[pout];
    }
    p.is_level_1 = parent ? 0 : 1;
    p.tau = L->tau;
    p.tau_parent = parent_tau;
    p.temporal_weight = temporal_weight;
    const int scale = 1 << (L->level_id - 1);   // reference src/physics_v2.jl:55-56
    p.nx_g = fl->domain_nx * scale; p.ny_g = fl->domain_ny * scale; p.nz_g = fl->domain_nz * scale;
    // a parent without temporal storage cannot be blended with (reference would index a dummy array)
    p.use_temporal = (fl->use_temporal_interp && (!parent || parent->has_temporal)) ? 1 : 0;
}

// One pair of side buffers of a level's interface pass: the values for the pass's own weight, those for the second sub-step of the
// pair (TWO), and the per-source scratch of each. Set 0 is the level's own; set 1 exists on levels whose parent runs the pass.
struct IfaceBuffers {
    float *f_iface, *f_iface2;
    float4 *mac, *mac2;
};

static IfaceBuffers iface_buffers(const LudwigLevel *L, int part, int set)
{
    if (set) return {L->f_iface_b, L->f_iface2_b, L->mac_b, L->mac2_b};
    return {L->f_iface, L->f_iface2, L->source_mac[part], L->source_mac2[part]};
}

// The two kernels of an interface pass of L's `part` on `st`: into b.f_iface for p's weight and, with `two`, into b.f_iface2 for 0.5.
static int launch_interface_kernels(const LudwigLevel *L, int part, SCParams p, const IfaceBuffers &b, bool two, hipStream_t st)
{
    p.f_iface = b.f_iface;
    p.n_iface_blocks = L->n_iface_blocks;
    InterfaceArgs a{};
    a.corners = L->sources[part]; a.weights = L->source_w[part];
    a.mac = b.mac; a.mac2 = b.mac2;
    a.links = L->links[part];
    a.f_iface2 = b.f_iface2;
    a.tw2 = 0.5f;
    a.n_sources = L->n_sources[part]; a.n_links = L->n_links[part];
    const dim3 gs((unsigned)((a.n_sources + 255) / 256)), gl((unsigned)((a.n_links + 255) / 256));
    if (two) {
        hipLaunchKernelGGL(k_interface_sources<true>, gs, dim3(256), 0, st, p, a);
        hipLaunchKernelGGL(k_interface_links<true>, gl, dim3(256), 0, st, p, a);
    } else {
        hipLaunchKernelGGL(k_interface_sources<false>, gs, dim3(256), 0, st, p, a);
        hipLaunchKernelGGL(k_interface_links<false>, gl, dim3(256), 0, st, p, a);
    }
    LW_HIP(hipGetLastError());
    return LUDWIG_OK;
}

// Coarse -> fine interface pass for the general blocks of `part` (reference src/physics_kernels.jl:122-137), in two halves.
// interface_decide: leaves p.f_iface pointing at the values sub-step t_sub loads and says whether kernels have to run for them
// (IFACE_LAUNCH) or they exist already - produced ahead by the parent's stream or by interface_prepass (READY), or together with the
// previous sub-step's (HIT). interface_launch: the two kernels on `st`. ahead_of_step: called by interface_prepass, before the step's
// own launch.
enum IfaceState { IFACE_NONE, IFACE_READY, IFACE_HIT, IFACE_LAUNCH };

static int interface_decide(LudwigLevel *L, const LudwigLevel *parent, int part, SCParams &p, int64_t t_sub, float parent_tau,
                            float temporal_weight, bool ahead_of_step, IfaceState *state)
{
    *state = IFACE_NONE;
    if (!parent || L->n_items[part][1] == 0) return LUDWIG_OK;
    const int r = build_interface_links(L, parent, p.nx_g, p.ny_g, p.nz_g);
    if (r) return r;
    p.f_iface = L->f_iface;
    p.n_iface_blocks = L->n_iface_blocks;
    if (L->n_links[part] == 0) return LUDWIG_OK;
    // 1. produced by the parent's stream for this pair of sub-steps (interface_pass_for_child)? One record serves both sub-steps:
    //    the first half of its set was made with weight 0.0, the second with 0.5
    const LudwigLevel::IfaceKey &pr = L->pair_ready;
    if (!ahead_of_step && part == LUDWIG_PART_ALL && temporal_weight == ((t_sub & 1) ? 0.5f : 0.0f) &&
        pr.matches(parent, t_sub >> 1, 0.0f, parent_tau, p.use_temporal)) {
        const IfaceBuffers b = iface_buffers(L, part, pr.set);
        p.f_iface = (t_sub & 1) ? b.f_iface2 : b.f_iface;
        *state = IFACE_READY;
        return LUDWIG_OK;
    }
    // 2. prepared ahead of this step (interface_prepass)? The look-ahead record for t_sub + 1 stays as it is
    LudwigLevel::IfaceKey &pre = L->prepared[part];
    const bool ready = pre.matches(parent, t_sub, temporal_weight, parent_tau, p.use_temporal);
    pre.valid = ready && ahead_of_step;
    *state = IFACE_READY;
    if (ready) return LUDWIG_OK;
    // 3. speculated together with the previous sub-step's values?
    LudwigLevel::IfaceKey &ah = L->ahead[part];
    const bool hit = ah.matches(parent, t_sub, temporal_weight, parent_tau, p.use_temporal);
    if (hit && ahead_of_step) return LUDWIG_OK;  // nothing to do ahead: the step will find the values in f_iface2
    ah.valid = false;
    *state = IFACE_HIT;
    if (hit) {
        p.f_iface = L->f_iface2;
        return LUDWIG_OK;
    }
    *state = IFACE_LAUNCH;
    return LUDWIG_OK;
}

static int interface_launch(LudwigLevel *L, const LudwigLevel *parent, int part, const SCParams &p, int64_t t_sub, float parent_tau,
                            float temporal_weight, bool ahead_of_step, hipStream_t st)
{
    // first sub-step of a pair (even t_sub): also produce the values for t_sub + 1 at weight 0.5
    const bool two = (t_sub % 2 == 0) && !parent->external_writer && !env::no_iface_ahead();
    if (two) L->ahead[part].fill(parent, t_sub + 1, 0.5f, parent_tau, p.use_temporal);
    const int r = launch_interface_kernels(L, part, p, iface_buffers(L, part, 0), two, st);
    if (r) return r;
    if (ahead_of_step) L->prepared[part].fill(parent, t_sub, temporal_weight, parent_tau, p.use_temporal);
    // level streams (ludwig_execute_timestep_batch): the parent's buffers have been read - the last time for this
    // pair of sub-steps when the values for the second one were produced alongside
    if (parent->ev_consumed && L->own_stream && L->stream == L->own_stream) {
        LW_HIP(hipEventRecord(parent->ev_consumed, st));
        const_cast<LudwigLevel *>(parent)->ev_consumed_set = true;
    }
    return LUDWIG_OK;
}

// The second pair of side buffers of C and the two events that guard its sets - all of it, or nothing: after a failure every slot
// is null again and nothing is counted, so a later batch tries again instead of finding half a set.
static int make_second_iface_set(LudwigLevel *C, size_t n_side, size_t n_src)
{
    if (C->f_iface_b) return LUDWIG_OK;
    Dev<float> side, side2;
    Dev<float4> mac, mac2;
    HipEvent done[2];
    int e = side.alloc(n_side);
    if (!e) e = side2.alloc(n_side);
    if (!e) e = mac.alloc(n_src);
    if (!e) e = mac2.alloc(n_src);
    if (!e) e = done[0].create();
    if (!e) e = done[1].create();
    if (e) return fail(LUDWIG_ERR_HIP, "second set of interface side buffers: %s", hipGetErrorString((hipError_t)e));
    C->f_iface_b = std::move(side); C->f_iface2_b = std::move(side2);
    C->mac_b = std::move(mac); C->mac2_b = std::move(mac2);
    C->ev_pair_done[0] = std::move(done[0]); C->ev_pair_done[1] = std::move(done[1]);
    C->device_bytes += (int64_t)(2 * n_side * sizeof(float) + 2 * n_src * sizeof(float4));
    return LUDWIG_OK;
}

// Parent-side interface pass: `parent` has just stepped t_pair on ITS stream; the interface values its child C needs for sub-steps
// 2 t_pair (temporal weight 0.0) and 2 t_pair + 1 (0.5) are computed right there, behind that step, into set t_pair & 1 of C's side
// buffers. C's stream, the critical chain of a nested case, then runs nothing but stream-collide and Bouzidi launches; the pass
// shares the parent's (low-priority) stream with the parent's own kernels and fills the gaps the finest level leaves.
// Dependencies: the pass reads the parent's new and saved state - same stream, right after the step that made them, before the
// next one that overwrites them (the ev_consumed hand-shake of the child-side pass is not needed); it overwrites the set C read
// two pairs ago - waited for through C's ev_pair_done. Same kernels, same arguments as the child-side pass: same bits.
static int interface_pass_for_child(LudwigLevel *parent, LudwigLevel *C, int64_t t_pair, const LudwigStepFlags *fl)
{
    const int part = LUDWIG_PART_ALL;
    if (C->n_blocks == 0 || C->n_items[part][1] == 0 || parent->external_writer) return LUDWIG_OK;
    SCParams p{};
    fill_pass_params(p, C, parent, 2 * t_pair, parent->tau, 0.0f, fl);
    int rc = build_interface_links(C, parent, p.nx_g, p.ny_g, p.nz_g);
    if (rc) return rc;
    if (C->n_links[part] == 0) return LUDWIG_OK;
    if ((rc = make_second_iface_set(C, (size_t)C->n_iface_blocks * CELLS * Q, (size_t)C->n_sources[part]))) return rc;
    const int set = (int)(t_pair & 1);
    if (C->pair_done_set[set]) LW_HIP(hipStreamWaitEvent(parent->stream, C->ev_pair_done[set], 0));      // C has finished with this set
    if ((rc = launch_interface_kernels(C, part, p, iface_buffers(C, part, set), true, parent->stream))) return rc;
    C->pair_ready.fill(parent, t_pair, 0.0f, parent->tau, p.use_temporal);
    C->pair_ready.set = set;
    C->ahead[part].valid = false;          // the child-side look-ahead buffers (set 0's second half) are about to be / have been reused
    C->prepared[part].valid = false;
    return LUDWIG_OK;
}

// The interface pass of sub-step t_sub, launched before the step itself. It reads the PARENT's buffers and writes this level's
// interface side buffers only, so a level with children can run it before it waits for them (recursive_step).
static int interface_prepass(LudwigLevel *L, const LudwigLevel *parent, int64_t t_sub, float parent_tau, float temporal_weight,
                             const LudwigStepFlags *fl)
{
    const int part = LUDWIG_PART_ALL;
    if (!parent || L->n_blocks == 0 || L->n_items[part][1] == 0) return LUDWIG_OK;
    LW_HIP(hipSetDevice(L->device));
    SCParams p{};
    fill_pass_params(p, L, parent, t_sub, parent_tau, temporal_weight, fl);
    IfaceState state;
    const int r = interface_decide(L, parent, part, p, t_sub, parent_tau, temporal_weight, true, &state);
    if (r || state != IFACE_LAUNCH) return r;
    return interface_launch(L, parent, part, p, t_sub, parent_tau, temporal_weight, true, L->stream);
}

// ---- record step (kernels.hpp "Record step") ------------------------------------------------------------------------------
// From now on this level steps on the f path: somebody reads its arrays without asking (another level's interface pass).
int ban_records(LudwigLevel *L)
{
    L->rec_banned = true;
    const bool behind = !L->f_valid[0] || !L->f_valid[1];
    const int r = ensure_populations(L, -1);
    if (r) return r;
    L->rec_valid[0] = L->rec_valid[1] = false;
    if (behind) LW_HIP(hipStreamSynchronize(L->stream));      // the reader may sit on another stream; this happens once per level
    return LUDWIG_OK;
}

// The level's part of the rule (ludwig_record_step_rule), looked at again after every set_items / upload_meta.
bool record_level_ok(LudwigLevel *L)
{
    if (L->rec_eligible < 0) {
        std::vector<int32_t> flags((size_t)L->n_blocks);
        for (int b = 0; b < L->n_blocks; ++b) flags[b] = L->h_meta[(size_t)b * NBR_STRIDE + NBR_FLAGS];
        const bool one_list = L->n_items_merged[LUDWIG_PART_ALL] == 0 && L->n_items[LUDWIG_PART_ALL][1] == 0 && L->n_items[LUDWIG_PART_ALL][2] > 0;
        L->rec_eligible = one_list && ludwig_record_step_rule(flags.data(), L->n_blocks, L->n_owned, 0, L->has_temporal ? 1 : 0,
                                                              (L->has_post || L->bouzidi_enabled) ? 1 : 0, 0) == 1;
    }
    return L->rec_eligible == 1;
}

// The class-2 work list in the order the record step launches it. The f path's order deals the 8 planes of a run of blocks to the 8
// XCDs (default_items): fine for populations, which no two planes share, but a record plane is wanted by the waves of planes z - 1, z
// and z + 1. LUDWIG_RECORD_ORDER=1 transposes every 8 x 8 tile of workgroups, so that slot 8 j + x of a tile - XCD x - holds what was slot
// 8 x + j: all 8 planes of one run on one XCD. Workgroups stay whole, so the link bits hold. profiles/record_step_order.txt.
int build_record_items(LudwigLevel *L)
{
    const int64_t n = L->n_items[LUDWIG_PART_ALL][2];
    std::vector<int32_t> src((size_t)n), dst;
    LW_HIP(hipMemcpy(src.data(), L->items[LUDWIG_PART_ALL][2], (size_t)n * 4, hipMemcpyDeviceToHost));
    dst = src;
    if (env::record_order() == 1) {
        const int64_t n_wg = n / XRUN;
        for (int64_t t0 = 0; t0 + 64 <= n_wg; t0 += 64)
            for (int j = 0; j < 8; ++j)
                for (int x = 0; x < 8; ++x)
                    for (int w = 0; w < XRUN; ++w) dst[(size_t)(t0 + 8 * j + x) * XRUN + w] = src[(size_t)(t0 + 8 * x + j) * XRUN + w];
    }
    hipError_t e = hipSuccess;
    Dev<int32_t> made;
    upload_table(e, dst, made);
    if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "record work list: %s", hipGetErrorString(e));
    L->rec_items = std::move(made);
    return LUDWIG_OK;
}

// Does this step go by records? Also makes what the record step needs on its first use.
int record_step_wanted(LudwigLevel *L, const LudwigLevel *parent, const LudwigStepFlags *fl, int part, bool *yes)
{
    *yes = false;
    if (env::record_step_off() || L->rec_banned || L->rec_hold || L->external_writer || L->rho_old_pending || parent || part != LUDWIG_PART_ALL ||
        fl->wall_model_active || !record_level_ok(L))
        return LUDWIG_OK;
    if (!L->rec[0]) {
        const size_t n = (size_t)L->n_blocks * R_BLOCK_BYTES / sizeof(float);
        Dev<float> a, b;
        if (a.alloc(n) || b.alloc(n)) {
            (void)hipGetLastError();                 // no room for the records: the f path needs none
            L->rec_banned = true;
            return LUDWIG_OK;
        }
        L->rec[0] = std::move(a); L->rec[1] = std::move(b);
        L->device_bytes += (int64_t)(2 * n * sizeof(float));
    }
    if (!L->rec_items) {
        const int r = build_record_items(L);
        if (r) return r;
    }
    *yes = true;
    return LUDWIG_OK;
}

// Several launches (parts, the two paths) may belong to one sub-step: it counts once.
void count_step(LudwigLevel *L, int64_t t_sub)
{
    if (t_sub != L->last_step_t) { ++L->step_count; L->last_step_t = t_sub; }
}

// ---- from the runtime flags of a launch to the instantiation of its kernel: ONE place each for the f path and the record path ----
using StepKernel = void (*)(SCParams);
// from_records: rec[in] holds the state (wide = 64-bit per-lane record addresses); else it is read from f[in] / vel[in] (wide = the level's)
StepKernel record_step_kernel(bool from_records, bool wide)
{
    if (from_records) return wide ? k_step_records<XRUN, true> : k_step_records<XRUN, false>;
    return wide ? k_records_from_populations<XRUN, true> : k_records_from_populations<XRUN, false>;
}
template <bool GENERAL, bool POST, bool WALL, bool RHO_ONLY>
StepKernel xrun_kernel(bool wide)
{
    return wide ? k_stream_collide_xrun<XRUN, GENERAL, POST, WALL, RHO_ONLY, true> : k_stream_collide_xrun<XRUN, GENERAL, POST, WALL, RHO_ONLY, false>;
}
// (The order in which the instantiations are named here and above is the order of the kernels in the code object. tools/device_code_diff.py
// compares bytes, and the wall-model kernels hold their distance to wall_model_force_mag: keep the order when nothing else changes.)
StepKernel stream_collide_kernel(bool general, bool post, bool wall, bool rho_only, bool wide)
{
    if (!rho_only) {
        // WALL without POST goes through the <POST, WALL> instantiation (no block is flagged for the f_post store, so the null
        // pointer is never used): the register allocator gets <POST = false, WALL = true> down to 96 VGPRs only by spilling
        // 208 B per lane, while the POST variant sits at 88-90 without - same arithmetic, same bits
        // GENERAL without POST needs a 104-byte spill to stay at 96 VGPRs: the POST variant serves it too
        if (general) return wall ? xrun_kernel<true, true, true, false>(wide) : xrun_kernel<true, true, false, false>(wide);
        if (wall) return xrun_kernel<false, true, true, false>(wide);
        return post ? xrun_kernel<false, true, false, false>(wide) : xrun_kernel<false, false, false, false>(wide);
    }
    return general ? xrun_kernel<true, false, false, true>(wide) : xrun_kernel<false, false, false, true>(wide);   // ensure_rho's replay
}

// One whole-level step in -> out that writes records: from rec[in] where that holds the state, else from f[in] / vel[in].
int launch_record_step(LudwigLevel *L, SCParams p, int in, int out, int64_t t_sub)
{
    count_step(L, t_sub);
    L->rho_replay[LUDWIG_PART_ALL].stale = false;     // superseded, as by any whole-level step
    p.items = L->rec_items;
    p.rec_out = L->rec[out];
    p.store_rho = 0;
    const dim3 grid((unsigned)(L->n_items[LUDWIG_PART_ALL][2] / XRUN)), block(64 * XRUN);
    const bool from_records = L->rec_valid[in];
    if (from_records) p.rec_in = L->rec[in];
    // 64-bit per-lane record addresses from 4 GiB of records on (190 650 blocks)
    const bool wide = from_records ? (uint64_t)L->n_blocks * R_BLOCK_BYTES >= (1ull << 32) : L->wide;
    hipLaunchKernelGGL(record_step_kernel(from_records, wide), grid, block, 0, L->stream, p);
    LW_HIP(hipGetLastError());
    L->rec_valid[out] = true;
    L->f_valid[out] = false;
    L->rho_in_rec = out;
    ++L->n_record_steps;
    return LUDWIG_OK;
}

int launch_stream_collide(LudwigLevel *L, const LudwigLevel *parent, int64_t t_sub, float u_curr, float parent_tau,
                          float temporal_weight, const LudwigStepFlags *fl, int part)
{
    if (!L || !fl) return fail(LUDWIG_ERR_INVALID, "null level or flags");
    if (part < 0 || part >= N_PARTS) return fail(LUDWIG_ERR_INVALID, "bad part %d", part);
    if (t_sub < 0) return fail(LUDWIG_ERR_INVALID, "t_sub must be >= 0");
    L->wale_known = true;                     // what ludwig_level_subgrid_* evaluates with
    L->c_wale = fl->c_wale;
    L->nu_bg = fl->nu_sgs_background;
    if (L->n_blocks == 0) return LUDWIG_OK;   // reference src/physics_v2.jl:41
    if (parent && parent->device != L->device) return fail(LUDWIG_ERR_INVALID, "parent level lives on another device");
    LW_HIP(hipSetDevice(L->device));
    const int in = (t_sub % 2 == 0) ? 0 : 1, out = 1 - in;   // reference src/solver_control.jl:35-41
    ++L->version;                                            // this level's fields are about to change
    if (L->old_alias == out) {                               // about to overwrite the buffer that holds the saved state
        const int r = materialize_old(L);
        if (r) return r;
    }
    SCParams p{};
    p.f_in = L->f[in];
    p.f_out = L->f[out];
    p.vel_in = L->vel[in];
    p.vel_out = L->vel[out];
    p.rho = L->rho;
    // reference src/physics_v2.jl:77: store_post_collision = bouzidi_enabled && n_boundary_cells > 0; a rank that owns no
    // Bouzidi cell of a Bouzidi level still stores it when asked to (n_boundary_cells < 0): a peer's cells read its face layer
    p.f_post = L->has_post ? L->f_post : nullptr;
    // rows: the links with q > 0 are the only readers as long as q_min >= 0 (a negative threshold makes every direction of a listed
    // cell a link, src/bouzidi_kernel.jl:44: whole blocks then)
    p.post_rows = (p.f_post && fl->q_min_threshold >= 0.0f) ? L->post_rows : nullptr;
    if (p.f_post) L->post_rows_used = p.post_rows != nullptr;
    p.obstacle = L->obstacle;
    p.sponge = L->sponge;
    p.wall_dist = L->wall_dist;
    p.meta = L->meta;
    fill_pass_params(p, L, parent, t_sub, parent_tau, temporal_weight, fl);
    p.c_wale = fl->c_wale;
    p.nu_bg = fl->nu_sgs_background;
    p.u_inlet = u_curr;
    p.inlet_turbulence = fl->inlet_turbulence;
    p.is_symmetric = fl->is_symmetric ? 1 : 0;
    p.wall_model = fl->wall_model_active ? 1 : 0;
    p.seed = (int32_t)(t_sub % 1000000);        // reference src/physics_v2.jl:76
    p.sponge_blend = fl->sponge_blend_distributions ? 1 : 0;

    if (parent && !parent->rec_banned) {           // the interface pass reads the parent's arrays: they stay populations
        const int r = ban_records(const_cast<LudwigLevel *>(parent));
        if (r) return r;
    }
    {
        bool by_records = false;
        int r = record_step_wanted(L, parent, fl, part, &by_records);
        if (r) return r;
        if (by_records) return launch_record_step(L, p, in, out, t_sub);
        if ((r = ensure_populations(L, -1))) return r;       // the f path: whatever only a record holds comes back first
        L->rec_valid[out] = false;
    }

    // lazy rho: who reads rho before this level's next step?
    if (parent && !parent->rho_eager) {            // a child interpolates from its parent's rho after every parent step
        LudwigLevel *pm = const_cast<LudwigLevel *>(parent);
        pm->rho_eager = true;
        const int r = ensure_rho(pm);
        if (r) return r;
    }
    {
        count_step(L, t_sub);
        const bool store = env::eager_rho() || L->rho_eager || part != LUDWIG_PART_ALL;
        // This launch reuses the previous step's INPUT buffer as its output. A whole-level launch supersedes the elided rho of
        // the previous one (the reference would be overwriting it right now, unread); a part launch covers only some of the
        // cells, so the rest is produced first, while its inputs still exist.
        if (part != LUDWIG_PART_ALL && L->rho_replay[LUDWIG_PART_ALL].stale) {
            const int r = ensure_rho(L);
            if (r) return r;
        }
        L->rho_replay[LUDWIG_PART_ALL].stale = false;
        p.store_rho = store ? 1 : 0;
        // rho_old in the step (save_old_impl): this launch covers every cell and stores rho
        if (L->rho_old_pending) {
            if (part == LUDWIG_PART_ALL && store) p.rho_old_save = L->rho_old;
            else LW_HIP(hipMemcpyAsync(L->rho_old, L->rho, (size_t)L->sk * 4, hipMemcpyDeviceToDevice, L->stream));
            L->rho_old_pending = false;
        }
    }

    const bool post = p.f_post != nullptr, wall = p.wall_model != 0;
    const hipStream_t cs = L->stream;
    // one launch of a work list through the instantiation its blocks need
    auto launch_list = [&](const int32_t *items, int64_t n_items, bool general) -> int {
        if (n_items == 0) return LUDWIG_OK;
        p.items = items;
        const dim3 grid((unsigned)(n_items / XRUN)), block(64 * XRUN);
        hipLaunchKernelGGL(stream_collide_kernel(general, post, wall, false, L->wide), grid, block, 0, cs, p);
        LW_HIP(hipGetLastError());
        return LUDWIG_OK;
    };
    const hipEvent_t parent_wait = L->parent_wait;          // level streams: the parent step this sub-step's interface values come from
    L->parent_wait = nullptr;
    IfaceState istate;
    {
        const int r = interface_decide(L, parent, part, p, t_sub, parent_tau, temporal_weight, false, &istate);
        if (r) return r;
    }
    {
        if (parent_wait) LW_HIP(hipStreamWaitEvent(cs, parent_wait, 0));
        int r;
        if (istate == IFACE_LAUNCH && (r = interface_launch(L, parent, part, p, t_sub, parent_tau, temporal_weight, false, cs))) return r;
        if (L->n_items_merged[part] > 0) {
            if ((r = launch_list(L->items_merged[part], L->n_items_merged[part], true))) return r;
        } else {
            if ((r = launch_list(L->items[part][1], L->n_items[part][1], true))) return r;
            if ((r = launch_list(L->items[part][2], L->n_items[part][2], false))) return r;
        }
    }
    if (!p.store_rho) {
        LudwigLevel::RhoReplay &rr = L->rho_replay[part];
        rr.stale = true;
        rr.t_sub = t_sub;
        rr.p = p;                                    // pointers into this level's (and the parent's) buffers, scalars of the step
    }
    return LUDWIG_OK;
}

// Produce `rho` now if the last step left it unwritten (see LudwigLevel::rho_replay).
int ensure_rho(LudwigLevel *L)
{
    if (L->rho_in_rec >= 0) {          // the last step was a record step: rho is component 0 of its records
        const int r = ensure_populations(L, L->rho_in_rec);
        if (r) return r;
    }
    bool any = false;
    for (int a = 0; a < N_PARTS; ++a) any = any || L->rho_replay[a].stale;
    if (!any) return LUDWIG_OK;
    LW_HIP(hipSetDevice(L->device));
    // somebody reads rho after every step (e.g. a peer rank's finer blocks interpolate from this rank's cells: the halo pack
    // of rho): replaying costs a second pass over f each time, storing costs 4 B per cell - switch
    if (L->last_replay_step == L->step_count - 1) L->rho_eager = true;
    L->last_replay_step = L->step_count;
    for (int part = 0; part < N_PARTS; ++part) {
        LudwigLevel::RhoReplay &rr = L->rho_replay[part];
        if (!rr.stale) continue;
        SCParams p = rr.p;
        p.store_rho = 1;
        for (int c = 1; c < N_CLASSES; ++c) {
            if (L->n_items[part][c] == 0) continue;
            p.items = L->items[part][c];
            const dim3 grid((unsigned)(L->n_items[part][c] / XRUN)), block(64 * XRUN);
            hipLaunchKernelGGL(stream_collide_kernel(c == 1, false, false, true, L->wide), grid, block, 0, L->stream, p);
            LW_HIP(hipGetLastError());
        }
        rr.stale = false;
    }
    return LUDWIG_OK;
}

int launch_bouzidi(LudwigLevel *L, int64_t t_sub, float q_min)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    if (!(L->bouzidi_enabled && L->n_bc > 0)) return LUDWIG_OK;   // reference src/bouzidi_kernel.jl:107-109
    if (q_min < 0.0f && L->post_rows_used)
        return fail(LUDWIG_ERR_STATE, "q_min_threshold < 0 makes every direction a link: the stream-collide call must be given the same "
                                      "threshold (it stored f_post_collision for the links with q > 0 only)");
    ++L->version;
    LW_HIP(hipSetDevice(L->device));
    const int out = (t_sub % 2 == 0) ? 1 : 0;
    BouzidiParams p{};
    p.f_out = L->f[out];
    p.f_post = L->f_post;
    p.q_map = L->q_map;
    p.cell_block = L->cell_block;
    p.cell_x = L->cell_x; p.cell_y = L->cell_y; p.cell_z = L->cell_z;
    p.meta = L->meta;
    p.n_cells = L->n_bc;
    // q > q_min with q_min >= 0 can only hold where q > 0: the compact list; a negative threshold takes every (cell, k)
    const bool compact = q_min >= 0.0f && L->bouzidi_links;
    p.links = compact ? L->bouzidi_links : nullptr;
    p.n_links = L->n_bouzidi_links;
    p.q_min = q_min;
    const int64_t n_threads = compact ? (int64_t)L->n_bouzidi_links : (int64_t)L->n_bc * Q;
    if (n_threads == 0) return LUDWIG_OK;
    hipLaunchKernelGGL(k_bouzidi, dim3((unsigned)((n_threads + 255) / 256)), dim3(256), 0, L->stream, p);
    LW_HIP(hipGetLastError());
    return LUDWIG_OK;
}

// Host <-> device copy of a whole field between the caller's array (reference layout: population-major, reference block order)
// and the device array (block-major, internal block order). One component and the same block order: one copy; otherwise one
// component at a time through `scratch` and a kernel that places every block. K = components, es = element size (1: obstacle,
// 2: q map, else 4). Synchronous on the level's stream.
template <class T>
void place_component(const LudwigLevel *L, void *dev, void *scratch, int K, int k, bool to_device)
{
    const int64_t n = L->sk;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (to_device) hipLaunchKernelGGL(k_component_to_internal<T>, grid, block, 0, L->stream, (T *)dev, (const T *)scratch, L->d_ref2int, n, K, k);
    else hipLaunchKernelGGL(k_component_to_reference<T>, grid, block, 0, L->stream, (T *)scratch, (const T *)dev, L->d_ref2int, n, K, k);
}
int copy_field(LudwigLevel *L, void *dev, void *host, int K, size_t es, bool to_device)
{
    const size_t plane = (size_t)L->sk * es;                   // one component in bytes
    if (plane == 0) return LUDWIG_OK;
    if (K == 1 && !L->d_ref2int) {
        if (to_device) LW_HIP(hipMemcpyAsync(dev, host, plane, hipMemcpyHostToDevice, L->stream));
        else LW_HIP(hipMemcpyAsync(host, dev, plane, hipMemcpyDeviceToHost, L->stream));
        LW_HIP(hipStreamSynchronize(L->stream));
        return LUDWIG_OK;
    }
    if (!L->scratch) LW_HIP((hipError_t)L->scratch.alloc((size_t)L->sk));
    void *const scratch = L->scratch;
    const auto place = es == 1 ? place_component<uint8_t> : (es == 2 ? place_component<uint16_t> : place_component<float>);
    for (int k = 0; k < K; ++k) {
        char *h = (char *)host + (size_t)k * plane;
        if (to_device) {
            LW_HIP(hipMemcpyAsync(scratch, h, plane, hipMemcpyHostToDevice, L->stream));
            place(L, dev, scratch, K, k, true);
        } else {
            place(L, dev, scratch, K, k, false);
            LW_HIP(hipMemcpyAsync(h, scratch, plane, hipMemcpyDeviceToHost, L->stream));
            LW_HIP(hipStreamSynchronize(L->stream));          // pageable destination: the copy must be over before scratch is reused
        }
        LW_HIP(hipGetLastError());
    }
    LW_HIP(hipStreamSynchronize(L->stream));
    return LUDWIG_OK;
}

// Components first..first+K-1 of a block-major device array of K_total components (internal block order) into the caller's array in
// the reference layout: one component at a time into a plane in the reference block order, which is copied out. A result-file call,
// so the plane is allocated per call. Synchronous on the level's stream.
template <class T>
int download_components(const LudwigLevel *L, const T *dev, int K_total, int first, int K, T *host)
{
    const size_t plane = (size_t)L->sk * sizeof(T);
    LW_HIP(hipSetDevice(L->device));
    Dev<T> tmp;
    LW_HIP((hipError_t)tmp.alloc((size_t)L->sk));
    const int64_t n = L->sk;
    for (int k = 0; k < K; ++k) {
        hipLaunchKernelGGL(k_component_to_reference<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, L->stream, tmp.get(), dev,
                           L->d_ref2int.get(), n, K_total, first + k);
        LW_HIP(hipGetLastError());
        LW_HIP(hipMemcpyAsync((char *)host + (size_t)k * plane, tmp, plane, hipMemcpyDeviceToHost, L->stream));
        LW_HIP(hipStreamSynchronize(L->stream));
    }
    return LUDWIG_OK;
}

}  // namespace

extern "C" {

int ludwig_abi_version(void) { return LUDWIG_ABI_VERSION; }

const char *ludwig_last_error(void) { return g_err.c_str(); }

int ludwig_device_count(int *count)
{
    if (!count) return fail(LUDWIG_ERR_INVALID, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(LUDWIG_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return LUDWIG_OK;
}

void ludwig_level_destroy(LudwigLevel *L) { destroy_set(L); }

static int level_create_impl(const LudwigLevelHost *h, int device, LudwigLevel **out, bool x_fastest_memory);

int ludwig_level_create(const LudwigLevelHost *h, int device, LudwigLevel **out)
{
    if (out) *out = nullptr;
    if (!h || !out) return fail(LUDWIG_ERR_INVALID, "null argument");
    const int32_t nb = h->n_blocks;
    if (nb <= 1 || env::reference_block_order() || !h->neighbor_table || !h->map_x || !h->map_y || !h->map_z)
        return level_create_impl(h, device, out, false);
    const int n_owned = h->n_owned > 0 ? h->n_owned : (h->n_owned < 0 ? 0 : nb);
    if (n_owned > nb) return fail(LUDWIG_ERR_INVALID, "n_owned > n_blocks");
    // internal order: owned blocks first (as given), inside each group sorted by (bz, by, bx) - bx fastest
    std::vector<int32_t> int2ref((size_t)nb), ref2int((size_t)nb);
    for (int32_t b = 0; b < nb; ++b) int2ref[b] = b;
    std::stable_sort(int2ref.begin(), int2ref.end(), [&](int32_t a, int32_t c) {
        const bool oa = a < n_owned, oc = c < n_owned;
        if (oa != oc) return oa;
        if (h->map_z[a] != h->map_z[c]) return h->map_z[a] < h->map_z[c];
        if (h->map_y[a] != h->map_y[c]) return h->map_y[a] < h->map_y[c];
        return h->map_x[a] < h->map_x[c];
    });
    for (int32_t i = 0; i < nb; ++i) ref2int[int2ref[i]] = i;
    // the same description with every per-block array permuted and every block id translated (ids are 1-based, 0 = absent)
    LudwigLevelHost hp = *h;
    const size_t n = (size_t)nb;
    std::vector<int32_t> nt(n * 27), mx(n), my(n), mz(n), bp, cellb;
    std::vector<uint8_t> obs, cbnd;
    std::vector<float> spo, wal;
    std::vector<uint16_t> qm;
    for (size_t i = 0; i < n; ++i) {
        const size_t r = (size_t)int2ref[i];
        mx[i] = h->map_x[r]; my[i] = h->map_y[r]; mz[i] = h->map_z[r];
        for (int d = 0; d < 27; ++d) {
            const int32_t v = h->neighbor_table[r + n * d];
            if (v < 0 || v > nb) return fail(LUDWIG_ERR_INVALID, "neighbor_table[%zu,%d] = %d out of range", r + 1, d + 1, v);
            nt[i + n * d] = v > 0 ? ref2int[v - 1] + 1 : 0;
        }
    }
    hp.neighbor_table = nt.data(); hp.map_x = mx.data(); hp.map_y = my.data(); hp.map_z = mz.data();
    auto permute_cells = [&](auto &dst, const auto *src, size_t comps) {
        dst.resize(n * CELLS * comps);
        for (size_t k = 0; k < comps; ++k)
            for (size_t i = 0; i < n; ++i)
                memcpy(&dst[(k * n + i) * CELLS], &src[(k * n + (size_t)int2ref[i]) * CELLS], CELLS * sizeof(dst[0]));
    };
    if (h->obstacle) { permute_cells(obs, h->obstacle, 1); hp.obstacle = obs.data(); }
    if (h->sponge) { permute_cells(spo, h->sponge, 1); hp.sponge = spo.data(); }
    if (h->wall_dist) { permute_cells(wal, h->wall_dist, 1); hp.wall_dist = wal.data(); }
    if (h->bouzidi_q_map && h->n_boundary_cells > 0) { permute_cells(qm, h->bouzidi_q_map, Q); hp.bouzidi_q_map = qm.data(); }
    if (h->bouzidi_cell_block && h->n_boundary_cells > 0) {
        cellb.resize((size_t)h->n_boundary_cells);
        for (int32_t i = 0; i < h->n_boundary_cells; ++i) {
            const int32_t v = h->bouzidi_cell_block[i];
            if (v < 1 || v > nb) return fail(LUDWIG_ERR_INVALID, "bouzidi cell %d out of range", i + 1);
            cellb[i] = ref2int[v - 1] + 1;
        }
        hp.bouzidi_cell_block = cellb.data();
    }
    if (h->comm_boundary) {
        cbnd.resize(n);
        for (size_t i = 0; i < n; ++i) cbnd[i] = h->comm_boundary[int2ref[i]];
        hp.comm_boundary = cbnd.data();
    }
    const size_t nptr = (size_t)h->grid_dim_x * h->grid_dim_y * h->grid_dim_z;
    if (h->block_pointer && nptr > 0) {
        bp.resize(nptr);
        for (size_t i = 0; i < nptr; ++i) {
            const int32_t v = h->block_pointer[i];
            if (v < 0 || v > nb) return fail(LUDWIG_ERR_INVALID, "block_pointer[%zu] = %d out of range", i, v);
            bp[i] = v > 0 ? ref2int[v - 1] + 1 : 0;
        }
        hp.block_pointer = bp.data();
    }
    const int rc = level_create_impl(&hp, device, out, true);   // the description is in the internal order now
    if (rc) return rc;
    LudwigLevel *L = *out;
    L->ref2int.swap(ref2int);
    L->int2ref.swap(int2ref);
    hipError_t e = hipSuccess;
    upload_table(e, L->ref2int, L->d_ref2int);
    if (e != hipSuccess) { ludwig_level_destroy(L); *out = nullptr; return fail(LUDWIG_ERR_HIP, "block order table: %s", hipGetErrorString(e)); }
    return LUDWIG_OK;
}

static int level_create_impl(const LudwigLevelHost *h, int device, LudwigLevel **out, bool x_fastest_memory)
{
    if (out) *out = nullptr;
    if (!h || !out) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (h->n_blocks < 0 || h->level_id < 1 || h->level_id > 30) return fail(LUDWIG_ERR_INVALID, "bad n_blocks/level_id");
    if (h->n_blocks > 0 && (!h->neighbor_table || !h->map_x || !h->map_y || !h->map_z)) return fail(LUDWIG_ERR_INVALID, "neighbor_table and map_x/y/z are required");
    if ((int64_t)h->n_blocks * CELLS * 4 >= (int64_t)1 << 32) return fail(LUDWIG_ERR_INVALID, "n_blocks too large for 32-bit byte offsets (max 2^21 - 1 blocks per level)");
    const int n_owned = h->n_owned > 0 ? h->n_owned : (h->n_owned < 0 ? 0 : h->n_blocks);
    if (n_owned > h->n_blocks) return fail(LUDWIG_ERR_INVALID, "n_owned > n_blocks");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LUDWIG_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(LUDWIG_ERR_INVALID, "device %d out of range (have %d)", device, ndev);
    LW_HIP(hipSetDevice(device));

    std::unique_ptr<LudwigLevel> owner(new (std::nothrow) LudwigLevel());       // the device is current: whatever fails below, it releases
    LudwigLevel *const L = owner.get();
    if (!L) return fail(LUDWIG_ERR_ALLOC, "host allocation failed");
    L->device = device;
    L->x_fastest_memory = x_fastest_memory;
    L->level_id = h->level_id;
    L->n_blocks = h->n_blocks;
    L->n_owned = n_owned;
    L->tau = h->tau;
    L->gdx = h->grid_dim_x; L->gdy = h->grid_dim_y; L->gdz = h->grid_dim_z;
    L->sk = (int64_t)h->n_blocks * CELLS;
    L->wide = (int64_t)h->n_blocks * (int64_t)F_BLOCK_BYTES >= ((int64_t)1 << 32) || env::wide_addr();
    const size_t c = (size_t)L->sk, nb = (size_t)h->n_blocks;
    L->has_temporal = h->enable_temporal_interpolation && nb > 0;            // reference src/blocks.jl:123
    L->bouzidi_enabled = h->n_boundary_cells > 0 && h->bouzidi_q_map;        // reference src/blocks.jl:152
    L->n_bc = L->bouzidi_enabled ? h->n_boundary_cells : 0;
    L->has_post = h->n_boundary_cells != 0 && nb > 0;                         // reference src/blocks.jl:135 (< 0: forced, multi-GPU)
    if (L->bouzidi_enabled && (!h->bouzidi_cell_block || !h->bouzidi_cell_x || !h->bouzidi_cell_y || !h->bouzidi_cell_z))
        return fail(LUDWIG_ERR_INVALID, "bouzidi cell lists missing");

    int rc = LUDWIG_OK;
#define LW_TRY(expr) do { if (rc == LUDWIG_OK) rc = (expr); } while (0)
    LW_TRY(dev_alloc(L, L->f[0], c * Q));
    LW_TRY(dev_alloc(L, L->f[1], c * Q));
    LW_TRY(dev_alloc(L, L->vel[0], c * 3));
    LW_TRY(dev_alloc(L, L->vel[1], c * 3));
    LW_TRY(dev_alloc(L, L->rho, c));
    if (L->has_post) LW_TRY(dev_alloc(L, L->f_post, c * Q));
    if (L->has_temporal) {
        LW_TRY(dev_alloc(L, L->f_old, c * Q));
        LW_TRY(dev_alloc(L, L->rho_old, c));
        LW_TRY(dev_alloc(L, L->vel_old, c * 3));
    }
    LW_TRY(dev_alloc(L, L->obstacle, c));
    LW_TRY(dev_alloc(L, L->sponge, c));
    LW_TRY(dev_alloc(L, L->wall_dist, c));
    LW_TRY(dev_alloc(L, L->meta, nb * NBR_STRIDE));
    const size_t nptr = (size_t)h->grid_dim_x * h->grid_dim_y * h->grid_dim_z;
    if (L->bouzidi_enabled) {
        LW_TRY(dev_alloc(L, L->q_map, c * Q));
        LW_TRY(dev_alloc(L, L->cell_block, (size_t)L->n_bc));
        LW_TRY(dev_alloc(L, L->cell_x, (size_t)L->n_bc));
        LW_TRY(dev_alloc(L, L->cell_y, (size_t)L->n_bc));
        LW_TRY(dev_alloc(L, L->cell_z, (size_t)L->n_bc));
    }
    if (rc != LUDWIG_OK) return rc;

    // metadata rows: neighbours 0-based (-1 absent), flags, block coords
    L->h_meta.assign(nb * NBR_STRIDE, 0);
    for (size_t b = 0; b < nb; ++b) {
        int32_t *row = &L->h_meta[b * NBR_STRIDE];
        bool all = true;
        for (int d = 0; d < 27; ++d) {
            const int32_t v = h->neighbor_table[b + nb * d];
            if (v < 0 || v > h->n_blocks) return fail(LUDWIG_ERR_INVALID, "neighbor_table[%zu,%d] = %d out of range", b + 1, d + 1, v);
            row[d] = v - 1;
            if (d != 13 && v == 0) all = false;
        }
        row[13] = (int32_t)b;   // the block itself; the reference never reads this entry
        row[NBR_FLAGS] = all ? FLAG_ALL_NEIGHBOURS : 0;
        row[NBR_BX] = h->map_x[b]; row[NBR_BY] = h->map_y[b]; row[NBR_BZ] = h->map_z[b];
    }
    if (h->comm_boundary) L->h_comm_boundary.assign(h->comm_boundary, h->comm_boundary + nb);
    scan_flags(L, LUDWIG_OBSTACLE, h->obstacle);
    scan_flags(L, LUDWIG_SPONGE, h->sponge);
    scan_flags(L, LUDWIG_WALL_DIST, h->wall_dist);
    for (int b = 0; b < n_owned; ++b)
        if (L->h_meta[(size_t)b * NBR_STRIDE + NBR_FLAGS] & FLAG_ALL_NEIGHBOURS) ++L->n_fast_blocks;
    for (size_t b = 0; b < nb; ++b) L->h_meta[b * NBR_STRIDE + NBR_GBI] = -1;
    for (int b = 0; b < n_owned; ++b)
        if (!(L->h_meta[(size_t)b * NBR_STRIDE + NBR_FLAGS] & FLAG_ALL_NEIGHBOURS)) L->h_meta[(size_t)b * NBR_STRIDE + NBR_GBI] = L->n_iface_blocks++;

    auto init = [&]() -> int {
        // constructor defaults, reference src/blocks.jl:118-150
        LW_HIP(hipMemsetAsync(L->f[0], 0, c * Q * 4, L->stream));
        LW_HIP(hipMemsetAsync(L->f[1], 0, c * Q * 4, L->stream));
        LW_HIP(hipMemsetAsync(L->vel[0], 0, c * 3 * 4, L->stream));
        LW_HIP(hipMemsetAsync(L->vel[1], 0, c * 3 * 4, L->stream));
        int r = fill(L, L->rho, L->sk, 1.0f);
        if (r) return r;
        if (L->has_post) LW_HIP(hipMemsetAsync(L->f_post, 0, c * Q * 4, L->stream));
        if (L->has_temporal) {
            LW_HIP(hipMemsetAsync(L->f_old, 0, c * Q * 4, L->stream));
            LW_HIP(hipMemsetAsync(L->vel_old, 0, c * 3 * 4, L->stream));
            if ((r = fill(L, L->rho_old, L->sk, 1.0f))) return r;
        }
        if (h->obstacle) LW_HIP(hipMemcpyAsync(L->obstacle, h->obstacle, c, hipMemcpyHostToDevice, L->stream));
        else LW_HIP(hipMemsetAsync(L->obstacle, 0, c, L->stream));
        if (h->sponge) LW_HIP(hipMemcpyAsync(L->sponge, h->sponge, c * 4, hipMemcpyHostToDevice, L->stream));
        else LW_HIP(hipMemsetAsync(L->sponge, 0, c * 4, L->stream));
        if (h->wall_dist) LW_HIP(hipMemcpyAsync(L->wall_dist, h->wall_dist, c * 4, hipMemcpyHostToDevice, L->stream));
        else if ((r = fill(L, L->wall_dist, L->sk, 100.0f))) return r;
        // block_pointer stays on the host: its only use is the static corner lookup of a child's interface links
        if (h->block_pointer && nptr > 0) L->h_block_pointer.assign(h->block_pointer, h->block_pointer + nptr);
        std::vector<int4> bl;               // the links with q > 0: (own cell, k, q bits, cell behind or -1)
        if (L->bouzidi_enabled) {
            {   // host: population-major (already in the internal block order here), device: block-major
                const int r = copy_field(L, L->q_map, const_cast<uint16_t *>(h->bouzidi_q_map), Q, 2, true);
                if (r) return r;
            }
            std::vector<int32_t> cb((size_t)L->n_bc);
            std::vector<int8_t> cx((size_t)L->n_bc), cy((size_t)L->n_bc), cz((size_t)L->n_bc);
            for (int i = 0; i < L->n_bc; ++i) {
                cb[i] = h->bouzidi_cell_block[i] - 1;
                cx[i] = (int8_t)(h->bouzidi_cell_x[i] - 1); cy[i] = (int8_t)(h->bouzidi_cell_y[i] - 1); cz[i] = (int8_t)(h->bouzidi_cell_z[i] - 1);
                if (cb[i] < 0 || cb[i] >= L->n_blocks || cx[i] < 0 || cx[i] > 7 || cy[i] < 0 || cy[i] > 7 || cz[i] < 0 || cz[i] > 7)
                    return fail(LUDWIG_ERR_INVALID, "bouzidi cell %d out of range", i + 1);
            }
            LW_HIP(hipMemcpy(L->cell_block, cb.data(), cb.size() * 4, hipMemcpyHostToDevice));
            LW_HIP(hipMemcpy(L->cell_x, cx.data(), cx.size(), hipMemcpyHostToDevice));
            LW_HIP(hipMemcpy(L->cell_y, cy.data(), cy.size(), hipMemcpyHostToDevice));
            LW_HIP(hipMemcpy(L->cell_z, cz.data(), cz.size(), hipMemcpyHostToDevice));
            const _Float16 *qh = reinterpret_cast<const _Float16 *>(h->bouzidi_q_map);
            for (int i = 0; i < L->n_bc; ++i) {
                const int own = cb[i] * CELLS + cx[i] + 8 * cy[i] + 64 * cz[i];
                for (int k = 0; k < Q; ++k) {
                    const float q = (float)qh[(size_t)own + c * k];
                    if (!(q > 0.0f)) continue;
                    // the cell one step behind along the link (reference src/bouzidi_kernel.jl:47-58): same block, the neighbour block
                    // of the table, or none (-1: the reference falls back to the cell's own value)
                    const int ok = 26 - k;
                    const int nx = cx[i] + CX(ok), ny = cy[i] + CY(ok), nz = cz[i] + CZ(ok);
                    const int ox = nx < 0 ? -1 : (nx >= BS ? 1 : 0), oy = ny < 0 ? -1 : (ny >= BS ? 1 : 0), oz = nz < 0 ? -1 : (nz >= BS ? 1 : 0);
                    const int nbb = (ox | oy | oz) == 0 ? cb[i] : L->h_meta[(size_t)cb[i] * NBR_STRIDE + DIR(ox, oy, oz)];
                    const int behind = nbb >= 0 ? nbb * CELLS + (nx & 7) + 8 * (ny & 7) + 64 * (nz & 7) : -1;
                    int qbits;
                    memcpy(&qbits, &q, 4);
                    bl.push_back(make_int4(own, k, qbits, behind));
                }
            }
            // population-major, cells in memory order inside a population: the lanes of a wave then work on ONE population array at
            // cells that are mostly neighbours along x - their f_post loads and f_out stores share 32-B sectors instead of touching 64
            // different 2-KiB population slices of a few cells (every link writes its own (cell, opp k): the order is free)
            std::sort(bl.begin(), bl.end(), [](const int4 &a, const int4 &c) { return a.y != c.y ? a.y < c.y : a.x < c.x; });
            hipError_t e = hipSuccess;
            Dev<int4> links;
            upload_table(e, bl, links);
            if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "bouzidi links: %s", hipGetErrorString(e));
            L->bouzidi_links = std::move(links);
            L->n_bouzidi_links = (int)bl.size();
        }
        if (L->has_post) {
            // where f_post_collision has a reader: blocks that hold a Bouzidi cell or a cell next to one (a link q < 1/2 reads
            // the cell one step behind, possibly across a block face). No cell list on this rank (forced store, multi-GPU:
            // the readers are a peer's cells), store_post_collision_everywhere or LUDWIG_FULL_POST_COLLISION set: every block, as the reference.
            const bool fixed = h->store_post_collision_everywhere != 0 || env::full_post_collision();
            const bool everywhere = L->n_bc == 0 || fixed;
            L->post_mode = fixed ? 1 : (L->n_bc == 0 ? 2 : 0);
            for (int b = 0; b < L->n_blocks && everywhere; ++b) L->h_meta[(size_t)b * NBR_STRIDE + NBR_FLAGS] |= FLAG_STORE_POST;
            for (int i = 0; i < L->n_bc && !everywhere; ++i) {
                // the cell itself and the 26 cells around it (a link reads f_post one cell behind the boundary cell)
                const int32_t *row = &L->h_meta[(size_t)(h->bouzidi_cell_block[i] - 1) * NBR_STRIDE];
                const int x = h->bouzidi_cell_x[i] - 1, y = h->bouzidi_cell_y[i] - 1, z = h->bouzidi_cell_z[i] - 1;
                for (int oz = (z == 0 ? -1 : 0); oz <= (z == 7 ? 1 : 0); ++oz)
                    for (int oy = (y == 0 ? -1 : 0); oy <= (y == 7 ? 1 : 0); ++oy)
                        for (int ox = (x == 0 ? -1 : 0); ox <= (x == 7 ? 1 : 0); ++ox) {
                            const int nb2 = row[DIR(ox, oy, oz)];
                            if (nb2 >= 0) L->h_meta[(size_t)nb2 * NBR_STRIDE + NBR_FLAGS] |= FLAG_STORE_POST;
                        }
            }
            // inside those blocks: the x-rows a link with q > 0 reads - its own cell and the cell one step behind
            // (LUDWIG_POST_ROWS=0: whole blocks, round 2's granularity)
            if (!fixed && !env::post_rows_off()) {
                L->h_post_rows.assign((size_t)L->n_blocks * 2, 0u);
                auto mark = [&](int cell) { const int row = (cell & (CELLS - 1)) >> 3; L->h_post_rows[(size_t)(cell / CELLS) * 2 + (row >> 5)] |= 1u << (row & 31); };
                for (const int4 &l : bl) { mark(l.x); if (l.w >= 0) mark(l.w); }
                if (!everywhere) {
                    const int r = upload_post_rows(L);
                    if (r) return r;
                }
            }
        }
        LW_HIP(hipStreamSynchronize(L->stream));
        int r2 = upload_meta(L);
        if (r2) return r2;
        for (int part = 0; part < N_PARTS; ++part)
            if ((r2 = default_items(L, part))) return r2;
        return LUDWIG_OK;
    };
    rc = nb > 0 ? init() : LUDWIG_OK;
    if (rc != LUDWIG_OK) return rc;
#undef LW_TRY
    *out = owner.release();
    return LUDWIG_OK;
}

int ludwig_level_add_post_collision_readers(LudwigLevel *L, const int64_t *offsets, int64_t n)
{
    if (!L || (!offsets && n > 0) || n < 0) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (!L->has_post) return fail(LUDWIG_ERR_STATE, "level %d has no f_post_collision", L->level_id);
    if (L->post_mode == 1 || L->n_blocks == 0) return LUDWIG_OK;      // every block is stored already, and stays so
    LW_HIP(hipSetDevice(L->device));
    LW_HIP(hipStreamSynchronize(L->stream));
    const int64_t sk = (int64_t)L->n_blocks * CELLS;
    for (int64_t i = 0; i < n; ++i)
        if (offsets[i] < 0 || offsets[i] >= sk * Q) return fail(LUDWIG_ERR_INVALID, "reader offset %lld outside f_post_collision", (long long)i);
    if (L->post_mode == 2) {             // "everything, because nobody said who reads": now somebody has
        for (int b = 0; b < L->n_blocks; ++b) L->h_meta[(size_t)b * NBR_STRIDE + NBR_FLAGS] &= ~FLAG_STORE_POST;
        L->post_mode = 0;
    }
    const bool by_rows = !L->h_post_rows.empty();
    for (int64_t i = 0; i < n; ++i) {
        const int64_t e = offsets[i] % sk;
        int b = (int)(e / CELLS);
        if (!L->ref2int.empty()) b = L->ref2int[b];
        const int row = (int)(e % CELLS) >> 3;
        L->h_meta[(size_t)b * NBR_STRIDE + NBR_FLAGS] |= FLAG_STORE_POST;
        if (by_rows) L->h_post_rows[(size_t)b * 2 + (row >> 5)] |= 1u << (row & 31);
    }
    if (by_rows) {
        const int r = upload_post_rows(L);
        if (r) return r;
    }
    ++L->version;
    return upload_meta(L);
}

int ludwig_level_set_stream(LudwigLevel *L, void *hip_stream)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    L->stream = (hipStream_t)hip_stream;
    return LUDWIG_OK;
}

int ludwig_stream_create(int device, int reserved_cus, void **stream_out)
{
    if (!stream_out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *stream_out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return fail(LUDWIG_ERR_NO_DEVICE, "no HIP device %d", device);
    LW_HIP(hipSetDevice(device));
    hipStream_t st = nullptr;
    if (reserved_cus <= 0) {
        LW_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        *stream_out = st;
        return LUDWIG_OK;
    }
    int n_cu = 0;
    LW_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    if (reserved_cus > n_cu / 2) return fail(LUDWIG_ERR_INVALID, "%d of %d compute units reserved: at most half", reserved_cus, n_cu);
    std::vector<uint32_t> mask((size_t)(n_cu + 31) / 32, 0u);
    for (int i = 0; i < n_cu; ++i) mask[(size_t)i / 32] |= 1u << (i % 32);
    // Bit i of the mask is a CU of XCD i mod 8, and inside an XCD four consecutive CU indices sit in its four shader engines
    // (measured, tools/cu_mask_patterns.py, profiles/r03_cu_mask_patterns.txt: CUs 0, 8, 16, 24 of every XCD off = +51 %, CUs 0-3 of
    // every XCD off = +4.5 %; one CU per XCD off = +6 %, a single CU = +8 %). What a mask costs the stepping kernel is the IMBALANCE between
    // shader engines, not the number of CUs: the cheapest mask that reserves anything takes one CU out of every shader engine of every
    // XCD - 32 mask bits - and costs less than round 2's one-per-XCD pattern. So on 256 CUs the request is rounded up to a multiple of 32
    // (bits 224-255, then 192-223, ...; 64 CUs: +12.6 %).
    int done = 0;
    if (n_cu == 256) {
        const int groups = (reserved_cus + 31) / 32;
        for (int bit = 256 - 32 * groups; bit < 256; ++bit, ++done) mask[(size_t)bit / 32] &= ~(1u << (bit % 32));
    }
    for (int k = 0; done < reserved_cus; ++k) {      // generic / remainder: evenly spaced, skipping bits already cleared
        const int bit = (int)(((int64_t)k * n_cu) / reserved_cus + 5) % n_cu;
        if (mask[(size_t)bit / 32] & (1u << (bit % 32))) { mask[(size_t)bit / 32] &= ~(1u << (bit % 32)); ++done; }
        if (k > 4 * n_cu) break;
    }
    LW_HIP(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
    *stream_out = st;
    return LUDWIG_OK;
}

int ludwig_stream_destroy(int device, void *hip_stream)
{
    if (!hip_stream) return LUDWIG_OK;
    LW_HIP(hipSetDevice(device));
    LW_HIP((hipError_t)HipStreamOps::destroy((hipStream_t)hip_stream));     // the caller owned it (ludwig_stream_create)
    return LUDWIG_OK;
}

int ludwig_level_set_order(LudwigLevel *L, int part, const int32_t *items, int64_t n_items)
{
    if (!L || (!items && n_items > 0)) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (part < 0 || part >= N_PARTS) return fail(LUDWIG_ERR_INVALID, "bad part %d", part);
    LW_HIP(hipSetDevice(L->device));
    LW_HIP(hipStreamSynchronize(L->stream));
    // every (block, z-plane) of the part exactly once
    std::vector<uint8_t> seen((size_t)L->n_owned * 8, 0);
    int64_t expect = 0, real = 0;
    for (int b = 0; b < L->n_owned; ++b)
        if (block_in_part(L, b, part)) expect += 8;
    for (int64_t i = 0; i < n_items; ++i) {
        if (items[i] < 0) continue;
        ++real;
        const int b = items[i] >> 3;
        if (b >= L->n_owned) return fail(LUDWIG_ERR_INVALID, "bad work item %lld", (long long)i);
        if (seen[(size_t)items[i]]++) return fail(LUDWIG_ERR_INVALID, "work item %lld listed twice", (long long)i);
    }
    if (real != expect) return fail(LUDWIG_ERR_INVALID, "order has %lld work items, part has %lld", (long long)real, (long long)expect);
    if (L->ref2int.empty()) return set_items(L, part, items, n_items);
    std::vector<int32_t> tr(items, items + n_items);           // the caller counts blocks in the reference order
    for (int32_t &it : tr)
        if (it >= 0) it = (L->ref2int[it >> 3] << 3) | (it & 7);
    return set_items(L, part, tr.data(), n_items);
}

int ludwig_level_upload(LudwigLevel *L, int field, const void *host, size_t bytes)
{
    if (!L || !host) return fail(LUDWIG_ERR_INVALID, "null argument");
    const FieldDesc d = field_desc(L, field);
    if (!d.ptr || d.bytes == 0) return fail(LUDWIG_ERR_STATE, "field %d is not allocated on this level", field);
    if (bytes != d.bytes) return fail(LUDWIG_ERR_INVALID, "field %d: got %zu bytes, expected %zu", field, bytes, d.bytes);
    LW_HIP(hipSetDevice(L->device));
    ++L->version;
    {
        const int r = before_external_write(L, field);
        if (r) return r;
    }
    const size_t es = (size_t)d.es;
    {
        const FieldDesc dn = field_desc(L, field);             // after before_external_write: the saved state may have moved
        const int r = copy_field(L, dn.ptr, const_cast<void *>(host), dn.comps, es, true);
        if (r) return r;
    }
    if (field == LUDWIG_OBSTACLE || field == LUDWIG_SPONGE || field == LUDWIG_WALL_DIST) {
        if (!L->ref2int.empty()) {                             // the per-block flags are indexed by internal block id
            std::vector<char> tmp(bytes);
            for (size_t i = 0; i < (size_t)L->n_blocks; ++i)
                memcpy(&tmp[i * CELLS * es], (const char *)host + (size_t)L->int2ref[i] * CELLS * es, CELLS * es);
            scan_flags(L, field, tmp.data());
        } else {
            scan_flags(L, field, host);
        }
        return upload_meta(L);
    }
    return LUDWIG_OK;
}

int ludwig_level_download(const LudwigLevel *L, int field, void *host, size_t bytes)
{
    if (!L || !host) return fail(LUDWIG_ERR_INVALID, "null argument");
    const FieldDesc d = field_desc(L, field);
    if (!d.ptr || d.bytes == 0) return fail(LUDWIG_ERR_STATE, "field %d is not allocated on this level", field);
    if (bytes != d.bytes) return fail(LUDWIG_ERR_INVALID, "field %d: got %zu bytes, expected %zu", field, bytes, d.bytes);
    LW_HIP(hipSetDevice(L->device));
    {   // what a record holds of this field comes back first: one parity for f / vel, the last step's for rho
        const bool p0 = field == LUDWIG_F || field == LUDWIG_VEL, p1 = field == LUDWIG_F_TEMP || field == LUDWIG_VEL_TEMP;
        const int r = (p0 || p1) ? ensure_populations(const_cast<LudwigLevel *>(L), p0 ? 0 : 1)
                                 : (field == LUDWIG_RHO ? LUDWIG_OK : ensure_populations(const_cast<LudwigLevel *>(L), -1));
        if (r) return r;
    }
    if (field == LUDWIG_RHO) {
        const int r = ensure_rho(const_cast<LudwigLevel *>(L));
        if (r) return r;
    }
    return copy_field(const_cast<LudwigLevel *>(L), d.ptr, host, d.comps, (size_t)d.es, false);
}

int ludwig_level_block_order(const LudwigLevel *L, int32_t *ref_to_internal)
{
    if (!L || (!ref_to_internal && L->n_blocks > 0)) return fail(LUDWIG_ERR_INVALID, "null argument");
    for (int32_t b = 0; b < L->n_blocks; ++b) ref_to_internal[b] = L->ref2int.empty() ? b : L->ref2int[b];
    return LUDWIG_OK;
}

int ludwig_level_field_ptr(const LudwigLevel *L, int field, void **device_ptr, size_t *bytes)
{
    if (!L || !device_ptr) return fail(LUDWIG_ERR_INVALID, "null argument");
    ++const_cast<LudwigLevel *>(L)->version;
    {   // the caller may write through the pointer: give the saved state its own storage first
        const int r = before_external_write(const_cast<LudwigLevel *>(L), field);
        if (r) return r;
    }
    const FieldDesc d = field_desc(L, field);
    if (!d.ptr || d.bytes == 0) return fail(LUDWIG_ERR_STATE, "field %d is not allocated on this level", field);
    if (field != LUDWIG_OBSTACLE && field != LUDWIG_SPONGE && field != LUDWIG_WALL_DIST) {   // those three feed per-block flags: upload them
        LudwigLevel *m = const_cast<LudwigLevel *>(L);
        m->external_writer = true;
        m->rho_eager = true;
    }
    *device_ptr = d.ptr;
    if (bytes) *bytes = d.bytes;
    return LUDWIG_OK;
}

int ludwig_level_set_rho_store(LudwigLevel *L, int every_step)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    if (every_step) {
        const int r = ensure_rho(L);                // what the last step elided is produced now; from here on every step stores
        if (r) return r;
        L->rho_eager = true;
    } else {
        L->rho_eager = false;                       // steps may elide again; a reader that turns up twice in a row makes it eager again
        L->last_replay_step = -10;
    }
    return LUDWIG_OK;
}

int ludwig_level_field_layout(const LudwigLevel *L, int field, int32_t *components, int64_t *block_stride, int64_t *component_stride)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    const FieldDesc d = field_desc(L, field);
    if (field < 0 || field >= LUDWIG_FIELD_COUNT) return fail(LUDWIG_ERR_INVALID, "bad field %d", field);
    if (components) *components = d.comps;
    if (block_stride) *block_stride = (int64_t)d.comps * CELLS;      // block-major: the components of a block are contiguous
    if (component_stride) *component_stride = CELLS;
    return LUDWIG_OK;
}

int ludwig_init_equilibrium(LudwigLevel *L)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    if (L->n_blocks == 0) return LUDWIG_OK;
    LW_HIP(hipSetDevice(L->device));
    const unsigned grid = (unsigned)((L->sk + 255) / 256);
    ++L->version;
    {
        int r = ensure_populations(L, -1);           // vel and rho stay what the last step made of them; f is populations from here on
        if (r) return r;
        L->rec_valid[0] = L->rec_valid[1] = false;
        r = ensure_rho(L);                           // init_eq! leaves rho alone: it must hold what the last step made of it
        if (r) return r;
    }
    hipLaunchKernelGGL(k_fill_weights, dim3(grid), dim3(256), 0, L->stream, L->f[0], L->sk);
    hipLaunchKernelGGL(k_fill_weights, dim3(grid), dim3(256), 0, L->stream, L->f[1], L->sk);
    if (L->has_temporal) {
        L->old_alias = -1;
        hipLaunchKernelGGL(k_fill_weights, dim3(grid), dim3(256), 0, L->stream, L->f_old, L->sk);
        int r = fill(L, L->rho_old, L->sk, 1.0f);
        if (r) return r;
        LW_HIP(hipMemsetAsync(L->vel_old, 0, (size_t)L->sk * 3 * 4, L->stream));
    }
    LW_HIP(hipGetLastError());
    return LUDWIG_OK;
}

int ludwig_stream_collide(LudwigLevel *L, const LudwigLevel *parent, int64_t t_sub, float u_curr, float parent_tau,
                          float temporal_weight, const LudwigStepFlags *flags, int part)
{
    return launch_stream_collide(L, parent, t_sub, u_curr, parent_tau, temporal_weight, flags, part);
}

int ludwig_bouzidi_correction(LudwigLevel *L, int64_t t_sub, float q_min_threshold) { return launch_bouzidi(L, t_sub, q_min_threshold); }

int ludwig_step(LudwigLevel *L, const LudwigLevel *parent, int64_t t_sub, float u_curr, float parent_tau, float temporal_weight,
                const LudwigStepFlags *flags)
{
    int r = launch_stream_collide(L, parent, t_sub, u_curr, parent_tau, temporal_weight, flags, LUDWIG_PART_ALL);
    if (r) return r;
    return launch_bouzidi(L, t_sub, flags->q_min_threshold);
}

static int save_old_impl(LudwigLevel *L, int64_t t_sub, bool defer_rho);

int ludwig_save_old(LudwigLevel *L, int64_t t_sub) { return save_old_impl(L, t_sub, false); }

static int save_old_impl(LudwigLevel *L, int64_t t_sub, bool defer_rho)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    if (!L->has_temporal) return LUDWIG_OK;   // reference src/blocks.jl:200
    LW_HIP(hipSetDevice(L->device));
    const int in = (t_sub % 2 == 0) ? 0 : 1;
    const size_t c = (size_t)L->sk;
    // f and vel: no copy - the step that follows reads f[in] / vel[in] and never writes them (see old_alias)
    ++L->version;
    if (L->external_writer) {            // somebody holds raw pointers into f / vel: a real copy, as the reference does
        L->old_alias = -1;
        LW_HIP(hipMemcpyAsync(L->f_old, L->f[in], c * Q * 4, hipMemcpyDeviceToDevice, L->stream));
        LW_HIP(hipMemcpyAsync(L->vel_old, L->vel[in], c * 3 * 4, hipMemcpyDeviceToDevice, L->stream));
    } else {
        L->old_alias = in;
    }
    L->rho_eager = true;                             // a level that saves its old state has children reading rho every step
    {
        const int r = ensure_rho(L);
        if (r) return r;
    }
    if (defer_rho && L->n_owned == L->n_blocks && !L->external_writer && !env::rho_old_copy()) {
        L->rho_old_pending = true;                   // the step that follows saves it cell by cell (launch_stream_collide)
        return LUDWIG_OK;
    }
    L->rho_old_pending = false;
    LW_HIP(hipMemcpyAsync(L->rho_old, L->rho, c * 4, hipMemcpyDeviceToDevice, L->stream));
    return LUDWIG_OK;
}

// ---- what the observers share (statistics, gradient fields, monitor, probes, surface statistics, slices) ----
namespace {

// the output velocity buffer of sub-step t_sub (src/solver_control.jl:35-41)
const float *vel_out(const LudwigLevel *L, int64_t t_sub) { return L->vel[(t_sub % 2 == 0) ? 1 : 0]; }

// (reference block, cell) as the kernels index it: internal block * 512 + cell
int32_t internal_cell(const LudwigLevel *L, int32_t b, int32_t x) { return (L->ref2int.empty() ? b : L->ref2int[b]) * CELLS + x; }

// rho as ludwig_level_download(LUDWIG_RHO) would return it now: an elided store is replayed first, on the level's stream
#define LW_ENSURE_RHO(L)                                                                                  \
    do {                                                                                                  \
        LW_ENSURE_POPULATIONS(L);                                                                         \
        const int r_ = ensure_rho(const_cast<LudwigLevel *>(L));                                          \
        if (r_) return r_;                                                                                \
    } while (0)

int set_device(int device)
{
    LW_HIP(hipSetDevice(device));
    return LUDWIG_OK;
}

// One trilinear stencil point p of a probe or slice set ("probe", "slice point"; `set` = "probes", "slices"): its level, which must be
// on the device of the first one seen, and its 8 corners and 3 weights.
int check_stencil_point(const char *noun, const char *set, int32_t p, LudwigLevel *const *levels, int32_t n_levels, const int32_t *level_index,
                        const int32_t *blocks, const int32_t *cells, const float *weights, const LudwigLevel *&first)
{
    const int li = level_index[p];
    if (li < 0 || li >= n_levels) return fail(LUDWIG_ERR_INVALID, "%s %d: level index %d not in 0..%d", noun, p, li, n_levels - 1);
    const LudwigLevel *L = levels[li];
    if (!L) return fail(LUDWIG_ERR_INVALID, "%s %d: level %d is null", noun, p, li);
    if (first && L->device != first->device) return fail(LUDWIG_ERR_INVALID, "%s: levels on different devices", set);
    if (!first) first = L;
    // the kernel indexes cells as internal block * 512 + cell in 32 bits
    if ((int64_t)L->n_blocks * CELLS > (int64_t)INT32_MAX)
        return fail(LUDWIG_ERR_INVALID, "%s %d: level %d has %d blocks, more than 32-bit cell indices reach", noun, p, li, L->n_blocks);
    for (int c = 0; c < 8; ++c) {
        const int32_t b = blocks[8 * p + c], x = cells[8 * p + c];
        if (b < 0 || b >= L->n_blocks) return fail(LUDWIG_ERR_INVALID, "%s %d corner %d: block %d not in 0..%d", noun, p, c, b, L->n_blocks - 1);
        if (x < 0 || x >= CELLS) return fail(LUDWIG_ERR_INVALID, "%s %d corner %d: cell %d not in 0..511", noun, p, c, x);
    }
    for (int a = 0; a < 3; ++a) {
        const float w = weights[3 * p + a];
        if (!(w >= 0.0f && w <= 1.0f)) return fail(LUDWIG_ERR_INVALID, "%s %d: weight %d = %g not in [0, 1]", noun, p, a, (double)w);
    }
    return LUDWIG_OK;
}

// every level of the set, also one that holds none of its points, is on the device of `first`
int check_one_device(const char *set, LudwigLevel *const *levels, int32_t n_levels, const LudwigLevel *first)
{
    for (int li = 0; li < n_levels; ++li)
        if (levels[li] && levels[li]->device != first->device) return fail(LUDWIG_ERR_INVALID, "%s: levels on different devices", set);
    return LUDWIG_OK;
}

// The cell table of a triangle set (`set` = "surface statistics", "force series", "wall surface"), checked before anything is allocated:
// per triangle, in the caller's order, the nearest fluid cell in the internal block order, or -1 for none.
int triangle_cells(const char *set, const LudwigLevel *L, const LudwigSurfaceParams *sp, int32_t n_tri, const int32_t *blocks,
                   const int32_t *cells, std::vector<int32_t> &hc)
{
    if (!L || !sp || n_tri < 0 || (n_tri > 0 && (!blocks || !cells))) return fail(LUDWIG_ERR_INVALID, "null argument");
    // the kernel indexes cells as internal block * 512 + cell in 32 bits
    if (n_tri > 0 && (int64_t)L->n_blocks * CELLS > (int64_t)INT32_MAX)
        return fail(LUDWIG_ERR_INVALID, "%s: level has %d blocks, more than 32-bit cell indices reach", set, L->n_blocks);
    hc.resize((size_t)n_tri);
    for (int32_t i = 0; i < n_tri; ++i) {
        const int32_t b = blocks[i], x = cells[i];
        if (b < -1 || b >= L->n_blocks) return fail(LUDWIG_ERR_INVALID, "%s: triangle %d: block %d not in -1..%d", set, i, b, L->n_blocks - 1);
        if (b >= 0 && (x < 0 || x >= CELLS)) return fail(LUDWIG_ERR_INVALID, "%s: triangle %d: cell %d not in 0..511", set, i, x);
        hc[i] = b < 0 ? -1 : internal_cell(L, b, x);
    }
    return LUDWIG_OK;
}

// The stencil tables of one level of a probe or flux-plane set: per point 8 corner cells in the internal block order and 3 weights.
struct StencilTables {
    std::vector<int32_t> cell;
    std::vector<float> w;
    void add(const LudwigLevel *L, int64_t p, const int32_t *blocks, const int32_t *cells, const float *weights)
    {
        for (int c = 0; c < 8; ++c) cell.push_back(internal_cell(L, blocks[8 * p + c], cells[8 * p + c]));
        for (int a = 0; a < 3; ++a) w.push_back(weights[3 * p + a]);
    }
    int points() const { return (int)(cell.size() / 8); }
    void upload(hipError_t &e, Dev<int32_t> &d_cell, Dev<float> &d_w) const
    {
        upload_table(e, cell, d_cell);
        upload_table(e, w, d_w);
    }
};

// whether coarse step t is one of start_step, start_step + interval, ...; and how many of first..last are
bool step_sampled(int64_t t, int64_t start_step, int32_t interval)
{
    return t >= start_step && (t - start_step) % interval == 0;
}

int64_t samples_in(int64_t first, int64_t last, int64_t start_step, int32_t interval)
{
    const int64_t lo = std::max(first, start_step);
    if (last < lo) return 0;
    const int64_t k0 = (lo - start_step + interval - 1) / interval, s0 = start_step + k0 * interval;
    return s0 > last ? 0 : (last - s0) / interval + 1;
}

}  // namespace

// ---- probes (ludwig_probes_*; no reference counterpart) ----
// A probe set over a level array: per level the probes it holds (stencil cells in the internal block order, weights, place in the set)
// and one device ring [capacity][n_probes][4] of samples. The host keeps the coarse step of every used slot; _download empties it.
struct LudwigProbes {
    int device = 0;
    int n_levels = 0, n_probes = 0, capacity = 0;
    std::vector<LudwigLevel *> levels;          // borrowed, as given; an entry without probes may be null (a rank that holds no copy of it)
    struct PerLevel {
        int n = 0;
        Dev<int32_t> cell;                      // [n][8] internal block * 512 + cell
        Dev<float> w;                           // [n][3]
        Dev<int32_t> col;                       // [n] place in the set
    };
    std::vector<PerLevel> per;
    Dev<float> ring;
    std::vector<int64_t> slot_step;             // coarse step of each used slot, oldest first
    std::vector<uint64_t> slot_levels;          // bit li: level li has written its probes into the slot
};

namespace {

uint64_t probed_levels_mask(const LudwigProbes *P)
{
    uint64_t m = 0;
    for (int li = 0; li < P->n_levels; ++li)
        if (P->per[li].n > 0) m |= (uint64_t)1 << li;
    return m;
}

// a new slot for coarse step t, every probed level writing it (the batch; the caller has checked the free capacity)
int probes_open_slot(LudwigProbes *P, int64_t t)
{
    P->slot_step.push_back(t);
    P->slot_levels.push_back(probed_levels_mask(P));
    return (int)P->slot_step.size() - 1;
}

}  // namespace

static int probes_launch(LudwigProbes *P, int li, int slot, int64_t t_sub)
{
    const LudwigProbes::PerLevel &q = P->per[li];
    if (q.n == 0) return LUDWIG_OK;                       // a level without probes launches nothing
    LudwigLevel *L = P->levels[li];
    LW_ENSURE_RHO(L);                                     // a no-op on the probed levels, which store it every step
    float *out = P->ring + (size_t)slot * P->n_probes * 4;
    hipLaunchKernelGGL(k_probe_sample, dim3((unsigned)((q.n + 63) / 64)), dim3(64), 0, L->stream, out, q.cell, q.w, q.col, q.n, L->rho,
                       vel_out(L, t_sub));
    LW_HIP(hipGetLastError());
    return LUDWIG_OK;
}

// ---- surface statistics (ludwig_surface_stats_*; no reference counterpart) ----
// Per triangle, in the caller's order: the nearest fluid cell in the internal block order (-1: none), and [4][n] floats of wall distance
// and normal; [SURFACE_STAT_COMPONENTS][n] float64 sums. The set does not own its level.
struct LudwigSurfaceStats {
    LudwigLevel *level = nullptr;               // borrowed
    int device = 0, n_tri = 0;
    float tau = 0.0f, pressure_scale = 0.0f, stress_scale = 0.0f;
    Dev<int32_t> cell;
    Dev<float> rec;
    Dev<double> sums;
    int64_t n_samples = 0;
};

static int surface_stats_launch(LudwigSurfaceStats *S, int64_t t_sub)
{
    LudwigLevel *L = S->level;
    if (S->n_tri > 0) {
        LW_ENSURE_RHO(L);                                 // a no-op on the level, which stores it every step since the set was made
        hipLaunchKernelGGL(k_accumulate_surface_stats, dim3((unsigned)((S->n_tri + 255) / 256)), dim3(256), 0, L->stream, S->sums, S->cell,
                           S->rec, S->n_tri, L->rho, vel_out(L, t_sub), S->tau, S->pressure_scale, S->stress_scale);
        LW_HIP(hipGetLastError());
    }
    ++S->n_samples;
    return LUDWIG_OK;
}

// ---- force series (ludwig_force_series_*; no reference counterpart) ----
// Per triangle, in the caller's order: the nearest fluid cell in the internal block order (-1: none) and [FORCE_REC_ROWS][n] floats of
// wall distance, normal, area and moment arm; a slab of per-chunk records for the stages of the tree and one device ring [capacity] of
// finished records. The host keeps the coarse step of every used slot; _download empties it. The set does not own its level.
struct LudwigForceSeries {
    LudwigLevel *level = nullptr;               // borrowed
    int device = 0, n_tri = 0, capacity = 0;
    float tau = 0.0f, pressure_scale = 0.0f, stress_scale = 0.0f;
    Dev<int32_t> cell;
    Dev<float> rec;
    Dev<ForceRecord> slab;                      // n_chunks records, then ceil(n / 512) until two or more are left (none for one chunk)
    Dev<ForceRecord> ring;
    std::vector<int64_t> slot_step;             // coarse step of each used slot, oldest first
};

// one record of the state sub-step t_sub wrote into the next free slot (the caller has checked that there is one)
static int force_series_launch(LudwigForceSeries *F, int64_t t_sub, int64_t t_coarse)
{
    LudwigLevel *L = F->level;
    ForceRecord *dst = F->ring + F->slot_step.size();
    if (F->n_tri > 0) {                                   // (no triangle: the record of zeros is made by _download, nothing is launched)
        LW_ENSURE_RHO(L);                                 // a no-op on the level, which stores it every step since the set was made
        int64_t n = ((int64_t)F->n_tri + CELLS - 1) / CELLS;
        ForceRecord *in = F->slab;
        hipLaunchKernelGGL(k_force_chunks, dim3((unsigned)n), dim3(CELLS / 2), 0, L->stream, n == 1 ? dst : in, F->cell, F->rec, F->n_tri,
                           L->rho, vel_out(L, t_sub), F->tau, F->pressure_scale, F->stress_scale);
        LW_HIP(hipGetLastError());
        while (n > 1) {
            const int64_t m = (n + CELLS - 1) / CELLS;
            hipLaunchKernelGGL(k_force_combine, dim3((unsigned)m), dim3(CELLS / 2), 0, L->stream, m == 1 ? dst : in + n, in, n);
            LW_HIP(hipGetLastError());
            in += n;
            n = m;
        }
    }
    F->slot_step.push_back(t_coarse);
    return LUDWIG_OK;
}

// ---- flux planes (ludwig_flux_planes_*; no reference counterpart) ----
// A set over a level array. Per level: the valid points it holds, list after list (one list per plane with points there, in plane
// order; within a list in point order), the chunk table of k_flux_chunks, one table per further stage of k_flux_combine, and a slab for
// the records of every stage but a list's last, which goes into the ring [capacity][n_planes][n_levels]. A (plane, level) pair without
// points has no list and its ring record is never written or read. The host keeps the coarse step of every used slot.
struct LudwigFluxPlanes {
    int device = 0;
    int n_levels = 0, n_planes = 0, capacity = 0;
    std::vector<LudwigLevel *> levels;          // borrowed, as given; an entry without points may be null
    struct PerLevel {
        int n = 0;                              // points
        Dev<int32_t> cell;                      // [n][8] internal block * 512 + cell
        Dev<float> w;                           // [n][3]
        Dev<FluxChunk> table;                   // every stage's workgroups, stage after stage
        std::vector<int> stage_groups;          // workgroups of each stage (the first: k_flux_chunks)
        Dev<FluxRecord> slab;
    };
    std::vector<PerLevel> per;
    std::vector<uint8_t> has_list;              // [n_planes][n_levels]
    Dev<FluxRecord> ring;
    std::vector<int64_t> slot_step;             // coarse step of each used slot, oldest first
};

// a new slot for coarse step t (the caller has checked that there is one)
static int flux_planes_open_slot(LudwigFluxPlanes *P, int64_t t)
{
    P->slot_step.push_back(t);
    return (int)P->slot_step.size() - 1;
}

// level li's lists of the state sub-step t_sub wrote, reduced into ring slot `slot` on the level's stream
static int flux_planes_launch(LudwigFluxPlanes *P, int li, int slot, int64_t t_sub)
{
    const LudwigFluxPlanes::PerLevel &q = P->per[li];
    if (q.n == 0) return LUDWIG_OK;                       // a level without points launches nothing
    LudwigLevel *L = P->levels[li];
    LW_ENSURE_RHO(L);                                     // a no-op on these levels, which store it every step since the set was made
    FluxRecord *dst = P->ring + (size_t)slot * P->n_planes * P->n_levels;
    const FluxChunk *tab = q.table;
    for (size_t s = 0; s < q.stage_groups.size(); ++s) {
        const int g = q.stage_groups[s];
        if (s == 0)
            hipLaunchKernelGGL(k_flux_chunks, dim3((unsigned)g), dim3(CELLS / 2), 0, L->stream, q.slab, dst, tab, q.cell, q.w, L->rho,
                               vel_out(L, t_sub));
        else
            hipLaunchKernelGGL(k_flux_combine, dim3((unsigned)g), dim3(CELLS / 2), 0, L->stream, q.slab, dst, tab);
        LW_HIP(hipGetLastError());
        tab += g;
    }
    return LUDWIG_OK;
}

// ---- Fourier modes (ludwig_modes_*; no reference counterpart) ----
// A set over a level array: the weight table [n_rows][n_columns] on the device and, per level with owned blocks, the sums
// [n_blocks][n_columns][MODE_FIELDS][512] in the internal block order (ghost blocks stay zero). The library knows nothing of
// frequencies: a sample adds the state times one table row. The host counts each level's samples; rows come in order.
struct LudwigModes {
    int device = 0;
    int n_levels = 0, n_columns = 0, n_rows = 0;
    std::vector<LudwigLevel *> levels;          // borrowed, as given
    Dev<double> table;
    std::vector<Dev<double>> sums;              // per level; null: no owned blocks
    std::vector<size_t> sums_count;             // doubles in each
    std::vector<int64_t> count;                 // samples of each level since the last reset
};

// the table row of sampled coarse step t
static int64_t modes_row_of(int64_t t, int64_t start_step, int32_t interval, int n_rows)
{
    return ((t - start_step) / interval) % n_rows;
}

// one sample of level li with table row `row` of the state sub-step t_sub wrote, on the level's stream (the caller has checked the row)
static int modes_launch(LudwigModes *S, int li, int64_t t_sub, int64_t row)
{
    if (S->sums[li]) {
        LudwigLevel *L = S->levels[li];
        LW_ENSURE_RHO(L);                                 // a no-op on these levels, which store it every step since the set was made
        hipLaunchKernelGGL(k_accumulate_modes, dim3((unsigned)L->n_owned), dim3(CELLS / 2), 0, L->stream, S->sums[li],
                           (const double *)(S->table + (size_t)row * S->n_columns), S->n_columns, (const float *)L->rho, vel_out(L, t_sub));
        LW_HIP(hipGetLastError());
    }
    ++S->count[li];
    return LUDWIG_OK;
}

// What a batch observes (ludwig_execute_timestep_batch_observed): one typed slot per LUDWIG_OBSERVE_* kind, a null set is not observed.
struct ObserverSchedule {
    int64_t start_step = 0;
    int32_t interval = 1;
    bool due(int64_t t) const { return step_sampled(t, start_step, interval); }
};
struct BatchObservers {
    // every `set` is borrowed: the caller made it and destroys it
    struct : ObserverSchedule { LudwigProbes *set = nullptr; } probes;
    struct : ObserverSchedule { LudwigSurfaceStats *set = nullptr; } surface;
    struct : ObserverSchedule { LudwigForceSeries *set = nullptr; } forces;
    struct : ObserverSchedule { LudwigTracers *set = nullptr; } tracers;
    struct : ObserverSchedule { LudwigFluxPlanes *set = nullptr; } fluxes;
    struct : ObserverSchedule { LudwigModes *set = nullptr; } modes;
    bool any() const { return probes.set || surface.set || forces.set || tracers.set || fluxes.set || modes.set; }
};
// The observers inside one coarse step: the step being run, the probes' ring slot (-1 = not sampled) and whether the surface set and
// the force series sample this step, the flux planes' ring slot (-1 = not sampled) and the modes' table row (-1 = not sampled).
struct BatchHook {
    const BatchObservers *obs = nullptr;
    int64_t t = 0;
    int slot = -1;
    bool surface = false, forces = false;
    int flux_slot = -1;
    int64_t modes_row = -1;
};

static int recursive_step(LudwigLevel *const *levels, int n_levels, int lvl /*1-based*/, int64_t t_sub, const LudwigLevel *parent,
                          float parent_tau, float temporal_weight, float u_vel, const LudwigStepFlags *fl, bool concurrent,
                          const BatchHook *ph = nullptr)
{
    // recursive_step! / recursive_step_temporal!, reference src/solver_control.jl:21-143
    if (lvl > n_levels) return LUDWIG_OK;
    LudwigLevel *L = levels[lvl - 1];
    const bool has_children = lvl < n_levels;
    int rc;
    if (concurrent) {
        // every event operation costs the stream ~7 us between two kernels (kernel trace of the 3-level sphere): wait for a
        // parent step once, not once per sub-step
        // the only reader of the parent is this level's interface pass: the wait for the parent's step goes where that pass goes
        // (launch_stream_collide) - unless the pass is hoisted below
        const bool need_parent = parent && (L->waited_parent != parent || L->waited_gen != parent->stepped_gen);
        // This level's own interface pass reads the parent and writes side buffers: it need not wait for the children to have
        // read THIS level's buffers, only the step behind it must. Running it ahead (hoisted) shortens what is left to do after the
        // wait. That pays when this level is not much smaller than its child - its step then comes in late for the child's next
        // pair of sub-steps (3-level sphere, 1000 blocks under 1728: 25 us late per coarse step, 0.370 -> 0.337 ms) - and costs
        // when the child dwarfs it and nothing was late (wing, 1728 under 5256: 0.848 -> 0.883 ms of added contention).
        // LUDWIG_IFACE_HOIST=0 / 1 overrides the size rule.
        const bool wait_children = has_children && L->ev_consumed_set;
        const bool hoist = wait_children && (env::iface_hoist() >= 0 ? env::iface_hoist() != 0
                                                                     : 20 * (int64_t)L->n_blocks >= 9 * (int64_t)levels[lvl]->n_blocks);
        if (need_parent) {
            // a hoisted pass needs the parent now; otherwise the wait is handed to launch_stream_collide, which waits right before the pass
            if (hoist) LW_HIP(hipStreamWaitEvent(L->stream, parent->ev_stepped, 0));
            else L->parent_wait = parent->ev_stepped;
            L->waited_parent = parent; L->waited_gen = parent->stepped_gen;
        }
        if (wait_children) {
            if (hoist && (rc = interface_prepass(L, parent, t_sub, parent_tau, temporal_weight, fl))) return rc;
            LW_HIP(hipStreamWaitEvent(L->stream, L->ev_consumed, 0));
        }
    }
    if (has_children && fl->use_temporal_interp && L->has_temporal)
        if ((rc = save_old_impl(L, t_sub, true))) return rc;      // rho's part rides in the step's launch where it can
    if ((rc = ludwig_step(L, parent, t_sub, u_vel, parent_tau, temporal_weight, fl))) return rc;
    const bool parent_side = !env::child_side_iface();
    if (concurrent && parent && parent_side && (t_sub & 1) && L->ev_pair_done[0]) {
        // this level has read the last of set (t_sub >> 1) & 1 of its interface values: the parent's stream may overwrite it
        const int set = (int)((t_sub >> 1) & 1);
        LW_HIP(hipEventRecord(L->ev_pair_done[set], L->stream));
        L->pair_done_set[set] = true;
    }
    if (concurrent && has_children) {
        if (parent_side && (rc = interface_pass_for_child(L, levels[lvl], t_sub, fl))) return rc;
        LW_HIP(hipEventRecord(L->ev_stepped, L->stream));
        ++L->stepped_gen;
    }
    if (ph && (ph->slot >= 0 || ph->surface || ph->forces || ph->flux_slot >= 0 || ph->modes_row >= 0)) {
        // the level's last sub-step of a sampled coarse step: the probes and the surface sets of this level read its newest rho / vel
        // on its own stream, behind the step (and behind the event its children wait for) and ahead of the next write to either
        const int64_t m = (int64_t)1 << (lvl - 1);
        if (t_sub == m * ph->t + m - 1) {
            const BatchObservers &o = *ph->obs;
            if (ph->slot >= 0 && (rc = probes_launch(o.probes.set, lvl - 1, ph->slot, t_sub))) return rc;
            if (ph->surface && o.surface.set->level == L && (rc = surface_stats_launch(o.surface.set, t_sub))) return rc;
            if (ph->forces && o.forces.set->level == L && (rc = force_series_launch(o.forces.set, t_sub, ph->t))) return rc;
            if (ph->flux_slot >= 0 && (rc = flux_planes_launch(o.fluxes.set, lvl - 1, ph->flux_slot, t_sub))) return rc;
            if (ph->modes_row >= 0 && (rc = modes_launch(o.modes.set, lvl - 1, t_sub, ph->modes_row))) return rc;
        }
    }
    if (has_children) {
        if ((rc = recursive_step(levels, n_levels, lvl + 1, 2 * t_sub, L, L->tau, 0.0f, u_vel, fl, concurrent, ph))) return rc;
        if ((rc = recursive_step(levels, n_levels, lvl + 1, 2 * t_sub + 1, L, L->tau, 0.5f, u_vel, fl, concurrent, ph))) return rc;
    }
    return LUDWIG_OK;
}

int ludwig_sync(const LudwigLevel *L)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    LW_HIP(hipSetDevice(L->device));
    LW_HIP(hipStreamSynchronize(L->stream));
    return LUDWIG_OK;
}

int ludwig_map_surface_stresses(const LudwigLevel *L, int vel_field, int32_t n_tri, const float *centers, const float *normals,
                                const LudwigSurfaceParams *sp, float *pressure, float *shear_x, float *shear_y, float *shear_z)
{
    if (!L || !sp || n_tri < 0 || (n_tri > 0 && (!centers || !normals || !pressure || !shear_x || !shear_y || !shear_z)))
        return fail(LUDWIG_ERR_INVALID, "null argument");
    if (vel_field != LUDWIG_VEL && vel_field != LUDWIG_VEL_TEMP) return fail(LUDWIG_ERR_INVALID, "vel_field must be LUDWIG_VEL or LUDWIG_VEL_TEMP");
    if (n_tri == 0) return LUDWIG_OK;
    if (L->n_blocks == 0 || L->h_block_pointer.size() != (size_t)L->gdx * L->gdy * L->gdz)
        return fail(LUDWIG_ERR_STATE, "level has no blocks or was created without block_pointer");
    if (!(sp->dx > 0.0f) || sp->search_radius < 0 || sp->search_radius > 16) return fail(LUDWIG_ERR_INVALID, "bad dx or search radius");
    LW_HIP(hipSetDevice(L->device));
    LW_ENSURE_RHO(L);
    // scratch: [block_pointer | centers | normals | 4 outputs]; a diagnostics call every few hundred steps, so allocated per call
    const size_t nptr = L->h_block_pointer.size(), n = (size_t)n_tri;
    Dev<float> buf;                                   // 4-byte elements throughout: nptr indices, then 10 n floats
    LW_HIP((hipError_t)buf.alloc(nptr + n * 10));
    int32_t *d_ptr = (int32_t *)buf.get();
    float *d_c = buf + nptr, *d_n = d_c + 3 * n, *d_out = d_n + 3 * n;
    LW_HIP(hipMemcpyAsync(d_ptr, L->h_block_pointer.data(), nptr * 4, hipMemcpyHostToDevice, L->stream));
    LW_HIP(hipMemcpyAsync(d_c, centers, n * 12, hipMemcpyHostToDevice, L->stream));
    LW_HIP(hipMemcpyAsync(d_n, normals, n * 12, hipMemcpyHostToDevice, L->stream));
    SurfaceParams s{};
    s.rho = L->rho;
    s.vel = L->vel[vel_field == LUDWIG_VEL ? 0 : 1];
    s.obstacle = L->obstacle;
    s.block_pointer = d_ptr;
    s.gdx = L->gdx; s.gdy = L->gdy; s.gdz = L->gdz; s.n_tri = n_tri; s.radius = sp->search_radius;
    s.dx = sp->dx; s.tau = sp->tau; s.off_x = sp->offset_x; s.off_y = sp->offset_y; s.off_z = sp->offset_z;
    s.pressure_scale = sp->pressure_scale; s.stress_scale = sp->stress_scale;
    s.centers = d_c; s.normals = d_n;
    s.p = d_out; s.tx = d_out + n; s.ty = d_out + 2 * n; s.tz = d_out + 3 * n;
    hipLaunchKernelGGL(k_map_stresses, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, L->stream, s);
    LW_HIP(hipGetLastError());
    float *outs[4] = {pressure, shear_x, shear_y, shear_z};
    for (int i = 0; i < 4; ++i) LW_HIP(hipMemcpyAsync(outs[i], d_out + (size_t)i * n, n * 4, hipMemcpyDeviceToHost, L->stream));
    LW_HIP(hipStreamSynchronize(L->stream));
    return LUDWIG_OK;
}

int ludwig_level_rho_min(const LudwigLevel *L, float *rho_min)
{
    if (!L || !rho_min) return fail(LUDWIG_ERR_INVALID, "null argument");
    *rho_min = __builtin_inff();
    if (L->n_owned == 0) return LUDWIG_OK;
    LW_HIP(hipSetDevice(L->device));
    LW_ENSURE_RHO(L);
    Dev<int> d;
    LW_HIP((hipError_t)d.alloc(2));
    const int init[2] = {0x7f800000, 0};                  // +inf, "no NaN seen"
    LW_HIP(hipMemcpyAsync(d, init, sizeof init, hipMemcpyHostToDevice, L->stream));
    const int64_t n = (int64_t)L->n_owned * CELLS;
    hipLaunchKernelGGL(k_rho_min, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 2048)), dim3(256), 0, L->stream, L->rho, L->obstacle, n, d);
    LW_HIP(hipGetLastError());
    int res[2] = {init[0], 0};
    LW_HIP(hipMemcpyAsync(res, d, sizeof res, hipMemcpyDeviceToHost, L->stream));
    LW_HIP(hipStreamSynchronize(L->stream));
    memcpy(rho_min, &res[0], sizeof(float));
    if (res[1]) *rho_min = __builtin_nanf("");            // minimum() of the reference propagates NaN (src/diagnostics.jl:71)
    return LUDWIG_OK;
}

int ludwig_level_stats_reset(LudwigLevel *L)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    L->stats_ready = true;
    L->stats_n = 0;
    if (L->n_owned == 0) return LUDWIG_OK;           // no owned blocks: nothing to accumulate, nothing allocated
    LW_HIP(hipSetDevice(L->device));
    const size_t n = (size_t)L->n_blocks * STAT_COMPONENTS * CELLS;
    if (!L->stats) {
        const int r = dev_alloc(L, L->stats, n);
        if (r) { L->stats_ready = false; return r; }
    }
    LW_HIP(hipMemsetAsync(L->stats, 0, n * sizeof(double), L->stream));
    return LUDWIG_OK;
}

int ludwig_level_stats_accumulate(LudwigLevel *L, int64_t t_sub)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    if (!L->stats_ready) return fail(LUDWIG_ERR_STATE, "statistics: accumulate before ludwig_level_stats_reset");
    if (t_sub < 0) return fail(LUDWIG_ERR_INVALID, "statistics: t_sub %lld < 0", (long long)t_sub);
    if (L->n_owned == 0) return LUDWIG_OK;
    LW_HIP(hipSetDevice(L->device));
    LW_ENSURE_RHO(L);
    hipLaunchKernelGGL(k_accumulate_stats, dim3((unsigned)L->n_owned), dim3(CELLS / 2), 0, L->stream, L->stats, L->rho, vel_out(L, t_sub));
    LW_HIP(hipGetLastError());
    ++L->stats_n;
    return LUDWIG_OK;
}

int ludwig_level_monitor(LudwigLevel *L, int64_t t_sub, int64_t *counts, int64_t *cells, float *extremes, double *sums)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    if (!counts || !cells || !extremes || !sums) return fail(LUDWIG_ERR_INVALID, "monitor: null output");
    if (t_sub < 0) return fail(LUDWIG_ERR_INVALID, "monitor: t_sub %lld < 0", (long long)t_sub);
    counts[0] = counts[1] = 0;
    for (int i = 0; i < 16; ++i) cells[i] = -1;
    extremes[0] = __builtin_inff(); extremes[1] = extremes[2] = -__builtin_inff();
    sums[0] = sums[1] = 0.0;
    if (L->n_owned == 0) return LUDWIG_OK;            // no owned blocks: the empty record, nothing allocated
    LW_HIP(hipSetDevice(L->device));
    size_t total = 0;                                  // records of every stage: n_owned, then ceil(n / 512) until one is left
    for (size_t n = (size_t)L->n_owned;; n = (n + CELLS - 1) / CELLS) {
        total += n;
        if (n == 1) break;
    }
    if (!L->monitor_slab) {
        constexpr int32_t limit = 1 << MONITOR_COORD_BITS;
        for (int b = 0; b < L->n_owned; ++b) {
            const int32_t *row = &L->h_meta[(size_t)b * NBR_STRIDE];
            if (row[NBR_BX] < 0 || row[NBR_BX] >= limit || row[NBR_BY] < 0 || row[NBR_BY] >= limit || row[NBR_BZ] < 0 || row[NBR_BZ] >= limit)
                return fail(LUDWIG_ERR_INVALID, "monitor: block coordinates (%d, %d, %d) not in 0..%d", row[NBR_BX], row[NBR_BY], row[NBR_BZ], limit - 1);
        }
        const int r = dev_alloc(L, L->monitor_slab, total);
        if (r) return r;
    }
    LW_ENSURE_RHO(L);
    MonitorRecord *in = L->monitor_slab;
    hipLaunchKernelGGL(k_monitor_blocks, dim3((unsigned)L->n_owned), dim3(CELLS / 2), 0, L->stream, in, L->rho, vel_out(L, t_sub),
                       (const uint8_t *)L->obstacle, (const int32_t *)L->meta, (const int32_t *)L->d_ref2int);
    LW_HIP(hipGetLastError());
    for (int64_t n = L->n_owned; n > 1;) {
        const int64_t m = (n + CELLS - 1) / CELLS;
        hipLaunchKernelGGL(k_monitor_combine, dim3((unsigned)m), dim3(CELLS / 2), 0, L->stream, in + n, in, n);
        LW_HIP(hipGetLastError());
        in += n;
        n = m;
    }
    MonitorRecord rec;
    LW_HIP(hipMemcpyAsync(&rec, in, sizeof rec, hipMemcpyDeviceToHost, L->stream));
    LW_HIP(hipStreamSynchronize(L->stream));
    counts[0] = rec.n_fluid; counts[1] = rec.n_bad;
    extremes[0] = rec.rho_min; extremes[1] = rec.rho_max; extremes[2] = rec.v2_max;
    sums[0] = rec.sum_rho; sums[1] = rec.sum_rho_v2;
    const unsigned long long keys[4] = {rec.key_rho_min, rec.key_rho_max, rec.key_v2_max, rec.key_bad};
    const unsigned long long mask = (1ull << MONITOR_COORD_BITS) - 1;
    for (int i = 0; i < 4; ++i) {
        if (keys[i] == MONITOR_NO_KEY) continue;
        cells[4 * i + 0] = (int64_t)((keys[i] >> (9 + 2 * MONITOR_COORD_BITS)) & mask);
        cells[4 * i + 1] = (int64_t)((keys[i] >> (9 + MONITOR_COORD_BITS)) & mask);
        cells[4 * i + 2] = (int64_t)((keys[i] >> 9) & mask);
        cells[4 * i + 3] = (int64_t)(keys[i] & 511);
    }
    return LUDWIG_OK;
}

// ---- wall diagnostics (ludwig_level_wall_census, ludwig_wall_surface_*; no reference counterpart) ----
static_assert(sizeof(LudwigWallCensus) == sizeof(WallCensusRecord) && LUDWIG_WALL_BINS == WALL_BINS, "the census record is the ABI's");

int ludwig_level_wall_census(LudwigLevel *L, int64_t t_sub, LudwigWallCensus *out)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    if (!out) return fail(LUDWIG_ERR_INVALID, "wall census: null output");
    if (t_sub < 0) return fail(LUDWIG_ERR_INVALID, "wall census: t_sub %lld < 0", (long long)t_sub);
    memset(out, 0, sizeof *out);
    out->min_bits = 0xFFFFFFFFu;
    if (L->n_owned == 0) return LUDWIG_OK;            // no owned blocks: the empty record, nothing allocated
    LW_HIP(hipSetDevice(L->device));
    if (!L->wall_census) {
        const int r = dev_alloc(L, L->wall_census, 1);
        if (r) return r;
    }
    LW_ENSURE_RHO(L);
    LW_HIP(hipMemcpyAsync(L->wall_census, out, sizeof *out, hipMemcpyHostToDevice, L->stream));      // the empty record
    hipLaunchKernelGGL(k_wall_census, dim3((unsigned)L->n_owned), dim3(CELLS / 2), 0, L->stream, L->wall_census, (const float *)L->rho,
                       vel_out(L, t_sub), (const uint8_t *)L->obstacle, (const float *)L->wall_dist, (const int32_t *)L->meta, L->tau);
    LW_HIP(hipGetLastError());
    LW_HIP(hipMemcpyAsync(out, L->wall_census, sizeof *out, hipMemcpyDeviceToHost, L->stream));
    LW_HIP(hipStreamSynchronize(L->stream));
    return LUDWIG_OK;
}

// Per triangle, in the caller's order: the nearest fluid cell in the internal block order (-1: none) and [3][n] floats of normal;
// [WALL_SURFACE_ROWS][n] float32 results. The set does not own its level.
struct LudwigWallSurface {
    LudwigLevel *level = nullptr;               // borrowed
    int device = 0, n_tri = 0;
    float pressure_scale = 0.0f, stress_scale = 0.0f;
    Dev<int32_t> cell;
    Dev<float> nrm, out;
    bool computed = false;
};

void ludwig_wall_surface_destroy(LudwigWallSurface *S) { destroy_set(S); }

int ludwig_wall_surface_create(LudwigLevel *L, int32_t n_tri, const int32_t *blocks, const int32_t *cells, const float *normals,
                               const LudwigSurfaceParams *sp, LudwigWallSurface **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n_tri > 0 && !normals) return fail(LUDWIG_ERR_INVALID, "null argument");
    std::vector<int32_t> hc;
    if (const int r = triangle_cells("wall surface", L, sp, n_tri, blocks, cells, hc)) return r;
    std::vector<float> hn((size_t)n_tri * 3);
    for (int32_t i = 0; i < n_tri; ++i)
        for (int a = 0; a < 3; ++a) hn[(size_t)a * n_tri + i] = normals[3 * i + a];
    std::unique_ptr<LudwigWallSurface> S(new (std::nothrow) LudwigWallSurface);
    if (!S) return fail(LUDWIG_ERR_ALLOC, "wall surface: out of host memory");
    S->level = L;
    S->device = L->device;
    S->n_tri = n_tri;
    S->pressure_scale = sp->pressure_scale;
    S->stress_scale = sp->stress_scale;
    if (const int r = set_device(S->device)) return r;
    if (n_tri > 0) {
        hipError_t e = hipSuccess;
        upload_table(e, hc, S->cell);
        upload_table(e, hn, S->nrm);
        if (e == hipSuccess) e = (hipError_t)S->out.alloc((size_t)n_tri * WALL_SURFACE_ROWS);
        if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "wall surface: %d triangles: %s", n_tri, hipGetErrorString(e));
    }
    *out = S.release();
    return LUDWIG_OK;
}

int ludwig_wall_surface_compute(LudwigWallSurface *S, int64_t t_sub)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null wall surface set");
    if (t_sub < 0) return fail(LUDWIG_ERR_INVALID, "wall surface: t_sub %lld < 0", (long long)t_sub);
    LudwigLevel *L = S->level;
    if (S->n_tri > 0) {
        LW_HIP(hipSetDevice(S->device));
        LW_ENSURE_RHO(L);
        hipLaunchKernelGGL(k_wall_surface, dim3((unsigned)((S->n_tri + 255) / 256)), dim3(256), 0, L->stream, S->out, (const int32_t *)S->cell,
                           (const float *)S->nrm, S->n_tri, (const float *)L->rho, vel_out(L, t_sub), (const uint8_t *)L->obstacle,
                           (const float *)L->wall_dist, L->tau, S->pressure_scale, S->stress_scale);
        LW_HIP(hipGetLastError());
    }
    S->computed = true;
    return LUDWIG_OK;
}

int ludwig_wall_surface_download(LudwigWallSurface *S, float *values, size_t bytes)
{
    if (!S || (!values && bytes > 0)) return fail(LUDWIG_ERR_INVALID, "null argument");
    const size_t want = (size_t)S->n_tri * WALL_SURFACE_ROWS * sizeof(float);
    if (bytes != want) return fail(LUDWIG_ERR_INVALID, "wall surface: got %zu bytes, expected %zu", bytes, want);
    if (!S->computed) return fail(LUDWIG_ERR_STATE, "wall surface: download before ludwig_wall_surface_compute");
    if (want == 0) return LUDWIG_OK;
    LW_HIP(hipSetDevice(S->device));
    LW_HIP(hipStreamSynchronize(S->level->stream));
    LW_HIP(hipMemcpy(values, S->out, want, hipMemcpyDeviceToHost));
    return LUDWIG_OK;
}

int ludwig_level_stats_download(const LudwigLevel *L, int stat, double *host, size_t bytes, int64_t *n_samples)
{
    if (!L || (!host && bytes > 0)) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (stat < LUDWIG_STAT_RHO || stat > LUDWIG_STAT_VEL2) return fail(LUDWIG_ERR_INVALID, "bad statistic %d", stat);
    if (!L->stats_ready) return fail(LUDWIG_ERR_STATE, "statistics: download before ludwig_level_stats_reset");
    const int K = stat == LUDWIG_STAT_RHO ? 1 : stat == LUDWIG_STAT_VEL ? 3 : 6, first = stat == LUDWIG_STAT_RHO ? 0 : stat == LUDWIG_STAT_VEL ? 1 : 4;
    const size_t plane = (size_t)L->sk * sizeof(double);
    if (bytes != plane * K) return fail(LUDWIG_ERR_INVALID, "statistic %d: got %zu bytes, expected %zu", stat, bytes, plane * K);
    if (n_samples) *n_samples = L->stats_n;
    if (plane == 0) return LUDWIG_OK;
    if (!L->stats) {                                  // no owned blocks: every block is a ghost
        memset(host, 0, bytes);
        return LUDWIG_OK;
    }
    return download_components(L, (const double *)L->stats, STAT_COMPONENTS, first, K, host);
}

int ludwig_level_gradient_fields_compute(LudwigLevel *L, int vel_field, float scale)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    if (vel_field != LUDWIG_VEL && vel_field != LUDWIG_VEL_TEMP) return fail(LUDWIG_ERR_INVALID, "vel_field must be LUDWIG_VEL or LUDWIG_VEL_TEMP");
    if (!std::isfinite(scale) || scale == 0.0f) return fail(LUDWIG_ERR_INVALID, "gradient fields: scale %g must be finite and non-zero", (double)scale);
    if (L->n_owned == 0) {                            // no owned blocks: nothing to compute, nothing allocated
        L->grad_ready = true;
        return LUDWIG_OK;
    }
    LW_HIP(hipSetDevice(L->device));
    LW_ENSURE_POPULATIONS(L);
    if (!L->grad) {
        const size_t n = (size_t)L->n_blocks * GRAD_COMPONENTS * CELLS;
        const int r = dev_alloc(L, L->grad, n);
        if (r) return r;
        LW_HIP(hipMemsetAsync(L->grad, 0, n * sizeof(float), L->stream));   // the ghost blocks are never written
    }
    hipLaunchKernelGGL(k_velocity_gradient_fields, dim3((unsigned)L->n_owned), dim3(CELLS / 2), 0, L->stream, L->grad,
                       (const float *)L->vel[vel_field == LUDWIG_VEL ? 0 : 1], (const uint8_t *)L->obstacle, (const int32_t *)L->meta, scale);
    LW_HIP(hipGetLastError());
    L->grad_ready = true;
    return LUDWIG_OK;
}

int ludwig_level_gradient_fields_download(const LudwigLevel *L, int which, float *host, size_t bytes)
{
    if (!L || (!host && bytes > 0)) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (which != LUDWIG_GRAD_VORTICITY && which != LUDWIG_GRAD_Q) return fail(LUDWIG_ERR_INVALID, "bad gradient field %d", which);
    if (!L->grad_ready) return fail(LUDWIG_ERR_STATE, "gradient fields: download before ludwig_level_gradient_fields_compute");
    const int K = which == LUDWIG_GRAD_VORTICITY ? 3 : 1, first = which == LUDWIG_GRAD_VORTICITY ? 0 : 3;
    const size_t plane = (size_t)L->sk * sizeof(float);
    if (bytes != plane * K) return fail(LUDWIG_ERR_INVALID, "gradient field %d: got %zu bytes, expected %zu", which, bytes, plane * K);
    if (plane == 0) return LUDWIG_OK;
    if (!L->grad) {                                   // no owned blocks: every block is a ghost
        memset(host, 0, bytes);
        return LUDWIG_OK;
    }
    return download_components(L, (const float *)L->grad, GRAD_COMPONENTS, first, K, host);
}

// ---- iso-surfaces (ludwig_level_isosurface_*; no reference counterpart) ----
#define LW_ISO_TRY(expr) do { const int r_ = (expr); if (r_) return r_; } while (0)
int ludwig_level_isosurface_extract(LudwigLevel *L, int which, int vel_field, float scale, float value, const uint8_t *skip,
                                    const int32_t *cell_lo, const int32_t *cell_hi, int64_t max_triangles, int64_t *n_triangles)
{
    if (!L || !cell_lo || !cell_hi || !n_triangles) return fail(LUDWIG_ERR_INVALID, "isosurface: null argument");
    *n_triangles = 0;
    if (which < LUDWIG_ISO_DENSITY || which > LUDWIG_ISO_VORTICITY_MAGNITUDE) return fail(LUDWIG_ERR_INVALID, "isosurface: unknown scalar %d", which);
    if (vel_field != LUDWIG_VEL && vel_field != LUDWIG_VEL_TEMP) return fail(LUDWIG_ERR_INVALID, "isosurface: vel_field must be LUDWIG_VEL or LUDWIG_VEL_TEMP");
    if (!std::isfinite(value)) return fail(LUDWIG_ERR_INVALID, "isosurface: value %g must be finite", (double)value);
    if (!std::isfinite(scale)) return fail(LUDWIG_ERR_INVALID, "isosurface: scale %g must be finite", (double)scale);
    const bool gradient = which == LUDWIG_ISO_Q_CRITERION || which == LUDWIG_ISO_VORTICITY_MAGNITUDE;
    if (gradient && scale == 0.0f) return fail(LUDWIG_ERR_INVALID, "isosurface: scale must be non-zero for a scalar of the velocity gradient");
    for (int a = 0; a < 3; ++a)
        if (cell_lo[a] > cell_hi[a]) return fail(LUDWIG_ERR_INVALID, "isosurface: cell_lo[%d] = %d > cell_hi[%d] = %d", a, cell_lo[a], a, cell_hi[a]);
    if (max_triangles < 0) return fail(LUDWIG_ERR_INVALID, "isosurface: max_triangles %lld < 0", (long long)max_triangles);
    if ((int64_t)L->n_blocks * CELLS > (int64_t)INT32_MAX)
        return fail(LUDWIG_ERR_INVALID, "isosurface: level has %d blocks, more than 32-bit vertex keys reach", L->n_blocks);
    if (L->n_owned == 0) {                            // no owned blocks: the empty surface, nothing allocated
        L->iso_n = 0;
        return LUDWIG_OK;
    }
    LW_HIP(hipSetDevice(L->device));
    LW_ENSURE_RHO(L);                                 // the attributes, and the scalar of LUDWIG_ISO_DENSITY
    if (gradient) {
        const int r = ludwig_level_gradient_fields_compute(L, vel_field, scale);
        if (r) return r;
    }
    const float *vel = L->vel[vel_field == LUDWIG_VEL ? 0 : 1];
    const size_t no = (size_t)L->n_owned;
    if (!L->iso_counts) LW_ISO_TRY(dev_alloc(L, L->iso_counts, no));
    if (!L->iso_offsets) LW_ISO_TRY(dev_alloc(L, L->iso_offsets, no));
    if (!L->iso_skip) LW_ISO_TRY(dev_alloc(L, L->iso_skip, no));
    if (!L->ref2int.empty() && !L->d_int2ref) {
        LW_ISO_TRY(dev_alloc(L, L->d_int2ref, (size_t)L->n_blocks));
        LW_HIP(hipMemcpyAsync(L->d_int2ref, L->int2ref.data(), (size_t)L->n_blocks * sizeof(int32_t), hipMemcpyHostToDevice, L->stream));
    }
    IsoArgs a;
    if (which == LUDWIG_ISO_DENSITY) { a.s = L->rho; a.s_stride = CELLS; }
    else if (which == LUDWIG_ISO_Q_CRITERION) { a.s = L->grad + 3 * CELLS; a.s_stride = GRAD_COMPONENTS * CELLS; }
    else {
        if (!L->iso_scalar) LW_ISO_TRY(dev_alloc(L, L->iso_scalar, (size_t)L->sk));
        if (which == LUDWIG_ISO_VELOCITY_MAGNITUDE)
            hipLaunchKernelGGL(k_iso_scalar<ISO_VELOCITY_MAGNITUDE>, dim3((unsigned)L->n_blocks), dim3(CELLS / 2), 0, L->stream, L->iso_scalar, vel);
        else
            hipLaunchKernelGGL(k_iso_scalar<ISO_VORTICITY_MAGNITUDE>, dim3((unsigned)L->n_blocks), dim3(CELLS / 2), 0, L->stream, L->iso_scalar,
                               (const float *)L->grad);
        LW_HIP(hipGetLastError());
        a.s = L->iso_scalar; a.s_stride = CELLS;
    }
    a.obstacle = L->obstacle;
    a.meta = L->meta;
    a.ref2int = L->d_ref2int;
    a.skip = L->iso_skip;
    for (int i = 0; i < 3; ++i) { a.lo[i] = cell_lo[i]; a.hi[i] = cell_hi[i]; }
    a.value = value;
    // the owned blocks are the first n_owned of the reference order; the caller's array is read before this call returns (the count
    // below synchronizes)
    if (skip) LW_HIP(hipMemcpyAsync(L->iso_skip, skip, no, hipMemcpyHostToDevice, L->stream));
    else LW_HIP(hipMemsetAsync(L->iso_skip, 0, no, L->stream));
    hipLaunchKernelGGL(k_iso_count, dim3((unsigned)no), dim3(CELLS / 2), 0, L->stream, L->iso_counts, a);
    LW_HIP(hipGetLastError());
    std::vector<int32_t> counts(no);
    LW_HIP(hipMemcpyAsync(counts.data(), L->iso_counts, no * sizeof(int32_t), hipMemcpyDeviceToHost, L->stream));
    LW_HIP(hipStreamSynchronize(L->stream));
    std::vector<int64_t> offsets(no);
    int64_t total = 0;
    for (size_t r = 0; r < no; ++r) {
        offsets[r] = total;
        total += counts[r];
    }
    *n_triangles = total;
    L->iso_n = 0;
    if (total > max_triangles) return LUDWIG_ISO_REFUSED;     // the caller reports it; nothing is allocated for a surface nobody can hold
    if (total == 0) return LUDWIG_OK;
    if (total > L->iso_capacity) {
        L->iso_capacity = 0;                      // sized with the result: released first, so the peak does not grow
        L->iso_pos.reset(); L->iso_att.reset(); L->iso_keys.reset();
        LW_ISO_TRY(dev_alloc(L, L->iso_pos, (size_t)total * ISO_POS_FLOATS));
        LW_ISO_TRY(dev_alloc(L, L->iso_att, (size_t)total * ISO_ATT_FLOATS));
        LW_ISO_TRY(dev_alloc(L, L->iso_keys, (size_t)total * ISO_KEY_INTS));
        L->iso_capacity = total;
    }
    LW_HIP(hipMemcpyAsync(L->iso_offsets, offsets.data(), no * sizeof(int64_t), hipMemcpyHostToDevice, L->stream));
    IsoEmitArgs o;
    o.counts = L->iso_counts;
    o.offsets = L->iso_offsets;
    o.n_triangles = total;
    o.int2ref = L->d_int2ref;
    o.rho = L->rho;
    o.vel = vel;
    o.pos = L->iso_pos;
    o.att = L->iso_att;
    o.keys = L->iso_keys;
    hipLaunchKernelGGL(k_iso_emit, dim3((unsigned)no), dim3(CELLS / 2), 0, L->stream, a, o);
    LW_HIP(hipGetLastError());
    LW_HIP(hipStreamSynchronize(L->stream));                  // `offsets` leaves scope
    L->iso_n = total;
    return LUDWIG_OK;
}

int ludwig_level_isosurface_download(LudwigLevel *L, float *positions, size_t position_bytes, float *attributes, size_t attribute_bytes,
                                     int32_t *keys, size_t key_bytes)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    if (L->iso_n < 0) return fail(LUDWIG_ERR_STATE, "isosurface: download before ludwig_level_isosurface_extract");
    const size_t n = (size_t)L->iso_n;
    const size_t want[3] = {n * ISO_POS_FLOATS * sizeof(float), n * ISO_ATT_FLOATS * sizeof(float), n * ISO_KEY_INTS * sizeof(int32_t)};
    if (position_bytes != want[0] || attribute_bytes != want[1] || key_bytes != want[2])
        return fail(LUDWIG_ERR_INVALID, "isosurface: got %zu, %zu, %zu bytes, expected %zu, %zu, %zu", position_bytes, attribute_bytes, key_bytes,
                    want[0], want[1], want[2]);
    if (n == 0) return LUDWIG_OK;
    if (!positions || !attributes || !keys) return fail(LUDWIG_ERR_INVALID, "isosurface: null output");
    LW_HIP(hipSetDevice(L->device));
    LW_HIP(hipStreamSynchronize(L->stream));
    LW_HIP(hipMemcpy(positions, L->iso_pos, want[0], hipMemcpyDeviceToHost));
    LW_HIP(hipMemcpy(attributes, L->iso_att, want[1], hipMemcpyDeviceToHost));
    LW_HIP(hipMemcpy(keys, L->iso_keys, want[2], hipMemcpyDeviceToHost));
    return LUDWIG_OK;
}
#undef LW_ISO_TRY

// ---- subgrid model (ludwig_level_subgrid_*; no reference counterpart) ----
static int subgrid_model_known(const LudwigLevel *L, const char *what)
{
    if (L->wale_known) return LUDWIG_OK;
    return fail(LUDWIG_ERR_STATE, "subgrid %s: the level has not been stepped yet, so it holds no c_wale / nu_sgs_background", what);
}

int ludwig_level_subgrid_fields_compute(LudwigLevel *L, int vel_field)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    if (vel_field != LUDWIG_VEL && vel_field != LUDWIG_VEL_TEMP) return fail(LUDWIG_ERR_INVALID, "vel_field must be LUDWIG_VEL or LUDWIG_VEL_TEMP");
    if (L->n_owned == 0) {                            // no owned blocks: nothing to compute, nothing allocated
        L->subgrid_fields_ready = true;
        return LUDWIG_OK;
    }
    if (const int r = subgrid_model_known(L, "fields")) return r;
    LW_HIP(hipSetDevice(L->device));
    LW_ENSURE_POPULATIONS(L);
    if (!L->subgrid_fields) {
        const size_t n = (size_t)L->n_blocks * SUBGRID_FIELD_COMPONENTS * CELLS;
        const int r = dev_alloc(L, L->subgrid_fields, n);
        if (r) return r;
        LW_HIP(hipMemsetAsync(L->subgrid_fields, 0, n * sizeof(float), L->stream));   // the ghost blocks are never written
    }
    hipLaunchKernelGGL(k_subgrid<SUBGRID_FIELDS>, dim3((unsigned)L->n_owned), dim3(CELLS / 2), 0, L->stream, L->subgrid_fields,
                       (const float *)L->vel[vel_field == LUDWIG_VEL ? 0 : 1], (const uint8_t *)L->obstacle, (const int32_t *)L->meta,
                       L->c_wale, L->nu_bg);
    LW_HIP(hipGetLastError());
    L->subgrid_fields_ready = true;
    return LUDWIG_OK;
}

int ludwig_level_subgrid_fields_download(const LudwigLevel *L, int which, float *host, size_t bytes)
{
    if (!L || (!host && bytes > 0)) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (which != LUDWIG_SUBGRID_NU && which != LUDWIG_SUBGRID_CODE) return fail(LUDWIG_ERR_INVALID, "bad subgrid field %d", which);
    if (!L->subgrid_fields_ready) return fail(LUDWIG_ERR_STATE, "subgrid fields: download before ludwig_level_subgrid_fields_compute");
    const size_t plane = (size_t)L->sk * sizeof(float);
    if (bytes != plane) return fail(LUDWIG_ERR_INVALID, "subgrid field %d: got %zu bytes, expected %zu", which, bytes, plane);
    if (plane == 0) return LUDWIG_OK;
    if (!L->subgrid_fields) {                         // no owned blocks: every block is a ghost
        memset(host, 0, bytes);
        return LUDWIG_OK;
    }
    return download_components(L, (const float *)L->subgrid_fields, SUBGRID_FIELD_COMPONENTS, which, 1, host);
}

int ludwig_level_subgrid_stats_reset(LudwigLevel *L)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    L->subgrid_stats_ready = true;
    L->subgrid_n = 0;
    if (L->n_owned == 0) return LUDWIG_OK;           // no owned blocks: nothing to accumulate, nothing allocated
    LW_HIP(hipSetDevice(L->device));
    const size_t n = (size_t)L->n_blocks * SUBGRID_SUM_COMPONENTS * CELLS;
    if (!L->subgrid_sums) {
        const int r = dev_alloc(L, L->subgrid_sums, n);
        if (r) { L->subgrid_stats_ready = false; return r; }
    }
    LW_HIP(hipMemsetAsync(L->subgrid_sums, 0, n * sizeof(double), L->stream));
    return LUDWIG_OK;
}

int ludwig_level_subgrid_stats_accumulate(LudwigLevel *L, int64_t t_sub)
{
    if (!L) return fail(LUDWIG_ERR_INVALID, "null level");
    if (!L->subgrid_stats_ready) return fail(LUDWIG_ERR_STATE, "subgrid statistics: accumulate before ludwig_level_subgrid_stats_reset");
    if (t_sub < 0) return fail(LUDWIG_ERR_INVALID, "subgrid statistics: t_sub %lld < 0", (long long)t_sub);
    if (L->n_owned == 0) return LUDWIG_OK;
    if (const int r = subgrid_model_known(L, "statistics")) return r;
    LW_HIP(hipSetDevice(L->device));
    LW_ENSURE_POPULATIONS(L);
    hipLaunchKernelGGL(k_subgrid<SUBGRID_SUMS>, dim3((unsigned)L->n_owned), dim3(CELLS / 2), 0, L->stream, L->subgrid_sums,
                       (const float *)vel_out(L, t_sub), (const uint8_t *)L->obstacle, (const int32_t *)L->meta, L->c_wale, L->nu_bg);
    LW_HIP(hipGetLastError());
    ++L->subgrid_n;
    return LUDWIG_OK;
}

int ludwig_level_subgrid_stats_download(const LudwigLevel *L, int which, double *host, size_t bytes, int64_t *n_samples)
{
    if (!L || (!host && bytes > 0)) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (which < LUDWIG_SUBGRID_SUM_NU || which > LUDWIG_SUBGRID_SUM_EPS) return fail(LUDWIG_ERR_INVALID, "bad subgrid statistic %d", which);
    if (!L->subgrid_stats_ready) return fail(LUDWIG_ERR_STATE, "subgrid statistics: download before ludwig_level_subgrid_stats_reset");
    const size_t plane = (size_t)L->sk * sizeof(double);
    if (bytes != plane) return fail(LUDWIG_ERR_INVALID, "subgrid statistic %d: got %zu bytes, expected %zu", which, bytes, plane);
    if (n_samples) *n_samples = L->subgrid_n;
    if (plane == 0) return LUDWIG_OK;
    if (!L->subgrid_sums) {                           // no owned blocks: every block is a ghost
        memset(host, 0, bytes);
        return LUDWIG_OK;
    }
    return download_components(L, (const double *)L->subgrid_sums, SUBGRID_SUM_COMPONENTS, which, 1, host);
}

void ludwig_probes_destroy(LudwigProbes *P) { destroy_set(P); }

int ludwig_probes_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_probes, const int32_t *level_index,
                         const int32_t *blocks, const int32_t *cells, const float *weights, int32_t capacity, LudwigProbes **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!levels || !level_index || !blocks || !cells || !weights) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (n_levels < 1 || n_levels > 64) return fail(LUDWIG_ERR_INVALID, "probes: n_levels %d not in 1..64", n_levels);
    if (n_probes < 1) return fail(LUDWIG_ERR_INVALID, "probes: n_probes %d < 1", n_probes);
    if (capacity < 1) return fail(LUDWIG_ERR_INVALID, "probes: capacity %d < 1", capacity);
    if ((int64_t)capacity * n_probes * 16 > ((int64_t)1 << 34)) return fail(LUDWIG_ERR_INVALID, "probes: ring of %d x %d samples too large", capacity, n_probes);
    // everything is checked before anything is allocated
    const LudwigLevel *first = nullptr;
    for (int32_t p = 0; p < n_probes; ++p) {
        const int r = check_stencil_point("probe", "probes", p, levels, n_levels, level_index, blocks, cells, weights, first);
        if (r) return r;
    }
    if (const int r = check_one_device("probes", levels, n_levels, first)) return r;
    std::unique_ptr<LudwigProbes> P(new (std::nothrow) LudwigProbes);
    if (!P) return fail(LUDWIG_ERR_ALLOC, "probes: out of host memory");
    P->device = first->device;
    P->n_levels = n_levels;
    P->n_probes = n_probes;
    P->capacity = capacity;
    P->levels.assign(levels, levels + n_levels);
    P->per.resize(n_levels);
    if (const int r = set_device(P->device)) return r;
    for (int li = 0; li < n_levels; ++li) {
        StencilTables st;
        std::vector<int32_t> hcol;
        for (int32_t p = 0; p < n_probes; ++p) {
            if (level_index[p] != li) continue;
            st.add(levels[li], p, blocks, cells, weights);
            hcol.push_back(p);
        }
        LudwigProbes::PerLevel &q = P->per[li];
        q.n = st.points();
        if (q.n == 0) continue;
        hipError_t e = hipSuccess;
        st.upload(e, q.cell, q.w);
        upload_table(e, hcol, q.col);
        if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "probes: level %d tables: %s", li, hipGetErrorString(e));
        // a probe reads rho after the level's last sub-step of every sampled coarse step: the level stores it every step from now
        // on (+4 of 216 B per cell where the store was elided), so a batch never replays it
        if (const int r = ludwig_level_set_rho_store(levels[li], 1)) return r;
    }
    if (const int e = P->ring.alloc((size_t)capacity * n_probes * 4))
        return fail(LUDWIG_ERR_ALLOC, "probes: ring of %d samples: %s", capacity, hipGetErrorString((hipError_t)e));
    *out = P.release();
    return LUDWIG_OK;
}

int ludwig_probes_sample(LudwigProbes *P, int32_t level_index, int64_t t_sub)
{
    if (!P) return fail(LUDWIG_ERR_INVALID, "null probe set");
    if (level_index < 0 || level_index >= P->n_levels) return fail(LUDWIG_ERR_INVALID, "probes: level index %d not in 0..%d", level_index, P->n_levels - 1);
    if (t_sub < 0) return fail(LUDWIG_ERR_INVALID, "probes: t_sub %lld < 0", (long long)t_sub);
    if (P->per[level_index].n == 0) return LUDWIG_OK;
    // the coarse step sub-step t_sub of level index li belongs to: t_sub >> li. Its slot is the newest one when that is for the same
    // step and this level has not written it yet; else a new slot, filled with NaN until every probed level has written its part
    const int64_t step = t_sub >> level_index;
    const uint64_t bit = (uint64_t)1 << level_index;
    LudwigLevel *L = P->levels[level_index];
    // a new slot is NaN-filled on this level's stream and the other levels write their columns of it on theirs: one stream orders both
    for (int li = 0; li < P->n_levels; ++li)
        if (P->per[li].n > 0 && P->levels[li]->stream != L->stream)
            return fail(LUDWIG_ERR_STATE, "probes: levels %d and %d sample on different streams", level_index, li);
    LW_HIP(hipSetDevice(P->device));
    int slot = (int)P->slot_step.size() - 1;
    if (slot < 0 || P->slot_step[slot] != step || (P->slot_levels[slot] & bit)) {
        if ((int)P->slot_step.size() >= P->capacity)
            return fail(LUDWIG_ERR_STATE, "probes: ring full (%d samples): download first", P->capacity);
        slot = (int)P->slot_step.size();
        LW_HIP(hipMemsetAsync(P->ring + (size_t)slot * P->n_probes * 4, 0xff, (size_t)P->n_probes * 16, L->stream));
        P->slot_step.push_back(step);
        P->slot_levels.push_back(0);
    }
    const int r = probes_launch(P, level_index, slot, t_sub);
    if (r) return r;
    P->slot_levels[slot] |= bit;
    return LUDWIG_OK;
}

int ludwig_probes_download(LudwigProbes *P, float *values, int64_t *steps, int32_t max_samples, int32_t *n_samples)
{
    if (!P || !n_samples || max_samples < 0 || (max_samples > 0 && (!values || !steps))) return fail(LUDWIG_ERR_INVALID, "null argument");
    const int n = (int)P->slot_step.size();
    if (n > max_samples) return fail(LUDWIG_ERR_INVALID, "probes: %d samples waiting, room for %d", n, max_samples);
    *n_samples = n;
    if (n == 0) return LUDWIG_OK;
    LW_HIP(hipSetDevice(P->device));
    for (int li = 0; li < P->n_levels; ++li)
        if (P->per[li].n > 0) LW_HIP(hipStreamSynchronize(P->levels[li]->stream));
    LW_HIP(hipMemcpy(values, P->ring, (size_t)n * P->n_probes * 16, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) steps[i] = P->slot_step[i];
    P->slot_step.clear();
    P->slot_levels.clear();
    return LUDWIG_OK;
}

void ludwig_surface_stats_destroy(LudwigSurfaceStats *S) { destroy_set(S); }

int ludwig_surface_stats_create(LudwigLevel *L, int32_t n_tri, const int32_t *blocks, const int32_t *cells, const float *wall_dist,
                                const float *normals, const LudwigSurfaceParams *sp, LudwigSurfaceStats **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n_tri > 0 && (!wall_dist || !normals)) return fail(LUDWIG_ERR_INVALID, "null argument");
    std::vector<int32_t> hc;
    if (const int r = triangle_cells("surface statistics", L, sp, n_tri, blocks, cells, hc)) return r;
    std::vector<float> hr((size_t)n_tri * 4);
    for (int32_t i = 0; i < n_tri; ++i) {
        hr[i] = wall_dist[i];
        for (int a = 0; a < 3; ++a) hr[(size_t)(a + 1) * n_tri + i] = normals[3 * i + a];
    }
    std::unique_ptr<LudwigSurfaceStats> S(new (std::nothrow) LudwigSurfaceStats);
    if (!S) return fail(LUDWIG_ERR_ALLOC, "surface statistics: out of host memory");
    S->level = L;
    S->device = L->device;
    S->n_tri = n_tri;
    S->tau = sp->tau;
    S->pressure_scale = sp->pressure_scale;
    S->stress_scale = sp->stress_scale;
    if (const int r = set_device(S->device)) return r;
    if (n_tri > 0) {
        const size_t n = (size_t)n_tri;
        hipError_t e = hipSuccess;
        upload_table(e, hc, S->cell);
        upload_table(e, hr, S->rec);
        if (e == hipSuccess) e = (hipError_t)S->sums.alloc(n * SURFACE_STAT_COMPONENTS);
        // zeroed on the level's stream: ahead of every sample, which is queued there (or on a batch's level stream, which starts behind it)
        if (e == hipSuccess) e = hipMemsetAsync(S->sums, 0, n * SURFACE_STAT_COMPONENTS * sizeof(double), L->stream);
        if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "surface statistics: %d triangles: %s", n_tri, hipGetErrorString(e));
    }
    // a sample reads rho after the level's last sub-step of every sampled coarse step: the level stores it every step from now on
    // (+4 of 216 B per cell where the store was elided), so a batch never replays it
    if (const int r = ludwig_level_set_rho_store(L, 1)) return r;
    *out = S.release();
    return LUDWIG_OK;
}

int ludwig_surface_stats_reset(LudwigSurfaceStats *S)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null surface statistics set");
    S->n_samples = 0;
    if (S->n_tri == 0) return LUDWIG_OK;
    LW_HIP(hipSetDevice(S->device));
    LW_HIP(hipMemsetAsync(S->sums, 0, (size_t)S->n_tri * SURFACE_STAT_COMPONENTS * sizeof(double), S->level->stream));
    return LUDWIG_OK;
}

int ludwig_surface_stats_accumulate(LudwigSurfaceStats *S, int64_t t_sub)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null surface statistics set");
    if (t_sub < 0) return fail(LUDWIG_ERR_INVALID, "surface statistics: t_sub %lld < 0", (long long)t_sub);
    LW_HIP(hipSetDevice(S->device));
    return surface_stats_launch(S, t_sub);
}

int ludwig_surface_stats_download(LudwigSurfaceStats *S, double *sums, size_t bytes, int64_t *n_samples)
{
    if (!S || (!sums && bytes > 0)) return fail(LUDWIG_ERR_INVALID, "null argument");
    const size_t want = (size_t)S->n_tri * SURFACE_STAT_COMPONENTS * sizeof(double);
    if (bytes != want) return fail(LUDWIG_ERR_INVALID, "surface statistics: got %zu bytes, expected %zu", bytes, want);
    if (n_samples) *n_samples = S->n_samples;
    if (want == 0) return LUDWIG_OK;
    LW_HIP(hipSetDevice(S->device));
    LW_HIP(hipStreamSynchronize(S->level->stream));
    LW_HIP(hipMemcpy(sums, S->sums, want, hipMemcpyDeviceToHost));
    return LUDWIG_OK;
}

// ---- force series (ludwig_force_series_*) ----
void ludwig_force_series_destroy(LudwigForceSeries *F) { destroy_set(F); }

int ludwig_force_series_create(LudwigLevel *L, int32_t n_tri, const int32_t *blocks, const int32_t *cells, const float *wall_dist,
                               const float *normals, const float *area, const float *arm, const LudwigSurfaceParams *sp, int32_t capacity,
                               LudwigForceSeries **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!L || !sp || n_tri < 0 || (n_tri > 0 && (!blocks || !cells || !wall_dist || !normals || !area || !arm)))
        return fail(LUDWIG_ERR_INVALID, "null argument");
    if (capacity < 1) return fail(LUDWIG_ERR_INVALID, "force series: capacity %d < 1", capacity);
    std::vector<int32_t> hc;
    if (const int r = triangle_cells("force series", L, sp, n_tri, blocks, cells, hc)) return r;
    const size_t n = (size_t)n_tri;
    std::vector<float> hr(n * FORCE_REC_ROWS);
    for (int32_t i = 0; i < n_tri; ++i) {
        hr[i] = wall_dist[i];
        for (int a = 0; a < 3; ++a) hr[(size_t)(a + 1) * n + i] = normals[3 * (size_t)i + a];
        hr[4 * n + i] = area[i];
        for (int a = 0; a < 3; ++a) hr[(size_t)(a + 5) * n + i] = arm[(size_t)a * n + i];
    }
    std::unique_ptr<LudwigForceSeries> F(new (std::nothrow) LudwigForceSeries);
    if (!F) return fail(LUDWIG_ERR_ALLOC, "force series: out of host memory");
    F->level = L;
    F->device = L->device;
    F->n_tri = n_tri;
    F->capacity = capacity;
    F->tau = sp->tau;
    F->pressure_scale = sp->pressure_scale;
    F->stress_scale = sp->stress_scale;
    if (const int r = set_device(F->device)) return r;
    if (n_tri > 0) {
        size_t slab = 0;                                   // records of every stage but the last, which goes into the ring
        for (size_t m = (n + CELLS - 1) / CELLS; m > 1; m = (m + CELLS - 1) / CELLS) slab += m;
        hipError_t e = hipSuccess;
        upload_table(e, hc, F->cell);
        upload_table(e, hr, F->rec);
        if (e == hipSuccess) e = (hipError_t)F->slab.alloc(slab);
        if (e == hipSuccess) e = (hipError_t)F->ring.alloc((size_t)capacity);
        if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "force series: %d triangles, %d records: %s", n_tri, capacity, hipGetErrorString(e));
    }
    // a sample reads rho after the level's last sub-step of every sampled coarse step: the level stores it every step from now on
    if (const int r = ludwig_level_set_rho_store(L, 1)) return r;
    *out = F.release();
    return LUDWIG_OK;
}

int ludwig_force_series_sample(LudwigForceSeries *F, int64_t t_sub, int64_t t_coarse)
{
    if (!F) return fail(LUDWIG_ERR_INVALID, "null force series");
    if (t_sub < 0) return fail(LUDWIG_ERR_INVALID, "force series: t_sub %lld < 0", (long long)t_sub);
    if ((int)F->slot_step.size() >= F->capacity)
        return fail(LUDWIG_ERR_STATE, "force series: ring full (%d records): download first", F->capacity);
    LW_HIP(hipSetDevice(F->device));
    return force_series_launch(F, t_sub, t_coarse);
}

int ludwig_force_series_download(LudwigForceSeries *F, double *sums, int64_t *covered, int64_t *steps, int32_t max_samples, int32_t *n_samples)
{
    if (!F || !n_samples || max_samples < 0 || (max_samples > 0 && (!sums || !covered || !steps))) return fail(LUDWIG_ERR_INVALID, "null argument");
    const int n = (int)F->slot_step.size();
    if (n > max_samples) return fail(LUDWIG_ERR_INVALID, "force series: %d records waiting, room for %d", n, max_samples);
    *n_samples = n;
    if (n == 0) return LUDWIG_OK;
    std::vector<ForceRecord> rec((size_t)n);               // value-initialised: the records of a set without triangles
    if (F->n_tri > 0) {
        LW_HIP(hipSetDevice(F->device));
        LW_HIP(hipStreamSynchronize(F->level->stream));
        LW_HIP(hipMemcpy(rec.data(), F->ring, (size_t)n * sizeof(ForceRecord), hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 9; ++k) sums[9 * (size_t)i + k] = rec[i].s[k];
        covered[i] = rec[i].covered;
        steps[i] = F->slot_step[i];
    }
    F->slot_step.clear();
    return LUDWIG_OK;
}

// ---- flux planes (ludwig_flux_planes_*) ----
void ludwig_flux_planes_destroy(LudwigFluxPlanes *P) { destroy_set(P); }

int ludwig_flux_planes_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_planes, const int32_t *plane_start,
                              const int32_t *plane_axis, const int32_t *level_index, const int32_t *blocks, const int32_t *cells,
                              const float *weights, const uint8_t *valid, int32_t capacity, LudwigFluxPlanes **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!levels || n_planes < 0 || (n_planes > 0 && (!plane_start || !plane_axis))) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (n_levels < 1 || n_levels > 64) return fail(LUDWIG_ERR_INVALID, "flux planes: n_levels %d not in 1..64", n_levels);
    if (capacity < 1) return fail(LUDWIG_ERR_INVALID, "flux planes: capacity %d < 1", capacity);
    const int64_t n_points = n_planes > 0 ? plane_start[n_planes] : 0;
    if (n_planes > 0 && plane_start[0] != 0) return fail(LUDWIG_ERR_INVALID, "flux planes: plane_start[0] = %d, not 0", plane_start[0]);
    for (int32_t k = 0; k < n_planes; ++k) {
        if (plane_start[k + 1] < plane_start[k]) return fail(LUDWIG_ERR_INVALID, "flux planes: plane_start decreases at plane %d", k);
        if (plane_axis[k] < 0 || plane_axis[k] > 2) return fail(LUDWIG_ERR_INVALID, "flux planes: plane %d: normal axis %d not in 0..2", k, plane_axis[k]);
    }
    if (n_points > 0 && (!level_index || !blocks || !cells || !weights || !valid)) return fail(LUDWIG_ERR_INVALID, "null argument");
    if ((int64_t)capacity * n_planes * n_levels * (int64_t)sizeof(FluxRecord) > ((int64_t)1 << 34))
        return fail(LUDWIG_ERR_INVALID, "flux planes: ring of %d x %d x %d records too large", capacity, n_planes, n_levels);
    // everything is checked before anything is allocated
    const LudwigLevel *first = nullptr;
    for (int64_t p = 0; p < n_points; ++p) {
        if (!valid[p]) continue;
        const int r = check_stencil_point("flux point", "flux planes", (int32_t)p, levels, n_levels, level_index, blocks, cells, weights, first);
        if (r) return r;
    }
    if (first)
        if (const int r = check_one_device("flux planes", levels, n_levels, first)) return r;
    std::unique_ptr<LudwigFluxPlanes> P(new (std::nothrow) LudwigFluxPlanes);
    if (!P) return fail(LUDWIG_ERR_ALLOC, "flux planes: out of host memory");
    P->n_levels = n_levels;
    P->n_planes = n_planes;
    P->capacity = capacity;
    P->levels.assign(levels, levels + n_levels);
    P->per.resize(n_levels);
    P->has_list.assign((size_t)n_planes * n_levels, 0);
    if (!first) {                                          // no valid point: nothing on the device, records of zeros
        *out = P.release();
        return LUDWIG_OK;
    }
    P->device = first->device;
    if (const int r = set_device(P->device)) return r;
    for (int li = 0; li < n_levels; ++li) {
        StencilTables pts;
        std::vector<std::vector<FluxChunk>> stages(1);
        int32_t slab = 0;                                  // records so far in the level's slab
        for (int32_t k = 0; k < n_planes; ++k) {
            const int32_t start = pts.points();
            for (int64_t p = plane_start[k]; p < plane_start[k + 1]; ++p)
                if (valid[p] && level_index[p] == li) pts.add(levels[li], p, blocks, cells, weights);
            int32_t n = pts.points() - start;
            if (n == 0) continue;
            P->has_list[(size_t)k * n_levels + li] = 1;
            const int32_t final_dst = ~(k * n_levels + li);
            // the list's stages: n elements from `from` (points, then slab records) -> ceil(n / 512) records
            int32_t from = start;
            for (size_t s = 0;; ++s) {
                if (stages.size() <= s) stages.emplace_back();
                const int32_t m = (n + CELLS - 1) / CELLS;
                for (int32_t c = 0; c < m; ++c) stages[s].push_back({from, n, c, m == 1 ? final_dst : slab + c, plane_axis[k], 0});
                if (m == 1) break;
                from = slab;
                slab += m;
                n = m;
            }
        }
        LudwigFluxPlanes::PerLevel &q = P->per[li];
        q.n = pts.points();
        if (q.n == 0) continue;
        std::vector<FluxChunk> table;
        for (const std::vector<FluxChunk> &st : stages) {
            q.stage_groups.push_back((int)st.size());
            table.insert(table.end(), st.begin(), st.end());
        }
        hipError_t e = hipSuccess;
        pts.upload(e, q.cell, q.w);
        upload_table(e, table, q.table);
        if (e == hipSuccess) e = (hipError_t)q.slab.alloc((size_t)slab);
        if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "flux planes: level %d tables: %s", li, hipGetErrorString(e));
        // a sample reads rho after the level's last sub-step of every sampled coarse step: the level stores it every step from now on
        if (const int r = ludwig_level_set_rho_store(levels[li], 1)) return r;
    }
    if (const int e = P->ring.alloc((size_t)capacity * n_planes * n_levels))
        return fail(LUDWIG_ERR_ALLOC, "flux planes: ring of %d records: %s", capacity, hipGetErrorString((hipError_t)e));
    *out = P.release();
    return LUDWIG_OK;
}

int ludwig_flux_planes_sample(LudwigFluxPlanes *P, int64_t t_coarse)
{
    if (!P) return fail(LUDWIG_ERR_INVALID, "null flux plane set");
    if (t_coarse < 0) return fail(LUDWIG_ERR_INVALID, "flux planes: t_coarse %lld < 0", (long long)t_coarse);
    if ((int)P->slot_step.size() >= P->capacity)
        return fail(LUDWIG_ERR_STATE, "flux planes: ring full (%d records): download first", P->capacity);
    if (P->ring) LW_HIP(hipSetDevice(P->device));
    const int slot = flux_planes_open_slot(P, t_coarse);
    for (int li = 0; li < P->n_levels; ++li) {
        // the level's last sub-step of coarse step t_coarse
        const int r = flux_planes_launch(P, li, slot, ((t_coarse + 1) << li) - 1);
        if (r) return r;
    }
    return LUDWIG_OK;
}

int ludwig_flux_planes_download(LudwigFluxPlanes *P, double *sums, int64_t *counts, int64_t *steps, int32_t max_samples, int32_t *n_samples)
{
    if (!P || !n_samples || max_samples < 0 || (max_samples > 0 && (!steps || (P->n_planes > 0 && (!sums || !counts)))))
        return fail(LUDWIG_ERR_INVALID, "null argument");
    const int n = (int)P->slot_step.size();
    if (n > max_samples) return fail(LUDWIG_ERR_INVALID, "flux planes: %d records waiting, room for %d", n, max_samples);
    *n_samples = n;
    if (n == 0) return LUDWIG_OK;
    const size_t per_slot = (size_t)P->n_planes * P->n_levels;
    std::vector<FluxRecord> rec(n * per_slot);
    if (P->ring && per_slot > 0) {
        LW_HIP(hipSetDevice(P->device));
        for (int li = 0; li < P->n_levels; ++li)
            if (P->per[li].n > 0) LW_HIP(hipStreamSynchronize(P->levels[li]->stream));
        LW_HIP(hipMemcpy(rec.data(), P->ring, rec.size() * sizeof(FluxRecord), hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < P->n_planes; ++k) {
            // the levels that hold points of the plane, coarsest first, added left to right; none: +0.0 and 0
            double s[FLUX_ROWS] = {};
            int64_t count = 0;
            bool any = false;
            for (int li = 0; li < P->n_levels; ++li) {
                if (!P->has_list[(size_t)k * P->n_levels + li]) continue;
                const FluxRecord &q = rec[i * per_slot + (size_t)k * P->n_levels + li];
                for (int j = 0; j < FLUX_ROWS; ++j) s[j] = any ? s[j] + q.s[j] : q.s[j];
                count += q.count;
                any = true;
            }
            for (int j = 0; j < FLUX_ROWS; ++j) sums[((size_t)i * P->n_planes + k) * FLUX_ROWS + j] = s[j];
            counts[(size_t)i * P->n_planes + k] = count;
        }
        steps[i] = P->slot_step[i];
    }
    P->slot_step.clear();
    return LUDWIG_OK;
}

// ---- Fourier modes (ludwig_modes_*) ----
void ludwig_modes_destroy(LudwigModes *S) { destroy_set(S); }

int ludwig_modes_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_columns, int32_t n_rows, const double *weights,
                        LudwigModes **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!levels || !weights) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (n_levels < 1 || n_levels > 64) return fail(LUDWIG_ERR_INVALID, "modes: n_levels %d not in 1..64", n_levels);
    if (n_columns < 1 || n_columns > MODE_MAX_COLUMNS)
        return fail(LUDWIG_ERR_INVALID, "modes: %d columns not in 1..%d", n_columns, MODE_MAX_COLUMNS);
    if (n_rows < 1 || n_rows > 65536) return fail(LUDWIG_ERR_INVALID, "modes: %d rows not in 1..65536", n_rows);
    // everything is checked before anything is allocated
    for (int li = 0; li < n_levels; ++li) {
        if (!levels[li]) return fail(LUDWIG_ERR_INVALID, "modes: level %d is null", li + 1);
        if (levels[li]->device != levels[0]->device) return fail(LUDWIG_ERR_INVALID, "modes: levels on different devices");
    }
    std::unique_ptr<LudwigModes> S(new (std::nothrow) LudwigModes);
    if (!S) return fail(LUDWIG_ERR_ALLOC, "modes: out of host memory");
    S->device = levels[0]->device;
    S->n_levels = n_levels;
    S->n_columns = n_columns;
    S->n_rows = n_rows;
    S->levels.assign(levels, levels + n_levels);
    S->sums.resize((size_t)n_levels);
    S->sums_count.assign((size_t)n_levels, 0);
    S->count.assign((size_t)n_levels, 0);
    int r = set_device(S->device);
    if (r) return r;
    const size_t bytes = (size_t)n_rows * n_columns * sizeof(double);
    if (const int e = S->table.alloc((size_t)n_rows * n_columns))
        return fail(LUDWIG_ERR_ALLOC, "modes: hipMalloc(%zu bytes) for the weight table failed: %s", bytes, hipGetErrorString((hipError_t)e));
    if (const hipError_t e = hipMemcpy(S->table, weights, bytes, hipMemcpyHostToDevice))
        return fail(LUDWIG_ERR_HIP, "modes: weight table: %s", hipGetErrorString(e));
    // all or nothing across levels: a level that fails takes the sums of the levels before it along
    for (int li = 0; li < n_levels && r == LUDWIG_OK; ++li) {
        LudwigLevel *L = levels[li];
        if (L->n_owned == 0) continue;                    // no owned blocks: accepted, does nothing
        const size_t n = (size_t)L->n_blocks * n_columns * MODE_FIELDS * CELLS;
        r = dev_alloc(L, S->sums[li], n);
        if (r != LUDWIG_OK) break;
        S->sums_count[li] = n;
        // zeroed on the level's stream: ahead of every sample, which is queued there (or on a batch's level stream, which starts behind it)
        const hipError_t e = hipMemsetAsync(S->sums[li], 0, n * sizeof(double), L->stream);
        if (e != hipSuccess) r = fail(LUDWIG_ERR_HIP, "modes: level %d: %s", li + 1, hipGetErrorString(e));
    }
    // a sample reads rho after the level's last sub-step of every sampled coarse step: every level stores it every step from now on
    // (+4 of 216 B per cell where the store was elided), so a batch never replays it
    for (int li = 0; li < n_levels && r == LUDWIG_OK; ++li) r = ludwig_level_set_rho_store(levels[li], 1);
    if (r != LUDWIG_OK) {
        for (int li = 0; li < n_levels; ++li)
            if (S->sums[li]) levels[li]->device_bytes -= (int64_t)(S->sums_count[li] * sizeof(double));
        return r;
    }
    *out = S.release();
    return LUDWIG_OK;
}

int ludwig_modes_reset(LudwigModes *S)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null mode set");
    LW_HIP(hipSetDevice(S->device));
    for (int li = 0; li < S->n_levels; ++li) {
        S->count[li] = 0;
        if (S->sums[li]) LW_HIP(hipMemsetAsync(S->sums[li], 0, S->sums_count[li] * sizeof(double), S->levels[li]->stream));
    }
    return LUDWIG_OK;
}

int ludwig_modes_accumulate(LudwigModes *S, int32_t level_index, int64_t t_sub, int32_t row)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null mode set");
    if (level_index < 0 || level_index >= S->n_levels)
        return fail(LUDWIG_ERR_INVALID, "modes: level index %d not in 0..%d", level_index, S->n_levels - 1);
    if (t_sub < 0) return fail(LUDWIG_ERR_INVALID, "modes: t_sub %lld < 0", (long long)t_sub);
    if (row < 0 || row >= S->n_rows) return fail(LUDWIG_ERR_INVALID, "modes: row %d not in 0..%d", row, S->n_rows - 1);
    if (row != S->count[level_index])
        return fail(LUDWIG_ERR_STATE, "modes: row %d given, level %d has %lld samples: rows come in order", row, level_index + 1,
                    (long long)S->count[level_index]);
    LW_HIP(hipSetDevice(S->device));
    return modes_launch(S, level_index, t_sub, row);
}

int ludwig_modes_download(LudwigModes *S, int32_t level_index, int32_t column, double *host, size_t bytes, int32_t *n_samples)
{
    if (!S || (!host && bytes > 0)) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (level_index < 0 || level_index >= S->n_levels)
        return fail(LUDWIG_ERR_INVALID, "modes: level index %d not in 0..%d", level_index, S->n_levels - 1);
    if (column < 0 || column >= S->n_columns) return fail(LUDWIG_ERR_INVALID, "modes: column %d not in 0..%d", column, S->n_columns - 1);
    const LudwigLevel *L = S->levels[level_index];
    const size_t want = (size_t)L->sk * sizeof(double) * MODE_FIELDS;
    if (bytes != want) return fail(LUDWIG_ERR_INVALID, "modes: got %zu bytes, expected %zu", bytes, want);
    if (n_samples) *n_samples = (int32_t)S->count[level_index];
    if (want == 0) return LUDWIG_OK;
    if (!S->sums[level_index]) {                          // no owned blocks: every block is a ghost
        memset(host, 0, bytes);
        return LUDWIG_OK;
    }
    return download_components(L, (const double *)S->sums[level_index], S->n_columns * MODE_FIELDS, column * MODE_FIELDS, MODE_FIELDS, host);
}

// ---- slices (ludwig_slices_*; no reference counterpart) ----
// Per level: its points in the order of their base cells (lanes of one wave read neighbouring cells), each with its base cell
// (internal block * 512 + cell), weights, replaced-corner mask and place in the set. One device result [n_rows][n_points], zero
// where no valid point writes.
struct LudwigSlices {
    int device = 0;
    int n_levels = 0, n_points = 0, n_rows = 0;
    bool grad = false;
    std::vector<LudwigLevel *> levels;          // borrowed
    std::vector<float> scales;
    struct PerLevel {
        int n = 0;
        Dev<int32_t> base;                      // [n]
        Dev<float> w;                           // [n][3]
        Dev<uint8_t> rep;                       // [n] bit c: corner c replaced by the base cell
        Dev<int32_t> col;                       // [n] place in the set
    };
    std::vector<PerLevel> per;
    Dev<float> out;
};

void ludwig_slices_destroy(LudwigSlices *S) { destroy_set(S); }

int ludwig_slices_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_points, const int32_t *level_index,
                         const int32_t *blocks, const int32_t *cells, const float *weights, const uint8_t *valid,
                         const float *scales, int32_t flags, LudwigSlices **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!levels || !level_index || !blocks || !cells || !weights || !valid || !scales) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (n_levels < 1 || n_levels > 64) return fail(LUDWIG_ERR_INVALID, "slices: n_levels %d not in 1..64", n_levels);
    if (n_points < 1) return fail(LUDWIG_ERR_INVALID, "slices: n_points %d < 1", n_points);
    if (flags & ~LUDWIG_SLICE_GRADIENT) return fail(LUDWIG_ERR_INVALID, "slices: unknown flags %d", flags);
    const bool grad = (flags & LUDWIG_SLICE_GRADIENT) != 0;
    const int n_rows = grad ? SLICE_ROWS_GRAD : SLICE_ROWS_BASIC;
    if ((int64_t)n_rows * n_points > (int64_t)INT32_MAX) return fail(LUDWIG_ERR_INVALID, "slices: %d points too many", n_points);
    // everything is checked before anything is allocated: every cell a point reads is found here, through the host copy of the
    // neighbour rows the kernel reads, so the kernel never needs a bounds check of its own
    const LudwigLevel *first = nullptr;
    std::vector<std::vector<int32_t>> hb(n_levels), hcol(n_levels);
    std::vector<std::vector<float>> hw(n_levels);
    std::vector<std::vector<uint8_t>> hr(n_levels);
    for (int32_t p = 0; p < n_points; ++p) {
        if (!valid[p]) continue;
        const int r = check_stencil_point("slice point", "slices", p, levels, n_levels, level_index, blocks, cells, weights, first);
        if (r) return r;
        const int li = level_index[p];
        const LudwigLevel *L = levels[li];
        if (!std::isfinite(scales[li]) || scales[li] == 0.0f)
            return fail(LUDWIG_ERR_INVALID, "slices: scale %g of level %d must be finite and non-zero", (double)scales[li], li);
        int32_t e[8];
        for (int c = 0; c < 8; ++c) e[c] = internal_cell(L, blocks[8 * p + c], cells[8 * p + c]);
        const int32_t b0 = e[0] / CELLS;
        if (b0 >= L->n_owned) return fail(LUDWIG_ERR_INVALID, "slice point %d: base block %d is not owned by this level", p, blocks[8 * p]);
        const int x0 = e[0] & 7, y0 = (e[0] >> 3) & 7, z0 = e[0] >> 6 & 7;
        auto locate = [&](int x, int y, int z) -> int64_t {
            const int ox = x >> 3, oy = y >> 3, oz = z >> 3;
            int64_t b = b0;
            if (ox | oy | oz) b = L->h_meta[(size_t)b0 * NBR_STRIDE + DIR(ox, oy, oz)];
            return b < 0 ? -1 : b * CELLS + ((x & 7) + 8 * (y & 7) + 64 * (z & 7));
        };
        uint8_t rep = 0;
        for (int c = 1; c < 8; ++c) {
            const int cx = x0 + (c & 1), cy = y0 + ((c >> 1) & 1), cz = z0 + (c >> 2);
            if (e[c] == e[0]) rep |= (uint8_t)(1u << c);
            else if (locate(cx, cy, cz) != e[c])
                return fail(LUDWIG_ERR_INVALID, "slice point %d corner %d: neither the cell next to the base cell nor the base cell", p, c);
        }
        for (int a = 0; a < 3; ++a) hw[li].push_back(weights[3 * p + a]);
        hb[li].push_back(e[0]);
        hr[li].push_back(rep);
        hcol[li].push_back(p);
    }
    if (!first) return fail(LUDWIG_ERR_INVALID, "slices: no valid point");
    if (const int r = check_one_device("slices", levels, n_levels, first)) return r;
    std::unique_ptr<LudwigSlices> S(new (std::nothrow) LudwigSlices);
    if (!S) return fail(LUDWIG_ERR_ALLOC, "slices: out of host memory");
    S->device = first->device;
    S->n_levels = n_levels;
    S->n_points = n_points;
    S->n_rows = n_rows;
    S->grad = grad;
    S->levels.assign(levels, levels + n_levels);
    S->scales.assign(scales, scales + n_levels);
    S->per.resize(n_levels);
    if (const int r = set_device(S->device)) return r;
    for (int li = 0; li < n_levels; ++li) {
        const size_t n = hcol[li].size();
        LudwigSlices::PerLevel &q = S->per[li];
        q.n = (int)n;
        if (n == 0) continue;
        // launch order: by base cell (stable, so points of one cell keep the set's order)
        std::vector<int32_t> ord(n);
        for (size_t i = 0; i < n; ++i) ord[i] = (int32_t)i;
        std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return hb[li][a] < hb[li][b]; });
        std::vector<int32_t> sb(n), sc(n);
        std::vector<float> sw(3 * n);
        std::vector<uint8_t> sr(n);
        for (size_t i = 0; i < n; ++i) {
            const int32_t j = ord[i];
            sb[i] = hb[li][j];
            sc[i] = hcol[li][j];
            sr[i] = hr[li][j];
            for (int a = 0; a < 3; ++a) sw[3 * i + a] = hw[li][3 * j + a];
        }
        hipError_t e = hipSuccess;
        upload_table(e, sb, q.base);
        upload_table(e, sw, q.w);
        upload_table(e, sr, q.rep);
        upload_table(e, sc, q.col);
        if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "slices: level %d tables: %s", li, hipGetErrorString(e));
    }
    hipError_t e = (hipError_t)S->out.alloc((size_t)n_rows * n_points);
    if (e == hipSuccess) e = hipMemset(S->out, 0, (size_t)n_rows * n_points * sizeof(float));           // invalid points stay 0
    if (e != hipSuccess) return fail(LUDWIG_ERR_ALLOC, "slices: result of %d points: %s", n_points, hipGetErrorString(e));
    *out = S.release();
    return LUDWIG_OK;
}

int ludwig_slices_sample(LudwigSlices *S, int64_t t_coarse)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null slice set");
    if (t_coarse < 0) return fail(LUDWIG_ERR_INVALID, "slices: t_coarse %lld < 0", (long long)t_coarse);
    LW_HIP(hipSetDevice(S->device));
    for (int li = 0; li < S->n_levels; ++li) {
        const LudwigSlices::PerLevel &q = S->per[li];
        if (q.n == 0) continue;
        LudwigLevel *L = S->levels[li];
        LW_ENSURE_RHO(L);
        const float *vel = vel_out(L, (t_coarse + 1) * ((int64_t)1 << li) - 1);    // the level's last sub-step of coarse step t_coarse
        const dim3 grid((unsigned)((q.n + 63) / 64)), block(64);
        if (S->grad)
            hipLaunchKernelGGL(k_slice_sample<true>, grid, block, 0, L->stream, S->out, (int64_t)S->n_points, q.base, q.w, q.rep, q.col,
                               q.n, L->rho, vel, (const int32_t *)L->meta, S->scales[li]);
        else
            hipLaunchKernelGGL(k_slice_sample<false>, grid, block, 0, L->stream, S->out, (int64_t)S->n_points, q.base, q.w, q.rep, q.col,
                               q.n, L->rho, vel, (const int32_t *)L->meta, S->scales[li]);
        LW_HIP(hipGetLastError());
    }
    return LUDWIG_OK;
}

int ludwig_slices_download(LudwigSlices *S, float *values, size_t bytes)
{
    if (!S || !values) return fail(LUDWIG_ERR_INVALID, "null argument");
    const size_t want = (size_t)S->n_rows * S->n_points * sizeof(float);
    if (bytes != want) return fail(LUDWIG_ERR_INVALID, "slices: got %zu bytes, expected %zu", bytes, want);
    LW_HIP(hipSetDevice(S->device));
    for (int li = 0; li < S->n_levels; ++li)
        if (S->per[li].n > 0) LW_HIP(hipStreamSynchronize(S->levels[li]->stream));
    LW_HIP(hipMemcpy(values, S->out, want, hipMemcpyDeviceToHost));
    return LUDWIG_OK;
}

// ---- what the sets that locate points on the hierarchy themselves share (streamlines, tracers, render) ----
// the creators' checks of the level array (`set` = "streamlines", "tracers", "render"; `what` = "a line", "a particle", "a ray")
static int check_locator_levels(const char *set, const char *what, LudwigLevel *const *levels, int32_t n_levels)
{
    for (int li = 0; li < n_levels; ++li) {
        const LudwigLevel *L = levels[li];
        if (!L) return fail(LUDWIG_ERR_INVALID, "%s: level %d is null", set, li);
        if (L->device != levels[0]->device) return fail(LUDWIG_ERR_STATE, "%s: levels on different devices", set);
        if (L->n_owned != L->n_blocks)
            return fail(LUDWIG_ERR_STATE, "%s: level %d holds ghost blocks (%d of %d owned): %s cannot cross ranks", set, li, L->n_owned,
                        L->n_blocks, what);
        if (L->h_block_pointer.size() != (size_t)L->gdx * L->gdy * L->gdz || (L->n_blocks > 0 && L->h_block_pointer.empty()))
            return fail(LUDWIG_ERR_STATE, "%s: level %d was created without block_pointer", set, li);
        if ((int64_t)L->gdx * 8 > (1 << 24) || (int64_t)L->gdy * 8 > (1 << 24) || (int64_t)L->gdz * 8 > (1 << 24))
            return fail(LUDWIG_ERR_INVALID, "%s: level %d has more cells per axis than float32 counts exactly", set, li);
        // the kernel trusts a positive entry as a block index
        for (const int32_t v : L->h_block_pointer)
            if (v < 0 || v > L->n_blocks) return fail(LUDWIG_ERR_STATE, "%s: level %d: block_pointer entry %d out of range", set, li, v);
    }
    return LUDWIG_OK;
}

// every level's block_pointer (bp[li], in the library's block order) and the table of StreamLevel entries on the device; with_rho =
// false leaves the rho pointers null (the tracers never read rho)
static void upload_locator_table(hipError_t &e, LudwigLevel *const *levels, int32_t n_levels, bool with_rho, std::vector<Dev<int32_t>> &bp,
                                 Dev<StreamLevel> &table_dev)
{
    std::vector<StreamLevel> table(n_levels);
    for (int li = 0; li < n_levels && e == hipSuccess; ++li) {
        const LudwigLevel *L = levels[li];
        if (!L->h_block_pointer.empty()) upload_table(e, L->h_block_pointer, bp[li]);
        StreamLevel &t = table[li];
        t.bp = bp[li];
        t.obstacle = L->obstacle;
        t.rho = with_rho ? L->rho.get() : nullptr;
        t.vel[0] = L->vel[0];
        t.vel[1] = L->vel[1];
        t.gx = L->gdx; t.gy = L->gdy; t.gz = L->gdz;
        t.n_blocks = L->n_blocks;
    }
    upload_table(e, table, table_dev);
}

// ---- streamlines (ludwig_streamlines_*; no reference counterpart) ----
// Per level its block_pointer on the device (internal block order, as the level keeps it) inside one table of StreamLevel entries; the
// records [n_lines][max_steps + 1][8], counts and codes. One event orders the trace after the other levels' streams and them after it.
struct LudwigStreamlines {
    int device = 0;
    int n_levels = 0, n_lines = 0, max_steps = 0;
    float step = 0.0f, min_speed = 0.0f;
    std::vector<LudwigLevel *> levels;          // borrowed
    std::vector<Dev<int32_t>> bp;               // per level
    Dev<StreamLevel> table;                     // [n_levels]
    Dev<float> seeds, sign;
    Dev<float> rec;
    Dev<int32_t> counts, codes;
    HipEvent ev;
    bool traced = false;
};

void ludwig_streamlines_destroy(LudwigStreamlines *S) { destroy_set(S); }

int ludwig_streamlines_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_lines, const float *seeds, const float *sign,
                              float step, float min_speed, int32_t max_steps, LudwigStreamlines **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!levels || (n_lines > 0 && (!seeds || !sign))) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (n_levels < 1 || n_levels > 30) return fail(LUDWIG_ERR_INVALID, "streamlines: n_levels %d not in 1..30", n_levels);
    if (n_lines < 0) return fail(LUDWIG_ERR_INVALID, "streamlines: n_lines %d < 0", n_lines);
    if (!(step > 0.0f) || !std::isfinite(step)) return fail(LUDWIG_ERR_INVALID, "streamlines: step %g must be positive and finite", (double)step);
    if (max_steps < 0) return fail(LUDWIG_ERR_INVALID, "streamlines: max_steps %d < 0", max_steps);
    if ((int64_t)n_lines * ((int64_t)max_steps + 1) > (int64_t)INT32_MAX)
        return fail(LUDWIG_ERR_INVALID, "streamlines: %d lines of %d steps are more than 2^31 - 1 records", n_lines, max_steps);
    for (int32_t i = 0; i < n_lines; ++i)
        if (sign[i] != 1.0f && sign[i] != -1.0f) return fail(LUDWIG_ERR_INVALID, "streamlines: sign[%d] = %g is neither 1 nor -1", i, (double)sign[i]);
    if (int rl = check_locator_levels("streamlines", "a line", levels, n_levels)) return rl;
    std::unique_ptr<LudwigStreamlines> S(new (std::nothrow) LudwigStreamlines);
    if (!S) return fail(LUDWIG_ERR_ALLOC, "streamlines: out of host memory");
    S->device = levels[0]->device;
    S->n_levels = n_levels;
    S->n_lines = n_lines;
    S->max_steps = max_steps;
    S->step = step;
    S->min_speed = min_speed;
    S->levels.assign(levels, levels + n_levels);
    S->bp.resize(n_levels);
    if (const int r = set_device(S->device)) return r;
    hipError_t e = hipSuccess;
    upload_locator_table(e, levels, n_levels, true, S->bp, S->table);
    if (n_lines > 0) {
        const size_t n = (size_t)n_lines;
        const std::vector<float> hs(seeds, seeds + 3 * n), hg(sign, sign + n);
        upload_table(e, hs, S->seeds);
        upload_table(e, hg, S->sign);
        if (e == hipSuccess) e = (hipError_t)S->rec.alloc(n * ((size_t)max_steps + 1) * STREAM_REC_FLOATS);
        if (e == hipSuccess) e = (hipError_t)S->counts.alloc(n);
        if (e == hipSuccess) e = (hipError_t)S->codes.alloc(n);
    }
    if (e == hipSuccess) e = (hipError_t)S->ev.create();
    if (e != hipSuccess) return fail(LUDWIG_ERR_ALLOC, "streamlines: %d lines of %d steps: %s", n_lines, max_steps, hipGetErrorString(e));
    *out = S.release();
    return LUDWIG_OK;
}

int ludwig_streamlines_trace(LudwigStreamlines *S, int64_t t_coarse)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null streamline set");
    if (t_coarse < 0) return fail(LUDWIG_ERR_INVALID, "streamlines: t_coarse %lld < 0", (long long)t_coarse);
    S->traced = true;
    if (S->n_lines == 0) return LUDWIG_OK;                        // nothing to trace: nothing launched
    LW_HIP(hipSetDevice(S->device));
    hipStream_t st = S->levels[0]->stream;
    uint32_t temp_mask = 0;
    for (int li = 0; li < S->n_levels; ++li) {
        LudwigLevel *L = S->levels[li];
        LW_ENSURE_RHO(L);
        if (vel_out(L, (t_coarse + 1) * ((int64_t)1 << li) - 1) == L->vel[1]) temp_mask |= 1u << li;
        if (L->stream != st) {                                    // the trace reads what this level's stream has queued
            LW_HIP(hipEventRecord(S->ev, L->stream));
            LW_HIP(hipStreamWaitEvent(st, S->ev, 0));
        }
    }
    StreamArgs a;
    a.lv = S->table;
    a.n_levels = S->n_levels;
    a.temp_mask = temp_mask;
    a.seeds = S->seeds;
    a.sign = S->sign;
    a.n_lines = S->n_lines;
    a.max_steps = S->max_steps;
    a.step = S->step;
    a.min_speed = S->min_speed;
    a.rec = S->rec;
    a.counts = S->counts;
    a.codes = S->codes;
    hipLaunchKernelGGL(k_streamlines, dim3((unsigned)(((int64_t)S->n_lines * 8 + 63) / 64)), dim3(64), 0, st, a);
    LW_HIP(hipGetLastError());
    bool others = false;
    for (int li = 1; li < S->n_levels; ++li) others = others || S->levels[li]->stream != st;
    if (others) {                                                 // and nothing queued there later overtakes the trace's reads
        LW_HIP(hipEventRecord(S->ev, st));
        for (int li = 1; li < S->n_levels; ++li)
            if (S->levels[li]->stream != st) LW_HIP(hipStreamWaitEvent(S->levels[li]->stream, S->ev, 0));
    }
    return LUDWIG_OK;
}

int ludwig_streamlines_download(LudwigStreamlines *S, int32_t *counts, int32_t *codes, float *vertices, size_t bytes)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null streamline set");
    if (!S->traced) return fail(LUDWIG_ERR_STATE, "streamlines: download before ludwig_streamlines_trace");
    const size_t n = (size_t)S->n_lines, row = ((size_t)S->max_steps + 1) * STREAM_REC_FLOATS * sizeof(float);
    if (bytes != n * row) return fail(LUDWIG_ERR_INVALID, "streamlines: got %zu bytes, expected %zu", bytes, n * row);
    if (n == 0) return LUDWIG_OK;
    if (!counts || !codes || !vertices) return fail(LUDWIG_ERR_INVALID, "null argument");
    LW_HIP(hipSetDevice(S->device));
    LW_HIP(hipStreamSynchronize(S->levels[0]->stream));
    LW_HIP(hipMemcpy(counts, S->counts, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    LW_HIP(hipMemcpy(codes, S->codes, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    int32_t longest = 0;
    for (size_t i = 0; i < n; ++i) longest = std::max(longest, counts[i]);
    if (longest > 0)                                              // the used head of every line's row
        LW_HIP(hipMemcpy2D(vertices, row, S->rec, row, (size_t)longest * STREAM_REC_FLOATS * sizeof(float), n, hipMemcpyDeviceToHost));
    return LUDWIG_OK;
}

// ---- volume images (ludwig_render_*; no reference counterpart) ----
// The streamlines' level table plus what an image needs: per level the scalar's address (uploaded with every image, it depends on the
// field and on t_coarse) and, for the scalars that are stored nowhere (|u|, |omega|), a buffer of the set, allocated by the first image
// that asks for it; the colour table; the pixel buffers [max_pixels]. The host copies of the two uploaded tables belong to the set, so
// an upload's source outlives the call that queued it.
struct LudwigRender {
    int device = 0;
    int n_levels = 0;
    int64_t max_pixels = 0;
    int32_t width = 0, height = 0;              // of the last image; 0: none yet
    std::vector<LudwigLevel *> levels;          // borrowed
    std::vector<Dev<int32_t>> bp;               // per level
    Dev<StreamLevel> table;                     // [n_levels]
    std::vector<Dev<float>> scalar;             // per level [n_blocks][512], null until |u| or |omega| is first asked for
    Dev<RenderScalar> sc;                       // [n_levels]
    Dev<float4> colours;                        // [256]
    Dev<float4> rgba;
    Dev<int32_t> codes, samples;
    std::vector<RenderScalar> h_sc;
    std::vector<float4> h_colours;
    HipEvent ev;
    HipEvent uploaded;                          // behind the last upload of h_sc and h_colours
    bool upload_queued = false;
};

void ludwig_render_destroy(LudwigRender *S) { destroy_set(S); }

int ludwig_render_create(LudwigLevel *const *levels, int32_t n_levels, int64_t max_pixels, LudwigRender **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!levels) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (n_levels < 1 || n_levels > 30) return fail(LUDWIG_ERR_INVALID, "render: n_levels %d not in 1..30", n_levels);
    if (max_pixels < 1 || max_pixels > (int64_t)INT32_MAX)
        return fail(LUDWIG_ERR_INVALID, "render: max_pixels %lld not in 1..2^31 - 1", (long long)max_pixels);
    if (int rl = check_locator_levels("render", "a ray", levels, n_levels)) return rl;
    std::unique_ptr<LudwigRender> S(new (std::nothrow) LudwigRender);
    if (!S) return fail(LUDWIG_ERR_ALLOC, "render: out of host memory");
    S->device = levels[0]->device;
    S->n_levels = n_levels;
    S->max_pixels = max_pixels;
    S->levels.assign(levels, levels + n_levels);
    S->bp.resize(n_levels);
    S->scalar.resize(n_levels);
    S->h_sc.resize(n_levels);
    S->h_colours.resize(256);
    if (const int r = set_device(S->device)) return r;
    hipError_t e = hipSuccess;
    upload_locator_table(e, levels, n_levels, true, S->bp, S->table);
    if (e == hipSuccess) e = (hipError_t)S->sc.alloc((size_t)n_levels);
    if (e == hipSuccess) e = (hipError_t)S->colours.alloc(256);
    if (e == hipSuccess) e = (hipError_t)S->rgba.alloc((size_t)max_pixels);
    if (e == hipSuccess) e = (hipError_t)S->codes.alloc((size_t)max_pixels);
    if (e == hipSuccess) e = (hipError_t)S->samples.alloc((size_t)max_pixels);
    if (e == hipSuccess) e = (hipError_t)S->ev.create();
    if (e == hipSuccess) e = (hipError_t)S->uploaded.create();
    if (e != hipSuccess) return fail(LUDWIG_ERR_ALLOC, "render: %lld pixels: %s", (long long)max_pixels, hipGetErrorString(e));
    *out = S.release();
    return LUDWIG_OK;
}

int ludwig_render_image(LudwigRender *S, int64_t t_coarse, int which, const float *scales, const float *camera, int perspective,
                        int32_t width, int32_t height, const float *params, int32_t max_samples, const float *table)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null render set");
    if (!scales || !camera || !params || !table) return fail(LUDWIG_ERR_INVALID, "render: null argument");
    if (t_coarse < 0) return fail(LUDWIG_ERR_INVALID, "render: t_coarse %lld < 0", (long long)t_coarse);
    if (which < LUDWIG_ISO_DENSITY || which > LUDWIG_ISO_VORTICITY_MAGNITUDE) return fail(LUDWIG_ERR_INVALID, "render: unknown scalar %d", which);
    if (perspective != 0 && perspective != 1) return fail(LUDWIG_ERR_INVALID, "render: perspective %d is neither 0 nor 1", perspective);
    if (width < 1 || height < 1 || (int64_t)width * height > S->max_pixels)
        return fail(LUDWIG_ERR_INVALID, "render: %d x %d pixels, the set holds 1..%lld", width, height, (long long)S->max_pixels);
    const float step = params[0], lo = params[1], hi = params[2], t_min = params[3];
    if (!(step > 0.0f) || !std::isfinite(step)) return fail(LUDWIG_ERR_INVALID, "render: step %g must be positive and finite", (double)step);
    if (!(t_min > 0.0f) || !std::isfinite(t_min)) return fail(LUDWIG_ERR_INVALID, "render: t_min %g must be positive and finite", (double)t_min);
    if (!(hi > lo)) return fail(LUDWIG_ERR_INVALID, "render: range [%g, %g] is empty", (double)lo, (double)hi);
    if (max_samples < 1) return fail(LUDWIG_ERR_INVALID, "render: max_samples %d < 1", max_samples);
    for (int li = 0; li < S->n_levels; ++li)
        if (!(scales[li] > 0.0f) || !std::isfinite(scales[li]))
            return fail(LUDWIG_ERR_INVALID, "render: scales[%d] = %g must be positive and finite", li, (double)scales[li]);
    LW_HIP(hipSetDevice(S->device));
    hipStream_t st = S->levels[0]->stream;
    if (S->upload_queued) LW_HIP(hipEventSynchronize(S->uploaded));   // the host tables are free to be rewritten
    const bool gradient = which == LUDWIG_ISO_Q_CRITERION || which == LUDWIG_ISO_VORTICITY_MAGNITUDE;
    for (int li = 0; li < S->n_levels; ++li) {
        LudwigLevel *L = S->levels[li];
        LW_ENSURE_RHO(L);
        const int vf = vel_out(L, (t_coarse + 1) * ((int64_t)1 << li) - 1) == L->vel[1] ? LUDWIG_VEL_TEMP : LUDWIG_VEL;
        RenderScalar &q = S->h_sc[li];
        q.s = nullptr;
        q.stride = CELLS;
        if (L->n_blocks > 0) {                                    // a level without blocks is found by no ray
            if (gradient) {
                const int r = ludwig_level_gradient_fields_compute(L, vf, scales[li]);
                if (r) return r;
            }
            if (which == LUDWIG_ISO_DENSITY) q.s = L->rho;
            else if (which == LUDWIG_ISO_Q_CRITERION) { q.s = L->grad + 3 * CELLS; q.stride = GRAD_COMPONENTS * CELLS; }
            else {
                if (!S->scalar[li]) {
                    const hipError_t ea = (hipError_t)S->scalar[li].alloc((size_t)L->n_blocks * CELLS);
                    if (ea != hipSuccess) return fail(LUDWIG_ERR_ALLOC, "render: scalar of level %d: %s", li, hipGetErrorString(ea));
                }
                if (which == LUDWIG_ISO_VELOCITY_MAGNITUDE)
                    hipLaunchKernelGGL(k_iso_scalar<ISO_VELOCITY_MAGNITUDE>, dim3((unsigned)L->n_blocks), dim3(CELLS / 2), 0, L->stream,
                                       S->scalar[li], (const float *)L->vel[vf == LUDWIG_VEL ? 0 : 1]);
                else
                    hipLaunchKernelGGL(k_iso_scalar<ISO_VORTICITY_MAGNITUDE>, dim3((unsigned)L->n_blocks), dim3(CELLS / 2), 0, L->stream,
                                       S->scalar[li], (const float *)L->grad);
                LW_HIP(hipGetLastError());
                q.s = S->scalar[li];
            }
        }
        if (L->stream != st) {                                    // the image reads what this level's stream has queued
            LW_HIP(hipEventRecord(S->ev, L->stream));
            LW_HIP(hipStreamWaitEvent(st, S->ev, 0));
        }
    }
    for (int i = 0; i < 256; ++i) S->h_colours[i] = make_float4(table[4 * i], table[4 * i + 1], table[4 * i + 2], table[4 * i + 3]);
    LW_HIP(hipMemcpyAsync(S->sc, S->h_sc.data(), (size_t)S->n_levels * sizeof(RenderScalar), hipMemcpyHostToDevice, st));
    LW_HIP(hipMemcpyAsync(S->colours, S->h_colours.data(), 256 * sizeof(float4), hipMemcpyHostToDevice, st));
    LW_HIP(hipEventRecord(S->uploaded, st));
    S->upload_queued = true;
    RenderArgs a;
    a.lv = S->table;
    a.sc = S->sc;
    a.n_levels = S->n_levels;
    a.width = width;
    a.height = height;
    a.perspective = perspective;
    for (int k = 0; k < 3; ++k) {
        a.eye[k] = camera[k];
        a.corner[k] = camera[3 + k];
        a.du[k] = camera[6 + k];
        a.dv[k] = camera[9 + k];
        a.dir[k] = camera[12 + k];
        a.bg[k] = params[4 + k];
        a.body[k] = params[7 + k];
    }
    a.hi[0] = (float)(8 * S->levels[0]->gdx) + 0.5f;
    a.hi[1] = (float)(8 * S->levels[0]->gdy) + 0.5f;
    a.hi[2] = (float)(8 * S->levels[0]->gdz) + 0.5f;
    a.step = step;
    a.lo = lo;
    a.inv = 1.0f / (hi - lo);
    a.t_min = t_min;
    a.max_samples = max_samples;
    a.table = S->colours;
    a.rgba = S->rgba;
    a.codes = S->codes;
    a.samples = S->samples;
    const int64_t tiles = (int64_t)((width + 7) / 8) * ((height + 7) / 8);
    hipLaunchKernelGGL(k_render, dim3((unsigned)tiles), dim3(64), 0, st, a);
    LW_HIP(hipGetLastError());
    S->width = width;
    S->height = height;
    bool others = false;
    for (int li = 1; li < S->n_levels; ++li) others = others || S->levels[li]->stream != st;
    if (others) {                                                 // and nothing queued there later overtakes the image's reads
        LW_HIP(hipEventRecord(S->ev, st));
        for (int li = 1; li < S->n_levels; ++li)
            if (S->levels[li]->stream != st) LW_HIP(hipStreamWaitEvent(S->levels[li]->stream, S->ev, 0));
    }
    return LUDWIG_OK;
}

int ludwig_render_download(LudwigRender *S, float *rgba, int32_t *codes, int32_t *samples, size_t bytes)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null render set");
    if (S->width == 0) return fail(LUDWIG_ERR_STATE, "render: download before ludwig_render_image");
    const size_t n = (size_t)S->width * S->height;
    if (bytes != n * sizeof(float4)) return fail(LUDWIG_ERR_INVALID, "render: got %zu bytes, expected %zu", bytes, n * sizeof(float4));
    if (!rgba || !codes || !samples) return fail(LUDWIG_ERR_INVALID, "null argument");
    LW_HIP(hipSetDevice(S->device));
    LW_HIP(hipStreamSynchronize(S->levels[0]->stream));
    LW_HIP(hipMemcpy(rgba, S->rgba, n * sizeof(float4), hipMemcpyDeviceToHost));
    LW_HIP(hipMemcpy(codes, S->codes, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    LW_HIP(hipMemcpy(samples, S->samples, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return LUDWIG_OK;
}

// ---- tracers (ludwig_tracers_*; no reference counterpart) ----
// The streamlines' level table (every level's block_pointer on the device) plus what persists: positions and states of n_seeds x
// generations slots, the snapshot records, and on the host the count of advances, which alone decides the released generation.
struct LudwigTracers {
    int device = 0;
    int n_levels = 0, n_seeds = 0, generations = 0, release_every = 0;
    int64_t n_slots = 0, n_advances = 0;
    float dt = 0.0f;
    std::vector<LudwigLevel *> levels;          // borrowed
    std::vector<Dev<int32_t>> bp;               // per level
    Dev<StreamLevel> table;                     // [n_levels]
    Dev<float> seeds, pos, rec;
    Dev<int32_t> state;
    HipEvent ev;
    bool snapshot = false;
};

void ludwig_tracers_destroy(LudwigTracers *S) { destroy_set(S); }

int ludwig_tracers_create(LudwigLevel *const *levels, int32_t n_levels, int32_t n_seeds, const float *seeds, int32_t generations,
                          int32_t release_every, float dt, LudwigTracers **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!levels || (n_seeds > 0 && !seeds)) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (n_levels < 1 || n_levels > 30) return fail(LUDWIG_ERR_INVALID, "tracers: n_levels %d not in 1..30", n_levels);
    if (n_seeds < 0) return fail(LUDWIG_ERR_INVALID, "tracers: n_seeds %d < 0", n_seeds);
    if (generations < 1) return fail(LUDWIG_ERR_INVALID, "tracers: generations %d < 1", generations);
    if (release_every < 1) return fail(LUDWIG_ERR_INVALID, "tracers: release_every %d < 1", release_every);
    if (!(dt > 0.0f) || !std::isfinite(dt)) return fail(LUDWIG_ERR_INVALID, "tracers: dt %g must be positive and finite", (double)dt);
    // eight lanes per slot, lane numbers and record offsets in 32 bits with room to spare
    if ((int64_t)n_seeds * (int64_t)generations > (int64_t)INT32_MAX / 8)
        return fail(LUDWIG_ERR_INVALID, "tracers: %d seeds of %d generations are more than 2^28 - 1 slots", n_seeds, generations);
    if (int rl = check_locator_levels("tracers", "a particle", levels, n_levels)) return rl;
    std::unique_ptr<LudwigTracers> S(new (std::nothrow) LudwigTracers);
    if (!S) return fail(LUDWIG_ERR_ALLOC, "tracers: out of host memory");
    S->device = levels[0]->device;
    S->n_levels = n_levels;
    S->n_seeds = n_seeds;
    S->generations = generations;
    S->release_every = release_every;
    S->n_slots = (int64_t)n_seeds * generations;
    S->dt = dt;
    S->levels.assign(levels, levels + n_levels);
    S->bp.resize(n_levels);
    if (const int r = set_device(S->device)) return r;
    hipError_t e = hipSuccess;
    upload_locator_table(e, levels, n_levels, false, S->bp, S->table);      // a tracer carries no rho
    if (S->n_slots > 0) {
        const size_t n = (size_t)S->n_slots;
        const std::vector<float> hs(seeds, seeds + 3 * (size_t)n_seeds);
        const std::vector<int32_t> empty(n, TRACER_EMPTY);
        const std::vector<float> zero(3 * n, 0.0f);
        upload_table(e, hs, S->seeds);
        upload_table(e, zero, S->pos);
        upload_table(e, empty, S->state);
        if (e == hipSuccess) e = (hipError_t)S->rec.alloc(n * STREAM_REC_FLOATS);
    }
    if (e == hipSuccess) e = (hipError_t)S->ev.create();
    if (e != hipSuccess) return fail(LUDWIG_ERR_ALLOC, "tracers: %d seeds of %d generations: %s", n_seeds, generations, hipGetErrorString(e));
    *out = S.release();
    return LUDWIG_OK;
}

// the kernel's arguments for the levels' newest velocity after coarse step t_coarse (the buffer ludwig_streamlines_trace chooses)
static TracerArgs tracers_args(const LudwigTracers *S, int64_t t_coarse)
{
    TracerArgs a{};
    a.s.lv = S->table;
    a.s.n_levels = S->n_levels;
    for (int li = 0; li < S->n_levels; ++li)
        if (vel_out(S->levels[li], (t_coarse + 1) * ((int64_t)1 << li) - 1) == S->levels[li]->vel[1]) a.s.temp_mask |= 1u << li;
    a.seeds = S->seeds;
    a.pos = S->pos;
    a.state = S->state;
    a.rec = S->rec;
    a.n_seeds = S->n_seeds;
    a.n_slots = (int32_t)S->n_slots;
    a.released = -1;
    a.dt = S->dt;
    return a;
}

// advance k = n_advances on stream st; the caller has ordered st behind the levels' steps. A set without slots launches nothing.
static int tracers_launch_advance(LudwigTracers *S, int64_t t_coarse, hipStream_t st)
{
    const int64_t k = S->n_advances++;
    if (S->n_slots == 0) return LUDWIG_OK;
    for (int li = 0; li < S->n_levels; ++li) LW_ENSURE_POPULATIONS(S->levels[li]);
    TracerArgs a = tracers_args(S, t_coarse);
    if (k % S->release_every == 0) a.released = (int32_t)((k / S->release_every) % S->generations);
    hipLaunchKernelGGL(k_tracers_advance, dim3((unsigned)((S->n_slots * 8 + 63) / 64)), dim3(64), 0, st, a);
    LW_HIP(hipGetLastError());
    return LUDWIG_OK;
}

// the first level's stream waits for what the other levels' streams have queued (outside a batch they are usually the same stream)
static int tracers_join(LudwigTracers *S, hipStream_t st)
{
    for (int li = 0; li < S->n_levels; ++li)
        if (S->levels[li]->stream != st) {
            LW_HIP(hipEventRecord(S->ev, S->levels[li]->stream));
            LW_HIP(hipStreamWaitEvent(st, S->ev, 0));
        }
    return LUDWIG_OK;
}

// and nothing queued there later overtakes the kernel's reads
static int tracers_release(LudwigTracers *S, hipStream_t st)
{
    bool others = false;
    for (int li = 1; li < S->n_levels; ++li) others = others || S->levels[li]->stream != st;
    if (!others) return LUDWIG_OK;
    LW_HIP(hipEventRecord(S->ev, st));
    for (int li = 1; li < S->n_levels; ++li)
        if (S->levels[li]->stream != st) LW_HIP(hipStreamWaitEvent(S->levels[li]->stream, S->ev, 0));
    return LUDWIG_OK;
}

int ludwig_tracers_advance(LudwigTracers *S, int64_t t_coarse)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null tracer set");
    if (t_coarse < 0) return fail(LUDWIG_ERR_INVALID, "tracers: t_coarse %lld < 0", (long long)t_coarse);
    if (S->n_slots == 0) { ++S->n_advances; return LUDWIG_OK; }
    LW_HIP(hipSetDevice(S->device));
    hipStream_t st = S->levels[0]->stream;
    int r = tracers_join(S, st);
    if (r) return r;
    if ((r = tracers_launch_advance(S, t_coarse, st))) return r;
    return tracers_release(S, st);
}

int ludwig_tracers_snapshot(LudwigTracers *S, int64_t t_coarse)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null tracer set");
    if (t_coarse < 0) return fail(LUDWIG_ERR_INVALID, "tracers: t_coarse %lld < 0", (long long)t_coarse);
    S->snapshot = true;
    if (S->n_slots == 0) return LUDWIG_OK;
    LW_HIP(hipSetDevice(S->device));
    hipStream_t st = S->levels[0]->stream;
    const int r = tracers_join(S, st);
    if (r) return r;
    for (int li = 0; li < S->n_levels; ++li) LW_ENSURE_POPULATIONS(S->levels[li]);
    const TracerArgs a = tracers_args(S, t_coarse);
    hipLaunchKernelGGL(k_tracers_snapshot, dim3((unsigned)((S->n_slots * 8 + 63) / 64)), dim3(64), 0, st, a);
    LW_HIP(hipGetLastError());
    return tracers_release(S, st);
}

int ludwig_tracers_download(LudwigTracers *S, float *records, size_t bytes, int64_t *n_advances)
{
    if (!S) return fail(LUDWIG_ERR_INVALID, "null tracer set");
    if (!S->snapshot) return fail(LUDWIG_ERR_STATE, "tracers: download before ludwig_tracers_snapshot");
    const size_t want = (size_t)S->n_slots * STREAM_REC_FLOATS * sizeof(float);
    if (bytes != want) return fail(LUDWIG_ERR_INVALID, "tracers: got %zu bytes, expected %zu", bytes, want);
    if (n_advances) *n_advances = S->n_advances;
    if (S->n_slots == 0) return LUDWIG_OK;
    if (!records) return fail(LUDWIG_ERR_INVALID, "null argument");
    LW_HIP(hipSetDevice(S->device));
    LW_HIP(hipStreamSynchronize(S->levels[0]->stream));
    LW_HIP(hipMemcpy(records, S->rec, want, hipMemcpyDeviceToHost));
    return LUDWIG_OK;
}

// ---- warm start (ludwig_flow_source_*, ludwig_level_init_from_source; no reference counterpart) ----
// A flow source is a hierarchy reduced to what stream_sample reads - per level block_pointer, obstacle, rho and ONE velocity array, in
// memory of its own - behind a StreamLevel table whose two vel entries both point at that array (temp_mask 0). It is no LudwigLevel
// and holds no populations: 17 B per cell. Block order: a host-made source keeps the caller's (reference) order, one made from live
// levels keeps theirs (the internal one); block_pointer names the blocks in the same order either way.
struct LudwigFlowSource {
    int device = 0;
    int n_levels = 0;
    std::vector<Dev<int32_t>> bp;
    std::vector<Dev<uint8_t>> obstacle;
    std::vector<Dev<float>> rho, vel;
    Dev<StreamLevel> table;                     // [n_levels]
};

void ludwig_flow_source_destroy(LudwigFlowSource *S) { destroy_set(S); }

static int flow_source_new(int device, int32_t n_levels, std::unique_ptr<LudwigFlowSource> &S)
{
    S.reset(new (std::nothrow) LudwigFlowSource);
    if (!S) return fail(LUDWIG_ERR_ALLOC, "flow source: out of host memory");
    S->device = device;
    S->n_levels = n_levels;
    S->bp.resize(n_levels);
    S->obstacle.resize(n_levels);
    S->rho.resize(n_levels);
    S->vel.resize(n_levels);
    return LUDWIG_OK;
}

// the table entry of level li once its four arrays are allocated
static StreamLevel flow_source_entry(const LudwigFlowSource *S, int li, int gx, int gy, int gz, int n_blocks)
{
    StreamLevel t;
    t.bp = S->bp[li];
    t.obstacle = S->obstacle[li];
    t.rho = S->rho[li];
    t.vel[0] = t.vel[1] = S->vel[li];
    t.gx = gx; t.gy = gy; t.gz = gz;
    t.n_blocks = n_blocks;
    return t;
}

int ludwig_flow_source_create(int device, int32_t n_levels, const int32_t *grid_dims, const int32_t *n_blocks, const int32_t *const *block_pointer,
                              const uint8_t *const *obstacle, const float *const *rho, const float *const *vel, LudwigFlowSource **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!grid_dims || !n_blocks || !block_pointer || !obstacle || !rho || !vel) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (n_levels < 1 || n_levels > WARM_MAX_LEVELS) return fail(LUDWIG_ERR_INVALID, "flow source: n_levels %d not in 1..30", n_levels);
    for (int li = 0; li < n_levels; ++li) {
        const int32_t *gd = grid_dims + 3 * li;
        const int32_t nb = n_blocks[li];
        if (nb < 0 || gd[0] < 0 || gd[1] < 0 || gd[2] < 0) return fail(LUDWIG_ERR_INVALID, "flow source: level %d has a negative size", li);
        if ((int64_t)nb * CELLS * 4 >= (int64_t)1 << 32) return fail(LUDWIG_ERR_INVALID, "flow source: level %d has too many blocks", li);
        for (int a = 0; a < 3; ++a)
            if ((int64_t)gd[a] * 8 > (1 << 24))
                return fail(LUDWIG_ERR_INVALID, "flow source: level %d has more cells per axis than float32 counts exactly", li);
        const size_t nptr = (size_t)gd[0] * gd[1] * gd[2];
        if ((nptr > 0 && !block_pointer[li]) || (nb > 0 && (!obstacle[li] || !rho[li] || !vel[li] || nptr == 0)))
            return fail(LUDWIG_ERR_INVALID, "flow source: level %d: null array", li);
        for (size_t i = 0; i < nptr; ++i)                      // the kernel trusts a positive entry as a block index
            if (block_pointer[li][i] < 0 || block_pointer[li][i] > nb)
                return fail(LUDWIG_ERR_INVALID, "flow source: level %d: block_pointer entry %d out of range", li, block_pointer[li][i]);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LUDWIG_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(LUDWIG_ERR_INVALID, "device %d out of range (have %d)", device, ndev);
    if (const int r = set_device(device)) return r;
    std::unique_ptr<LudwigFlowSource> S;
    if (const int r = flow_source_new(device, n_levels, S)) return r;
    std::vector<StreamLevel> table(n_levels);
    hipError_t e = hipSuccess;
    for (int li = 0; li < n_levels && e == hipSuccess; ++li) {
        const int32_t *gd = grid_dims + 3 * li;
        const size_t nb = (size_t)n_blocks[li], nptr = (size_t)gd[0] * gd[1] * gd[2];
        upload_table(e, std::vector<int32_t>(block_pointer[li], block_pointer[li] + nptr), S->bp[li]);
        if (nb > 0) {
            upload_table(e, std::vector<uint8_t>(obstacle[li], obstacle[li] + nb * CELLS), S->obstacle[li]);
            upload_table(e, std::vector<float>(rho[li], rho[li] + nb * CELLS), S->rho[li]);
            std::vector<float> v(nb * 3 * CELLS);              // [8,8,8,nb,3] -> block-major [nb][3][512]
            for (size_t k = 0; k < 3; ++k)
                for (size_t b = 0; b < nb; ++b) memcpy(&v[(b * 3 + k) * CELLS], &vel[li][(k * nb + b) * CELLS], CELLS * sizeof(float));
            upload_table(e, v, S->vel[li]);
        }
        table[li] = flow_source_entry(S.get(), li, gd[0], gd[1], gd[2], (int)nb);
    }
    upload_table(e, table, S->table);
    if (e != hipSuccess) return fail(LUDWIG_ERR_ALLOC, "flow source: %s", hipGetErrorString(e));
    *out = S.release();
    return LUDWIG_OK;
}

int ludwig_flow_source_from_levels(LudwigLevel *const *levels, int32_t n_levels, int64_t t_coarse, LudwigFlowSource **out)
{
    if (!out) return fail(LUDWIG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!levels) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (n_levels < 1 || n_levels > WARM_MAX_LEVELS) return fail(LUDWIG_ERR_INVALID, "flow source: n_levels %d not in 1..30", n_levels);
    if (t_coarse < 0) return fail(LUDWIG_ERR_INVALID, "flow source: t_coarse %lld < 0", (long long)t_coarse);
    if (int rl = check_locator_levels("flow source", "a sample", levels, n_levels)) return rl;
    const int device = levels[0]->device;
    if (const int r = set_device(device)) return r;
    std::unique_ptr<LudwigFlowSource> S;
    if (const int r = flow_source_new(device, n_levels, S)) return r;
    std::vector<StreamLevel> table(n_levels);
    hipError_t e = hipSuccess;
    for (int li = 0; li < n_levels; ++li) {
        LudwigLevel *L = levels[li];
        LW_ENSURE_RHO(L);                                      // rho as a download would return it, and f / vel out of any record
        const size_t c = (size_t)L->sk;
        upload_table(e, L->h_block_pointer, S->bp[li]);
        if (e == hipSuccess) e = (hipError_t)S->obstacle[li].alloc(c);
        if (e == hipSuccess) e = (hipError_t)S->rho[li].alloc(c);
        if (e == hipSuccess) e = (hipError_t)S->vel[li].alloc(c * 3);
        if (e != hipSuccess) break;
        if (c > 0) {                                           // ordered behind the steps queued on the level's stream
            const float *v = vel_out(L, (t_coarse + 1) * ((int64_t)1 << li) - 1);
            LW_HIP(hipMemcpyAsync(S->obstacle[li], L->obstacle, c, hipMemcpyDeviceToDevice, L->stream));
            LW_HIP(hipMemcpyAsync(S->rho[li], L->rho, c * 4, hipMemcpyDeviceToDevice, L->stream));
            LW_HIP(hipMemcpyAsync(S->vel[li], v, c * 3 * 4, hipMemcpyDeviceToDevice, L->stream));
        }
        table[li] = flow_source_entry(S.get(), li, L->gdx, L->gdy, L->gdz, L->n_blocks);
    }
    upload_table(e, table, S->table);
    if (e != hipSuccess) return fail(LUDWIG_ERR_ALLOC, "flow source: %s", hipGetErrorString(e));
    for (int li = 0; li < n_levels; ++li) LW_HIP(hipStreamSynchronize(levels[li]->stream));     // whoever reads the source finds it complete
    *out = S.release();
    return LUDWIG_OK;
}

int ludwig_level_init_from_source(LudwigLevel *L, const LudwigFlowSource *S, const float *map, float vel_scale, const float *fallback,
                                  int64_t *counts)
{
    if (!L || !S || !map || !fallback) return fail(LUDWIG_ERR_INVALID, "null argument");
    for (int a = 0; a < 6; ++a)
        if (!std::isfinite(map[a])) return fail(LUDWIG_ERR_INVALID, "init from source: map[%d] = %g is not finite", a, (double)map[a]);
    for (int a = 0; a < 3; ++a)
        if (!(map[a] > 0.0f)) return fail(LUDWIG_ERR_INVALID, "init from source: map[%d] = %g must be positive", a, (double)map[a]);
    if (!std::isfinite(vel_scale) || !(vel_scale > 0.0f))
        return fail(LUDWIG_ERR_INVALID, "init from source: vel_scale %g must be positive and finite", (double)vel_scale);
    for (int a = 0; a < 4; ++a)
        if (!std::isfinite(fallback[a])) return fail(LUDWIG_ERR_INVALID, "init from source: fallback[%d] = %g is not finite", a, (double)fallback[a]);
    if (S->device != L->device) return fail(LUDWIG_ERR_STATE, "init from source: the source is on device %d, the level on %d", S->device, L->device);
    // (float)gc + 0.5f must be exact
    for (int b = 0; b < L->n_blocks; ++b)
        for (int a = 0; a < 3; ++a) {
            const int32_t m = L->h_meta[(size_t)b * NBR_STRIDE + NBR_BX + a];
            if (m < 1 || (int64_t)m * 8 > (1 << 23))
                return fail(LUDWIG_ERR_INVALID, "init from source: block coordinate %d: more than 2^23 cells per axis (or < 1)", m);
        }
    const int n_counts = WARM_OUTCOMES + S->n_levels;
    if (counts) std::fill(counts, counts + n_counts, (int64_t)0);
    if (L->n_owned == 0 || L->n_blocks == 0) return LUDWIG_OK;   // a level that only holds ghost copies: accepted, nothing to do
    LW_HIP(hipSetDevice(L->device));
    // The level ends up as if f, f_temp, vel, vel_temp, rho (and the saved state) had been uploaded: the same helper, field by field -
    // whatever only a record, an elided rho store or an aliased saved state holds is settled before the arrays are overwritten.
    ++L->version;
    static const int written[] = {LUDWIG_F, LUDWIG_F_TEMP, LUDWIG_VEL, LUDWIG_VEL_TEMP, LUDWIG_RHO, LUDWIG_F_OLD, LUDWIG_VEL_OLD, LUDWIG_RHO_OLD};
    for (int i = 0; i < (L->has_temporal ? 8 : 5); ++i)
        if (const int r = before_external_write(L, written[i])) return r;
    L->rho_old_pending = false;                                // rho_old is written here: no save is owed any more
    Dev<unsigned long long> d_counts;
    if (counts) {
        LW_HIP((hipError_t)d_counts.alloc((size_t)n_counts));
        LW_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_counts * sizeof(unsigned long long), L->stream));
    }
    WarmArgs a{};
    a.s.lv = S->table;
    a.s.n_levels = S->n_levels;
    a.s.temp_mask = 0u;
    a.meta = L->meta;
    a.obstacle = L->obstacle;
    a.f[0] = L->f[0]; a.f[1] = L->f[1]; a.f[2] = L->has_temporal ? L->f_old.get() : nullptr;
    a.vel[0] = L->vel[0]; a.vel[1] = L->vel[1]; a.vel[2] = L->has_temporal ? L->vel_old.get() : nullptr;
    a.rho[0] = L->rho; a.rho[1] = L->has_temporal ? L->rho_old.get() : nullptr;
    for (int i = 0; i < 6; ++i) a.map[i] = map[i];
    a.scale = vel_scale;
    for (int i = 0; i < 4; ++i) a.fallback[i] = fallback[i];
    a.counts = counts ? d_counts.get() : nullptr;
    hipLaunchKernelGGL(k_init_from_source, dim3((unsigned)L->n_blocks), dim3(256), 0, L->stream, a);
    LW_HIP(hipGetLastError());
    if (counts) {
        std::vector<unsigned long long> h((size_t)n_counts);
        LW_HIP(hipMemcpyAsync(h.data(), d_counts, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, L->stream));
        LW_HIP(hipStreamSynchronize(L->stream));
        for (int i = 0; i < n_counts; ++i) counts[i] = (int64_t)h[i];
    }
    return LUDWIG_OK;
}

// ---- the batch (ludwig_execute_timestep_batch*): what it refuses, how it runs, its entry points ----
static int check_batch_levels(LudwigLevel *const *levels, int32_t n_levels, int32_t batch_size, const LudwigStepFlags *flags)
{
    if (!levels || !flags || n_levels < 1 || batch_size < 0) return fail(LUDWIG_ERR_INVALID, "bad argument");
    for (int i = 0; i < n_levels; ++i) {
        if (!levels[i]) return fail(LUDWIG_ERR_INVALID, "null level %d", i + 1);
        if (levels[i]->device != levels[0]->device || levels[i]->stream != levels[0]->stream)
            return fail(LUDWIG_ERR_INVALID, "all levels must share one device and one stream");
    }
    return LUDWIG_OK;
}

// the set was made over exactly these levels (probes, tracers)
static int check_made_over(const char *what, const std::vector<LudwigLevel *> &made_over, LudwigLevel *const *levels, int32_t n_levels)
{
    if ((int)made_over.size() != n_levels)
        return fail(LUDWIG_ERR_INVALID, "%s: set made over %d levels, batch of %d", what, (int)made_over.size(), n_levels);
    for (int i = 0; i < n_levels; ++i)
        if (made_over[i] != levels[i]) return fail(LUDWIG_ERR_INVALID, "%s: set made over other levels (level %d)", what, i + 1);
    return LUDWIG_OK;
}

// the set's level is one of the batch's (surface, forces)
static int check_level_in_batch(const char *what, const LudwigLevel *level, LudwigLevel *const *levels, int32_t n_levels)
{
    bool in_batch = false;
    for (int i = 0; i < n_levels; ++i) in_batch = in_batch || levels[i] == level;
    return in_batch ? LUDWIG_OK : fail(LUDWIG_ERR_INVALID, "%s: the set's level is not in the batch", what);
}

// nothing is stepped when what this batch adds to a ring would not fit (probes, forces)
static int check_ring_room(const char *what, const char *items, size_t used, int capacity, const ObserverSchedule &o, int64_t t_start,
                           int32_t batch_size)
{
    const int64_t k = batch_size > 0 ? samples_in(t_start, t_start + batch_size - 1, o.start_step, o.interval) : 0;
    if ((int64_t)used + k <= capacity) return LUDWIG_OK;
    return fail(LUDWIG_ERR_STATE, "%s: %lld %s of this batch overflow the ring (%d of %d used): download first", what, (long long)k, items,
                (int)used, capacity);
}

// Every refusal of a batch beyond its levels', before anything is stepped: the list itself, then each set in the fixed order probes,
// surface, tracers, forces, fluxes, modes. Fills `obs` from the entries with a set.
static int check_batch_observers(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size,
                                 const LudwigBatchObserver *observers, int32_t n_observers, BatchObservers *obs)
{
    if (n_observers < 0) return fail(LUDWIG_ERR_INVALID, "batch: %d observer entries", n_observers);
    if (n_observers > 0 && !observers) return fail(LUDWIG_ERR_INVALID, "batch: null observer list of %d entries", n_observers);
    const LudwigBatchObserver *of_kind[LUDWIG_OBSERVE_MODES + 1] = {};
    for (int i = 0; i < n_observers; ++i) {
        const LudwigBatchObserver &e = observers[i];
        if (!e.set) continue;
        if (e.kind < 0 || e.kind > LUDWIG_OBSERVE_MODES) return fail(LUDWIG_ERR_INVALID, "batch: observer entry %d of unknown kind %d", i, e.kind);
        if (of_kind[e.kind]) return fail(LUDWIG_ERR_INVALID, "batch: observer entry %d is the second of kind %d", i, e.kind);
        of_kind[e.kind] = &e;
    }
    int r;
    if (const LudwigBatchObserver *e = of_kind[LUDWIG_OBSERVE_PROBES]) {
        LudwigProbes *P = static_cast<LudwigProbes *>(e->set);
        obs->probes = {{e->start_step, e->interval}, P};
        if (e->interval < 1) return fail(LUDWIG_ERR_INVALID, "probes: interval %d < 1", e->interval);
        if ((r = check_made_over("probes", P->levels, levels, n_levels))) return r;
        if ((r = check_ring_room("probes", "samples", P->slot_step.size(), P->capacity, obs->probes, t_start, batch_size))) return r;
    }
    if (const LudwigBatchObserver *e = of_kind[LUDWIG_OBSERVE_SURFACE]) {
        LudwigSurfaceStats *S = static_cast<LudwigSurfaceStats *>(e->set);
        obs->surface = {{e->start_step, e->interval}, S};
        if (e->interval < 1) return fail(LUDWIG_ERR_INVALID, "surface statistics: interval %d < 1", e->interval);
        if ((r = check_level_in_batch("surface statistics", S->level, levels, n_levels))) return r;
    }
    if (const LudwigBatchObserver *e = of_kind[LUDWIG_OBSERVE_TRACERS]) {
        LudwigTracers *T = static_cast<LudwigTracers *>(e->set);
        obs->tracers = {{e->start_step, e->interval}, T};
        if (e->interval < 1) return fail(LUDWIG_ERR_INVALID, "tracers: interval %d < 1", e->interval);
        if ((r = check_made_over("tracers", T->levels, levels, n_levels))) return r;
    }
    if (const LudwigBatchObserver *e = of_kind[LUDWIG_OBSERVE_FORCES]) {
        LudwigForceSeries *F = static_cast<LudwigForceSeries *>(e->set);
        obs->forces = {{e->start_step, e->interval}, F};
        if (e->interval < 1) return fail(LUDWIG_ERR_INVALID, "force series: interval %d < 1", e->interval);
        if ((r = check_level_in_batch("force series", F->level, levels, n_levels))) return r;
        if ((r = check_ring_room("force series", "records", F->slot_step.size(), F->capacity, obs->forces, t_start, batch_size))) return r;
    }
    if (const LudwigBatchObserver *e = of_kind[LUDWIG_OBSERVE_FLUXES]) {
        LudwigFluxPlanes *P = static_cast<LudwigFluxPlanes *>(e->set);
        obs->fluxes = {{e->start_step, e->interval}, P};
        if (e->interval < 1) return fail(LUDWIG_ERR_INVALID, "flux planes: interval %d < 1", e->interval);
        if ((r = check_made_over("flux planes", P->levels, levels, n_levels))) return r;
        if ((r = check_ring_room("flux planes", "records", P->slot_step.size(), P->capacity, obs->fluxes, t_start, batch_size))) return r;
    }
    if (const LudwigBatchObserver *e = of_kind[LUDWIG_OBSERVE_MODES]) {
        LudwigModes *S = static_cast<LudwigModes *>(e->set);
        obs->modes = {{e->start_step, e->interval}, S};
        if (e->interval < 1) return fail(LUDWIG_ERR_INVALID, "modes: interval %d < 1", e->interval);
        if ((r = check_made_over("modes", S->levels, levels, n_levels))) return r;
        // the batch's due steps must give exactly the rows count, count + 1, ... of every level, all of them inside the window
        const int64_t last = t_start + batch_size - 1;
        const int64_t k = batch_size > 0 ? samples_in(t_start, last, e->start_step, e->interval) : 0;
        if (k > 0) {
            const int64_t lo = std::max(t_start, e->start_step);
            const int64_t first_due = e->start_step + (lo - e->start_step + e->interval - 1) / e->interval * e->interval;
            const int64_t row = modes_row_of(first_due, e->start_step, e->interval, S->n_rows);
            for (int i = 0; i < n_levels; ++i) {
                if (S->count[i] != row)
                    return fail(LUDWIG_ERR_STATE, "modes: step %lld is row %lld of the window, level %d has %lld samples", (long long)first_due,
                                (long long)row, i + 1, (long long)S->count[i]);
                if (row + k > S->n_rows)
                    return fail(LUDWIG_ERR_STATE, "modes: %lld samples of this batch from row %lld run past the window of %d rows: cut the "
                                "batch at the window's last step", (long long)k, (long long)row, S->n_rows);
            }
        }
    }
    return LUDWIG_OK;
}

// one advance of a batch's tracer set behind coarse step t: with level streams, a full join around the launch (see batch_impl)
static int batch_tracers_advance(LudwigLevel *const *levels, int32_t n_levels, LudwigTracers *T, int64_t t, bool concurrent)
{
    hipStream_t st = levels[0]->stream;
    if (!concurrent || T->n_slots == 0) return tracers_launch_advance(T, t, st);      // one stream, or nothing to launch: no event
    for (int i = 1; i < n_levels; ++i) {
        LW_HIP(hipEventRecord(T->ev, levels[i]->stream));
        LW_HIP(hipStreamWaitEvent(st, T->ev, 0));
    }
    const int rc = tracers_launch_advance(T, t, st);
    if (rc) return rc;
    LW_HIP(hipEventRecord(T->ev, st));
    for (int i = 1; i < n_levels; ++i) LW_HIP(hipStreamWaitEvent(levels[i]->stream, T->ev, 0));
    return LUDWIG_OK;
}

// Level streams. The reference steps its levels strictly one after the other (src/solver_control.jl:21-143), and every launch
// of a small level leaves most of the 256 CUs idle. The data dependencies are weaker than the call order: coupling is one-way,
// coarse -> fine, and a child reads its parent's buffers only in its interface pass (k_interface_sources / _links, once per
// pair of sub-steps). So each level gets a HIP stream of its own and two events:
//   * a child's sub-step waits for its parent's step (parent->ev_stepped) before it interpolates from it;
//   * a parent's NEXT step - which overwrites the buffer holding its old state, rho and rho_old - waits until the child's
//     interface pass has read them (ev_consumed, recorded on the child's stream right after that pass).
// Launches are still issued in the reference's order; the GPU then runs level 1's step t + 1 under the finer levels' sub-steps
// of step t, and a middle level's second sub-step under its children's first pair. Same kernels, same inputs: same bits.
// The finest level is the critical chain (2^(n-1) sub-steps per coarse step): its stream gets the highest priority, the others the
// lowest, so the coarser levels only fill what it leaves free. Measured on one box, alternating (profiles/
// r02_level_streams_with_priorities_ab_one_box.txt): 3-level sphere 0.419 -> 0.393 ms per coarse step, real wing 1.011 -> 0.949,
// 4-level sphere 1.72 -> 1.52; without the priorities 0.402 / 0.982 / 1.58 (and on another box the 4-level case got slower).
// LUDWIG_BATCH_SERIAL=1 keeps everything on one stream; LUDWIG_LEVEL_STREAM_PRIORITY=0 gives every level the same priority.
// Tracers: after the host has issued every launch of coarse step t and none of t + 1, an advanced step joins all level streams -
// the first level's stream waits for what the others have queued, runs the advance, and the others wait for it before they go on. That
// only adds ordering; at advanced steps it gives up the overlap of level 1's step t + 1 with the finer levels' tail of step t.
static int batch_impl(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size, float u_curr,
                      const LudwigStepFlags *flags, const BatchObservers &obs)
{
    const bool concurrent = n_levels > 1 && !env::batch_serial();
    hipStream_t user_stream = levels[0]->stream;
    if (concurrent) {
        LW_HIP(hipSetDevice(levels[0]->device));
        LW_HIP(hipStreamSynchronize(user_stream));             // everything queued before the batch is done
        // 1. every level gets its stream and its two events - or none does: they are made beside the levels and moved in once all
        //    exist, so that a later batch never finds a level with a stream but no events. The levels keep the caller's stream until then.
        int pr_least = 0, pr_greatest = 0;
        LW_HIP(hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
        const int pr_mode = env::level_stream_priority();
        struct Made { HipStream st; HipEvent stepped, consumed; };
        std::vector<Made> made((size_t)n_levels);
        int e = 0;
        for (int i = 0; i < n_levels && !e; ++i) {
            if (levels[i]->own_stream) continue;                              // complete from an earlier batch: keep
            // the finest level is the critical chain (2^(n-1) sub-steps per coarse step): its stream gets the highest priority, the
            // coarser levels fill what it leaves free (graded priorities: no better)
            // LUDWIG_LEVEL_STREAM_PRIORITY=2: graded - the finest level highest, its parent (whose stream carries the finest level's interface
            // pass since round 3) one below, the rest lowest
            int pr = pr_mode == 0 ? pr_least : (i == n_levels - 1 ? pr_greatest : pr_least);
            if (pr_mode == 2) pr = std::min(pr_least, pr_greatest + (n_levels - 1 - i));
            e = made[i].st.create(hipStreamNonBlocking, pr);
            if (!e) e = made[i].stepped.create();
            if (!e) e = made[i].consumed.create();
        }
        if (e) return fail(LUDWIG_ERR_HIP, "batch: level streams: %s", hipGetErrorString((hipError_t)e));
        for (int i = 0; i < n_levels; ++i) {
            if (!made[i].st) continue;
            levels[i]->own_stream = std::move(made[i].st);
            levels[i]->ev_stepped = std::move(made[i].stepped);
            levels[i]->ev_consumed = std::move(made[i].consumed);
        }
        // 2. switch over; one way back for every early return
        auto restore = [&]() { for (int j = 0; j < n_levels; ++j) levels[j]->stream = user_stream; };
        for (int i = 0; i < n_levels; ++i) {
            LudwigLevel *L = levels[i];
            L->ev_consumed_set = false;
            L->waited_parent = nullptr;
            L->parent_wait = nullptr;
            L->pair_ready.valid = false;
            L->pair_done_set[0] = L->pair_done_set[1] = false;      // the previous batch ended with every stream idle
            L->stream = L->own_stream;
        }
        for (int i = 0; i + 1 < n_levels; ++i) {
            LudwigLevel *L = levels[i];
            if (!L->rho_eager) {                               // children interpolate from rho after every step
                L->rho_eager = true;
                const int r = ensure_rho(L);
                if (r) { restore(); return r; }
            }
        }
    }
    for (int i = 0; i < n_levels; ++i) levels[i]->rho_old_pending = false;      // (only an aborted batch could have left one)
    // in-batch observers read f / vel / rho between the steps, and the levels of a nest read each other: such a batch runs the f path
    const bool hold_records = n_levels > 1 || obs.any();
    for (int i = 0; i < n_levels; ++i) levels[i]->rec_hold = hold_records;
    int rc = LUDWIG_OK;
    for (int32_t o = 0; o < batch_size && rc == LUDWIG_OK; ++o) {
        const int64_t t = t_start + o;
        BatchHook ph;
        ph.obs = &obs;
        ph.t = t;
        if (obs.probes.set && obs.probes.due(t)) ph.slot = probes_open_slot(obs.probes.set, t);
        ph.surface = obs.surface.set && obs.surface.due(t);
        ph.forces = obs.forces.set && obs.forces.due(t);
        if (obs.fluxes.set && obs.fluxes.due(t)) ph.flux_slot = flux_planes_open_slot(obs.fluxes.set, t);
        if (obs.modes.set && obs.modes.due(t)) ph.modes_row = modes_row_of(t, obs.modes.start_step, obs.modes.interval, obs.modes.set->n_rows);
        rc = recursive_step(levels, n_levels, 1, t, nullptr, 0.5f, 0.0f, u_curr, flags, concurrent, &ph);
        if (rc == LUDWIG_OK && obs.tracers.set && obs.tracers.due(t)) rc = batch_tracers_advance(levels, n_levels, obs.tracers.set, t, concurrent);
    }
    if (concurrent) {
        hipError_t e = hipSuccess;
        for (int i = 0; i < n_levels; ++i) {
            const hipError_t ei = hipStreamSynchronize(levels[i]->own_stream);
            if (e == hipSuccess) e = ei;
            levels[i]->stream = user_stream;
        }
        if (rc == LUDWIG_OK && e != hipSuccess) return fail(LUDWIG_ERR_HIP, "batch: %s", hipGetErrorString(e));
    }
    for (int i = 0; i < n_levels; ++i) levels[i]->rec_hold = false;
    if (rc) return rc;
    return ludwig_sync(levels[0]);
}

int ludwig_execute_timestep_batch_observed(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size, float u_curr,
                                           const LudwigStepFlags *flags, const LudwigBatchObserver *observers, int32_t n_observers)
{
    BatchObservers obs;
    int r = check_batch_levels(levels, n_levels, batch_size, flags);
    if (r) return r;
    if ((r = check_batch_observers(levels, n_levels, t_start, batch_size, observers, n_observers, &obs))) return r;
    return batch_impl(levels, n_levels, t_start, batch_size, u_curr, flags, obs);
}

int ludwig_execute_timestep_batch(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size, float u_curr,
                                  const LudwigStepFlags *flags)
{
    return ludwig_execute_timestep_batch_observed(levels, n_levels, t_start, batch_size, u_curr, flags, nullptr, 0);
}

// The four entry points from before the observer list: each fills its entries (a null set: a null entry) and forwards.
int ludwig_execute_timestep_batch_probes(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size, float u_curr,
                                         const LudwigStepFlags *flags, LudwigProbes *probes, int64_t start_step, int32_t interval)
{
    const LudwigBatchObserver o = {LUDWIG_OBSERVE_PROBES, probes, start_step, interval};
    return ludwig_execute_timestep_batch_observed(levels, n_levels, t_start, batch_size, u_curr, flags, &o, 1);
}

// the probes and surface entries of s (null: two null entries)
static void sampler_entries(const LudwigBatchSamplers *s, LudwigBatchObserver *o)
{
    const LudwigBatchSamplers none = {};
    if (!s) s = &none;
    o[0] = {LUDWIG_OBSERVE_PROBES, s->probes, s->probes_start_step, s->probes_interval};
    o[1] = {LUDWIG_OBSERVE_SURFACE, s->surface, s->surface_start_step, s->surface_interval};
}

int ludwig_execute_timestep_batch_sampled(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size, float u_curr,
                                          const LudwigStepFlags *flags, const LudwigBatchSamplers *s)
{
    LudwigBatchObserver o[2];
    sampler_entries(s, o);
    return ludwig_execute_timestep_batch_observed(levels, n_levels, t_start, batch_size, u_curr, flags, o, 2);
}

int ludwig_execute_timestep_batch_loads(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size, float u_curr,
                                        const LudwigStepFlags *flags, const LudwigBatchSamplers *s, LudwigForceSeries *fs, int64_t start_step,
                                        int32_t interval)
{
    LudwigBatchObserver o[3];
    sampler_entries(s, o);
    o[2] = {LUDWIG_OBSERVE_FORCES, fs, start_step, interval};
    return ludwig_execute_timestep_batch_observed(levels, n_levels, t_start, batch_size, u_curr, flags, o, 3);
}

int ludwig_execute_timestep_batch_tracers(LudwigLevel *const *levels, int32_t n_levels, int64_t t_start, int32_t batch_size, float u_curr,
                                          const LudwigStepFlags *flags, const LudwigBatchSamplers *s, LudwigForceSeries *fs,
                                          int64_t force_start_step, int32_t force_interval, LudwigTracers *tracers, int64_t start_step,
                                          int32_t interval)
{
    LudwigBatchObserver o[4];
    sampler_entries(s, o);
    o[2] = {LUDWIG_OBSERVE_FORCES, fs, force_start_step, force_interval};
    o[3] = {LUDWIG_OBSERVE_TRACERS, tracers, start_step, interval};
    return ludwig_execute_timestep_batch_observed(levels, n_levels, t_start, batch_size, u_curr, flags, o, 4);
}

int ludwig_halo_pack(const LudwigLevel *L, int field, const int64_t *index_dev, int64_t n, float *dst_dev, void *hip_stream)
{
    if (!L || (n > 0 && (!index_dev || !dst_dev))) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (n == 0) return LUDWIG_OK;
    const FieldDesc d = field_desc(L, field);
    if (!d.ptr || field == LUDWIG_OBSTACLE) return fail(LUDWIG_ERR_STATE, "field %d cannot be packed", field);
    LW_HIP(hipSetDevice(L->device));
    LW_ENSURE_POPULATIONS(L);
    if (field == LUDWIG_RHO) {
        bool stale = false;
        for (int a = 0; a < N_PARTS; ++a) stale = stale || L->rho_replay[a].stale;
        const int r = ensure_rho(const_cast<LudwigLevel *>(L));
        if (r) return r;
        // the replay ran on the level's stream: a pack queued on another stream must not overtake it
        if (stale && hip_stream && (hipStream_t)hip_stream != L->stream) LW_HIP(hipStreamSynchronize(L->stream));
    }
    hipLaunchKernelGGL(k_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hip_stream ? (hipStream_t)hip_stream : L->stream, (const float *)d.ptr, index_dev, n, dst_dev, (const int32_t *)L->d_ref2int, L->sk, d.comps);
    LW_HIP(hipGetLastError());
    return LUDWIG_OK;
}

int ludwig_halo_unpack(LudwigLevel *L, int field, const int64_t *index_dev, int64_t n, const float *src_dev, void *hip_stream)
{
    if (!L || (n > 0 && (!index_dev || !src_dev))) return fail(LUDWIG_ERR_INVALID, "null argument");
    if (n == 0) return LUDWIG_OK;
    ++L->version;
    {
        const bool aliased = L->old_alias >= 0;
        const int r = before_external_write(L, field);
        if (r) return r;
        if (aliased && L->old_alias < 0 && hip_stream && (hipStream_t)hip_stream != L->stream) LW_HIP(hipStreamSynchronize(L->stream));
    }
    const FieldDesc d = field_desc(L, field);
    if (!d.ptr || field == LUDWIG_OBSTACLE) return fail(LUDWIG_ERR_STATE, "field %d cannot be unpacked", field);
    LW_HIP(hipSetDevice(L->device));
    hipLaunchKernelGGL(k_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hip_stream ? (hipStream_t)hip_stream : L->stream, (float *)d.ptr, index_dev, n, src_dev, (const int32_t *)L->d_ref2int, L->sk, d.comps);
    LW_HIP(hipGetLastError());
    return LUDWIG_OK;
}

int ludwig_record_step_rule(const int32_t *block_flags, int32_t n_blocks, int32_t n_owned, int32_t has_parent, int32_t has_temporal_storage,
                            int32_t has_post_collision, int32_t wall_model_active)
{
    if (n_blocks < 0 || (n_blocks > 0 && !block_flags)) return fail(LUDWIG_ERR_INVALID, "record step rule: bad argument");
    if (n_blocks == 0 || n_owned != n_blocks || has_parent || has_temporal_storage || has_post_collision || wall_model_active) return 0;
    for (int32_t b = 0; b < n_blocks; ++b)
        if (block_flags[b] != FLAG_ALL_NEIGHBOURS) return 0;       // a missing neighbour, or an obstacle / sponge / near-wall / post bit
    return 1;
}

int ludwig_level_record_steps(const LudwigLevel *L, int64_t *n_steps)
{
    if (!L || !n_steps) return fail(LUDWIG_ERR_INVALID, "null argument");
    *n_steps = L->n_record_steps;
    return LUDWIG_OK;
}

int ludwig_level_info(const LudwigLevel *L, LudwigLevelInfo *info)
{
    if (!L || !info) return fail(LUDWIG_ERR_INVALID, "null argument");
    info->n_blocks = L->n_blocks;
    info->n_owned = L->n_owned;
    info->n_fast_blocks = L->n_fast_blocks;
    info->n_general_blocks = L->n_owned - L->n_fast_blocks;
    info->n_boundary_cells = L->n_bc;
    info->has_temporal_storage = L->has_temporal;
    info->has_post_collision = L->has_post;
    info->n_xrun_blocks = (int32_t)(L->n_linked_items[LUDWIG_PART_ALL] / 8);   // 8 planes per block
    info->device_bytes = L->device_bytes;
    return LUDWIG_OK;
}

// ============================================================================================================================
// Multi-GPU: communicator, halo plan, exchange, distributed step (include/ludwig_hip.h "multi-GPU")
// ============================================================================================================================
}  // extern "C"  (helpers below are internal)

#include <dlfcn.h>
#include <link.h>
#include <rccl/rccl.h>      // types and prototypes only: the functions are resolved at run time, the library is not linked

namespace {

struct RcclApi {
    void *handle = nullptr;
    std::string path;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};

int find_loaded_rccl(struct dl_phdr_info *info, size_t, void *data)
{
    if (info->dlpi_name && strstr(info->dlpi_name, "librccl")) {
        *static_cast<std::string *>(data) = info->dlpi_name;
        return 1;
    }
    return 0;
}

// The RCCL already mapped into the process wins (a host that also uses PyTorch has torch's copy loaded, and two RCCLs in one process
// each bring their own kernels, proxy threads and IPC state); else LUDWIG_RCCL_LIB, else the loader's librccl.so.1 / librccl.so.
RcclApi *rccl()
{
    static RcclApi api;
    static bool tried = false;
    if (tried) return api.handle ? &api : nullptr;
    tried = true;
    std::string loaded;
    dl_iterate_phdr(find_loaded_rccl, &loaded);
    const char *env_path = env::rccl_lib();
    std::vector<std::string> names;
    if (!loaded.empty()) names.push_back(loaded);
    if (env_path) names.push_back(env_path);
    names.push_back("librccl.so.1");
    names.push_back("librccl.so");
    for (const std::string &n : names) {
        void *h = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) continue;
        api.handle = h;
        api.path = n;
        break;
    }
    if (!api.handle) { g_err = std::string("librccl not found: ") + (dlerror() ? dlerror() : "?"); return nullptr; }
#define LW_SYM(f) api.f = reinterpret_cast<decltype(api.f)>(dlsym(api.handle, "nccl" #f)); if (!api.f) { g_err = "librccl lacks nccl" #f; api.handle = nullptr; return nullptr; }
    LW_SYM(GetUniqueId) LW_SYM(CommInitRank) LW_SYM(CommDestroy) LW_SYM(GroupStart) LW_SYM(GroupEnd) LW_SYM(Send) LW_SYM(Recv)
    LW_SYM(AllReduce) LW_SYM(GetErrorString)
#undef LW_SYM
    return &api;
}

#define LW_NCCL(api, call)                                                                                          \
    do {                                                                                                            \
        ncclResult_t r_ = (call);                                                                                   \
        if (r_ != ncclSuccess) return fail(LUDWIG_ERR_HIP, "%s failed: %s (%s:%d)", #call, (api)->GetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

constexpr int HALO_GROUP_COMPS[LUDWIG_HALO_GROUPS] = {Q, 3, Q, 1};      // populations, velocity, f_post_collision, rho
constexpr int TIMING_RING = 256;

}  // namespace

struct LudwigComm {
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1, device = 0;
    HipStream stream;                   // small collectives (diagnostics)
    Dev<float> scratch;                 // 2 x 256 floats
};

struct LudwigHaloPlan {
    LudwigLevel *L = nullptr;           // borrowed
    LudwigComm *comm = nullptr;         // borrowed
    std::vector<int32_t> peers;
    struct Group {
        int64_t n_send = 0, n_recv = 0, n_send_oct = 0, n_recv_oct = 0, n_send_single = 0, n_recv_single = 0;
        Dev<float> send_buf, recv_buf;
        Dev<uint4> send_desc, recv_desc;
        Dev<uint2> send_single, recv_single;
        std::vector<int64_t> send_off, recv_off;       // [n_peers + 1] prefix sums
    } g[LUDWIG_HALO_GROUPS];
    HipStream s_comm;                                  // high priority: a queue of its own beside the stepping stream
    HipEvent ev_ready, ev_done;
    bool pending = false;                              // an exchange has been queued since the last wait
    bool self_via_rccl = false;                        // LUDWIG_HALO_SELF_VIA_RCCL: messages to this rank itself go through ncclSend / ncclRecv
    bool timing = false;
    bool in_stream = false;                            // ludwig_halo_plan_in_stream: the exchange runs ON the level's stream (no event hand-over)
    HipEvent t0[TIMING_RING], t1[TIMING_RING];
    int64_t n_timed = 0, n_read = 0;
};

namespace {

// message elements (reference-layout offsets, in message order) -> octet descriptors of the device array (kernels.hpp: k_pack_octets)
int build_octets(const LudwigLevel *L, int K, const int64_t *index, int64_t n, std::vector<uint4> &out, std::vector<uint2> &singles)
{
    out.clear();
    singles.clear();
    const int64_t sk = L->sk, total = sk * K;
    int64_t cur_oct = -1;
    int last_j = -1;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t off = index[i];
        if (off < 0 || off >= total) return fail(LUDWIG_ERR_INVALID, "halo plan: element offset %lld outside the field (%lld elements)", (long long)off, (long long)total);
        const int64_t k = off / sk, r = off - k * sk;
        const int64_t blk = L->ref2int.empty() ? (r >> 9) : (int64_t)L->ref2int[(size_t)(r >> 9)];
        const int64_t in = (blk * K + k) * CELLS + (r & 511);
        const int64_t oct = in >> 3;
        const int j = (int)(in & 7);
        if (oct != cur_oct || j <= last_j) {             // a new sector, or not ascending inside it: a new descriptor
            if (oct >= ((int64_t)1 << 32) || i >= ((int64_t)1 << 32)) return fail(LUDWIG_ERR_INVALID, "halo plan: level too large for 32-bit octet descriptors");
            out.push_back(make_uint4((uint32_t)oct, (uint32_t)i, 0u, 0u));
            cur_oct = oct;
        }
        out.back().z |= 1u << j;
        last_j = j;
    }
    // octets with one or two members: one thread per member instead of eight per octet (kernels.hpp)
    if (n >= ((int64_t)1 << 29)) return fail(LUDWIG_ERR_INVALID, "halo plan: message too long for 29-bit positions");
    std::vector<uint4> full;
    full.reserve(out.size());
    for (const uint4 &d : out) {
        if (__builtin_popcount(d.z) >= 3) { full.push_back(d); continue; }
        uint32_t pos = d.y;
        for (uint32_t j = 0; j < 8; ++j)
            if ((d.z >> j) & 1u) singles.push_back(make_uint2(d.x, (pos++ << 3) | j));
    }
    out.swap(full);
    return LUDWIG_OK;
}

int halo_pack_group(LudwigHaloPlan *P, int group, int field, hipStream_t st)
{
    LudwigLevel *L = P->L;
    LudwigHaloPlan::Group &G = P->g[group];
    if (G.n_send == 0) return LUDWIG_OK;
    const FieldDesc d = field_desc(L, field);
    if (!d.ptr || d.es != 4 || d.comps != HALO_GROUP_COMPS[group]) return fail(LUDWIG_ERR_INVALID, "halo group %d cannot move field %d", group, field);
    hipLaunchKernelGGL(k_pack_octets, dim3((unsigned)((G.n_send_oct * 8 + G.n_send_single + 255) / 256)), dim3(256), 0, st, (const float *)d.ptr, G.send_desc,
                       G.n_send_oct, G.send_single, G.n_send_single, G.send_buf);
    LW_HIP(hipGetLastError());
    return LUDWIG_OK;
}

int halo_unpack_group(LudwigHaloPlan *P, int group, int field, hipStream_t st)
{
    LudwigLevel *L = P->L;
    LudwigHaloPlan::Group &G = P->g[group];
    if (G.n_recv == 0) return LUDWIG_OK;
    const FieldDesc d = field_desc(L, field);
    if (!d.ptr || d.es != 4 || d.comps != HALO_GROUP_COMPS[group]) return fail(LUDWIG_ERR_INVALID, "halo group %d cannot move field %d", group, field);
    hipLaunchKernelGGL(k_unpack_octets, dim3((unsigned)((G.n_recv_oct * 8 + G.n_recv_single + 255) / 256)), dim3(256), 0, st, (float *)d.ptr, G.recv_desc,
                       G.n_recv_oct, G.recv_single, G.n_recv_single, G.recv_buf);
    LW_HIP(hipGetLastError());
    return LUDWIG_OK;
}

// what has to be true on the LEVEL's stream before an exchange may read `field` (pack side) / write its ghosts (unpack side)
int halo_prepare_field(LudwigLevel *L, int group, int field)
{
    if (field == LUDWIG_RHO) {
        const int r = ensure_rho(L);                    // an elided rho is produced now, on the level's stream
        if (r) return r;
    }
    (void)group;
    return before_external_write(L, field);             // the ghosts of `field` are about to be written: saved-state alias, lazy rho inputs
}

}  // namespace

extern "C" {

int ludwig_comm_unique_id(void *id_out)
{
    if (!id_out) return fail(LUDWIG_ERR_INVALID, "null argument");
    RcclApi *api = rccl();
    if (!api) return fail(LUDWIG_ERR_STATE, "RCCL unavailable: %s", g_err.c_str());
    static_assert(sizeof(ncclUniqueId) == LUDWIG_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    LW_NCCL(api, api->GetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return LUDWIG_OK;
}

int ludwig_comm_create(const void *unique_id, int rank, int world, int device, LudwigComm **out)
{
    if (out) *out = nullptr;
    if (!unique_id || !out || world < 1 || rank < 0 || rank >= world) return fail(LUDWIG_ERR_INVALID, "bad argument");
    RcclApi *api = rccl();
    if (!api) return fail(LUDWIG_ERR_STATE, "RCCL unavailable: %s", g_err.c_str());
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(LUDWIG_ERR_NO_DEVICE, "no HIP device %d", device);
    LW_HIP(hipSetDevice(device));
    LudwigComm *c = new (std::nothrow) LudwigComm();
    if (!c) return fail(LUDWIG_ERR_ALLOC, "host allocation failed");
    c->rank = rank; c->world = world; c->device = device;
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof id);
    ncclResult_t r = api->CommInitRank(&c->comm, world, id, rank);
    if (r != ncclSuccess) { delete c; return fail(LUDWIG_ERR_HIP, "ncclCommInitRank: %s", api->GetErrorString(r)); }
    int e = c->stream.create(hipStreamNonBlocking);
    if (!e) e = c->scratch.alloc(512);
    if (e) { ludwig_comm_destroy(c); return fail(LUDWIG_ERR_HIP, "communicator set-up: %s", hipGetErrorString((hipError_t)e)); }
    *out = c;
    return LUDWIG_OK;
}

void ludwig_comm_destroy(LudwigComm *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    RcclApi *api = rccl();
    if (c->comm && api) (void)api->CommDestroy(c->comm);
    delete c;
}

int ludwig_comm_allreduce_f32(LudwigComm *c, float *buf, int32_t n, int32_t op)
{
    if (!c || !buf || n < 0 || n > 256) return fail(LUDWIG_ERR_INVALID, "bad argument (at most 256 values)");
    if (op != 0 && op != 2 && op != 3) return fail(LUDWIG_ERR_INVALID, "op must be 0 (sum), 2 (max) or 3 (min)");
    if (n == 0) return LUDWIG_OK;
    RcclApi *api = rccl();
    if (!api) return fail(LUDWIG_ERR_STATE, "RCCL unavailable");
    LW_HIP(hipSetDevice(c->device));
    // min / max: what the backend makes of a NaN is its own business, so NaN travels as a flag (second reduction, max)
    float host[512];
    for (int i = 0; i < n; ++i) {
        const bool nan = buf[i] != buf[i];
        host[i] = (nan && op != 0) ? (op == 3 ? __builtin_inff() : -__builtin_inff()) : buf[i];
        host[256 + i] = nan ? 1.0f : 0.0f;
    }
    LW_HIP(hipMemcpyAsync(c->scratch, host, 512 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    LW_NCCL(api, api->AllReduce(c->scratch, c->scratch, (size_t)n, ncclFloat, (ncclRedOp_t)op, c->comm, c->stream));
    if (op != 0) LW_NCCL(api, api->AllReduce(c->scratch + 256, c->scratch + 256, (size_t)n, ncclFloat, ncclMax, c->comm, c->stream));
    LW_HIP(hipMemcpyAsync(host, c->scratch, 512 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    LW_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) buf[i] = (op != 0 && host[256 + i] > 0.0f) ? __builtin_nanf("") : host[i];
    return LUDWIG_OK;
}

void ludwig_halo_plan_destroy(LudwigHaloPlan *P)
{
    if (!P) return;
    if (P->L) (void)hipSetDevice(P->L->device);
    if (P->s_comm) (void)hipStreamSynchronize(P->s_comm);
    delete P;
}

int ludwig_halo_plan_create(LudwigLevel *L, LudwigComm *comm, const LudwigHaloPlanDesc *desc, LudwigHaloPlan **out)
{
    if (out) *out = nullptr;
    if (!L || !desc || !out || desc->n_peers < 0 || (desc->n_peers > 0 && !desc->peer_ranks)) return fail(LUDWIG_ERR_INVALID, "bad argument");
    if (comm && comm->device != L->device) return fail(LUDWIG_ERR_INVALID, "communicator and level live on different devices");
    if (const int r = ban_records(L)) return r;              // a level whose arrays are exchanged keeps them as populations
    for (int p = 0; p < desc->n_peers; ++p) {
        const int r = desc->peer_ranks[p];
        if (comm ? (r < 0 || r >= comm->world) : r != 0) return fail(LUDWIG_ERR_INVALID, "peer %d: rank %d not in the communicator", p, r);
    }
    LW_HIP(hipSetDevice(L->device));
    std::unique_ptr<LudwigHaloPlan> P(new (std::nothrow) LudwigHaloPlan());
    if (!P) return fail(LUDWIG_ERR_ALLOC, "host allocation failed");
    P->L = L; P->comm = comm;
    P->peers.assign(desc->peer_ranks, desc->peer_ranks + desc->n_peers);
    P->self_via_rccl = comm && env::halo_self_via_rccl();
    int rc = LUDWIG_OK;
    for (int g = 0; g < LUDWIG_HALO_GROUPS && rc == LUDWIG_OK; ++g) {
        LudwigHaloPlan::Group &G = P->g[g];
        G.send_off.assign((size_t)desc->n_peers + 1, 0);
        G.recv_off.assign((size_t)desc->n_peers + 1, 0);
        for (int p = 0; p < desc->n_peers; ++p) {
            const int64_t ns = desc->send_count[g] ? desc->send_count[g][p] : 0, nr = desc->recv_count[g] ? desc->recv_count[g][p] : 0;
            if (ns < 0 || nr < 0) rc = fail(LUDWIG_ERR_INVALID, "negative count");
            G.send_off[(size_t)p + 1] = G.send_off[(size_t)p] + ns;
            G.recv_off[(size_t)p + 1] = G.recv_off[(size_t)p] + nr;
        }
        if (rc) break;
        G.n_send = G.send_off.back(); G.n_recv = G.recv_off.back();
        if ((G.n_send > 0 && !desc->send_index[g]) || (G.n_recv > 0 && !desc->recv_index[g])) { rc = fail(LUDWIG_ERR_INVALID, "group %d: index list missing", g); break; }
        if (g == 2 && (G.n_send || G.n_recv) && !L->has_post) { rc = fail(LUDWIG_ERR_STATE, "group 2 (f_post_collision) on a level without that array"); break; }
        std::vector<uint4> sd, rd;
        std::vector<uint2> ss, rs;
        if ((rc = build_octets(L, HALO_GROUP_COMPS[g], desc->send_index[g], G.n_send, sd, ss))) break;
        if ((rc = build_octets(L, HALO_GROUP_COMPS[g], desc->recv_index[g], G.n_recv, rd, rs))) break;
        G.n_send_oct = (int64_t)sd.size(); G.n_recv_oct = (int64_t)rd.size();
        G.n_send_single = (int64_t)ss.size(); G.n_recv_single = (int64_t)rs.size();
        hipError_t e = hipSuccess;
        upload_table(e, sd, G.send_desc);
        upload_table(e, rd, G.recv_desc);
        upload_table(e, ss, G.send_single);
        upload_table(e, rs, G.recv_single);
        if (e != hipSuccess) { rc = fail(LUDWIG_ERR_HIP, "halo descriptors: %s", hipGetErrorString(e)); break; }
        e = (hipError_t)G.send_buf.alloc((size_t)G.n_send);
        if (e == hipSuccess) e = (hipError_t)G.recv_buf.alloc((size_t)G.n_recv);
        if (e != hipSuccess) rc = fail(LUDWIG_ERR_ALLOC, "halo buffers: %s", hipGetErrorString(e));
    }
    if (rc) return rc;
    int pr_least = 0, pr_greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest);
    if (e == hipSuccess) e = (hipError_t)P->s_comm.create(hipStreamNonBlocking, pr_greatest);
    if (e == hipSuccess) e = (hipError_t)P->ev_ready.create();
    if (e == hipSuccess) e = (hipError_t)P->ev_done.create();
    if (e != hipSuccess) return fail(LUDWIG_ERR_HIP, "halo plan streams: %s", hipGetErrorString(e));
    *out = P.release();
    return LUDWIG_OK;
}

int ludwig_halo_plan_timing(LudwigHaloPlan *P, int enable)
{
    if (!P) return fail(LUDWIG_ERR_INVALID, "null plan");
    LW_HIP(hipSetDevice(P->L->device));
    if (enable && !P->t0[0]) {               // all 2 x TIMING_RING events, or none: made beside the plan, then moved in
        std::vector<HipEvent> made(2 * TIMING_RING);
        for (HipEvent &ev : made) LW_HIP((hipError_t)ev.create(hipEventDefault));
        for (int i = 0; i < TIMING_RING; ++i) { P->t0[i] = std::move(made[2 * i]); P->t1[i] = std::move(made[2 * i + 1]); }
    }
    P->timing = enable != 0;
    P->n_read = P->n_timed;
    return LUDWIG_OK;
}

int ludwig_halo_plan_in_stream(LudwigHaloPlan *P, int enable)
{
    if (!P) return fail(LUDWIG_ERR_INVALID, "null plan");
    if (P->pending) {                    // an exchange of the other kind is in flight: the level's stream joins it first
        const int r = ludwig_halo_wait(P);
        if (r) return r;
    }
    P->in_stream = enable != 0;
    return LUDWIG_OK;
}

int ludwig_halo_plan_exchange_ms(LudwigHaloPlan *P, float *ms_out, int32_t max, int32_t *n_out)
{
    if (!P || !n_out || (max > 0 && !ms_out)) return fail(LUDWIG_ERR_INVALID, "null argument");
    *n_out = 0;
    if (P->n_timed - P->n_read > TIMING_RING) P->n_read = P->n_timed - TIMING_RING;
    while (P->n_read < P->n_timed && *n_out < max) {
        const int i = (int)(P->n_read % TIMING_RING);
        float ms = 0.0f;
        LW_HIP(hipEventElapsedTime(&ms, P->t0[i], P->t1[i]));
        ms_out[(*n_out)++] = ms;
        ++P->n_read;
    }
    return LUDWIG_OK;
}

int ludwig_halo_plan_pack(LudwigHaloPlan *P, int32_t group, int32_t field, void *hip_stream)
{
    if (!P || group < 0 || group >= LUDWIG_HALO_GROUPS) return fail(LUDWIG_ERR_INVALID, "bad argument");
    LW_HIP(hipSetDevice(P->L->device));
    LW_ENSURE_POPULATIONS(P->L);
    if (field == LUDWIG_RHO) { const int r = ensure_rho(P->L); if (r) return r; }
    return halo_pack_group(P, group, field, hip_stream ? (hipStream_t)hip_stream : P->L->stream);
}

int ludwig_halo_plan_unpack(LudwigHaloPlan *P, int32_t group, int32_t field, void *hip_stream)
{
    if (!P || group < 0 || group >= LUDWIG_HALO_GROUPS) return fail(LUDWIG_ERR_INVALID, "bad argument");
    LW_HIP(hipSetDevice(P->L->device));
    ++P->L->version;
    { const int r = before_external_write(P->L, field); if (r) return r; }
    return halo_unpack_group(P, group, field, hip_stream ? (hipStream_t)hip_stream : P->L->stream);
}

int ludwig_halo_plan_buffers(const LudwigHaloPlan *P, int32_t group, void **send_dev, int64_t *n_send, void **recv_dev, int64_t *n_recv)
{
    if (!P || group < 0 || group >= LUDWIG_HALO_GROUPS) return fail(LUDWIG_ERR_INVALID, "bad argument");
    const LudwigHaloPlan::Group &G = P->g[group];
    if (send_dev) *send_dev = G.send_buf;
    if (n_send) *n_send = G.n_send;
    if (recv_dev) *recv_dev = G.recv_buf;
    if (n_recv) *n_recv = G.n_recv;
    return LUDWIG_OK;
}

static double host_now_us()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

int ludwig_halo_exchange(LudwigHaloPlan *P, int32_t n, const int32_t *groups, const int32_t *fields)
{
    if (!P || n < 0 || n > LUDWIG_HALO_GROUPS || (n > 0 && (!groups || !fields))) return fail(LUDWIG_ERR_INVALID, "bad argument");
    // LUDWIG_HALO_TRACE=1: host microseconds of the three parts of this call on stderr (what an exchange costs the host)
    const bool trace = env::halo_trace();
    const double h0 = trace ? host_now_us() : 0.0;
    double h1 = 0.0, h2 = 0.0;
    LudwigLevel *L = P->L;
    LW_HIP(hipSetDevice(L->device));
    for (int i = 0; i < n; ++i) {
        if (groups[i] < 0 || groups[i] >= LUDWIG_HALO_GROUPS) return fail(LUDWIG_ERR_INVALID, "bad group %d", groups[i]);
        const int r = halo_prepare_field(L, groups[i], fields[i]);     // may queue work on the level's stream: before the event below
        if (r) return r;
    }
    // nothing to send or to receive in these groups (a level this rank shares with nobody): no event, no kernel
    {
        int64_t moved = 0;
        for (int i = 0; i < n; ++i) moved += P->g[groups[i]].n_send + P->g[groups[i]].n_recv;
        if (moved == 0) return LUDWIG_OK;
    }
    ++L->version;
    // in-stream mode: pack, transfer and unpack are queued on the level's own stream - what follows on that stream follows the exchange,
    // at the price of no overlap and to the gain of two cross-stream hand-overs (tens of microseconds of idle device each, more than a
    // small level's whole exchange)
    const hipStream_t xs = P->in_stream ? L->stream : P->s_comm;
    if (!P->in_stream) {
        LW_HIP(hipEventRecord(P->ev_ready, L->stream));
        LW_HIP(hipStreamWaitEvent(P->s_comm, P->ev_ready, 0));
    }
    const int slot = (int)(P->n_timed % TIMING_RING);
    if (P->timing) LW_HIP(hipEventRecord(P->t0[slot], xs));
    for (int i = 0; i < n; ++i) {
        const int r = halo_pack_group(P, groups[i], fields[i], xs);
        if (r) return r;
    }
    if (trace) h1 = host_now_us();
    RcclApi *api = P->comm ? rccl() : nullptr;
    bool any_remote = false;
    for (size_t p = 0; p < P->peers.size(); ++p)
        if (P->comm && (P->peers[p] != P->comm->rank || P->self_via_rccl)) any_remote = true;
    if (any_remote && !api) return fail(LUDWIG_ERR_STATE, "RCCL unavailable");
    if (any_remote) LW_NCCL(api, api->GroupStart());
    for (size_t p = 0; p < P->peers.size(); ++p) {
        const bool self = !P->comm || (P->peers[p] == P->comm->rank && !P->self_via_rccl);
        for (int i = 0; i < n; ++i) {
            LudwigHaloPlan::Group &G = P->g[groups[i]];
            const int64_t s0 = G.send_off[p], ns = G.send_off[p + 1] - s0, r0 = G.recv_off[p], nr = G.recv_off[p + 1] - r0;
            if (self) {
                if (ns != nr) return fail(LUDWIG_ERR_INVALID, "peer %zu is this rank itself but sends %lld and receives %lld elements", p, (long long)ns, (long long)nr);
                if (ns) LW_HIP(hipMemcpyAsync(G.recv_buf + r0, G.send_buf + s0, (size_t)ns * 4, hipMemcpyDeviceToDevice, xs));
            } else {
                if (ns) LW_NCCL(api, api->Send(G.send_buf + s0, (size_t)ns, ncclFloat, P->peers[p], P->comm->comm, xs));
                if (nr) LW_NCCL(api, api->Recv(G.recv_buf + r0, (size_t)nr, ncclFloat, P->peers[p], P->comm->comm, xs));
            }
        }
    }
    if (any_remote) LW_NCCL(api, api->GroupEnd());
    if (trace) h2 = host_now_us();
    for (int i = 0; i < n; ++i) {
        const int r = halo_unpack_group(P, groups[i], fields[i], xs);
        if (r) return r;
    }
    if (P->timing) { LW_HIP(hipEventRecord(P->t1[slot], xs)); ++P->n_timed; }
    if (!P->in_stream) {
        LW_HIP(hipEventRecord(P->ev_done, P->s_comm));
        P->pending = true;
    }
    if (trace) fprintf(stderr, "[ludwig_halo_exchange] host us: events + pack %.1f, send/recv group (%zu peers) %.1f, unpack + event %.1f\n", h1 - h0, P->peers.size(), h2 - h1, host_now_us() - h2);
    return LUDWIG_OK;
}

int ludwig_halo_wait(LudwigHaloPlan *P)
{
    if (!P) return fail(LUDWIG_ERR_INVALID, "null plan");
    if (!P->pending) return LUDWIG_OK;
    LW_HIP(hipSetDevice(P->L->device));
    LW_HIP(hipStreamWaitEvent(P->L->stream, P->ev_done, 0));
    P->pending = false;
    return LUDWIG_OK;
}

int ludwig_step_distributed(LudwigLevel *L, LudwigHaloPlan *P, const LudwigLevel *parent, int64_t t_sub, float u_curr, float parent_tau,
                            float temporal_weight, const LudwigStepFlags *fl)
{
    if (!L || !P || !fl || P->L != L) return fail(LUDWIG_ERR_INVALID, "bad argument (the plan must belong to the level)");
    int rc;
    // interior blocks read and write owned cells only: they run while the ghosts of their input are still arriving
    if ((rc = launch_stream_collide(L, parent, t_sub, u_curr, parent_tau, temporal_weight, fl, LUDWIG_PART_INTERIOR))) return rc;
    if ((rc = ludwig_halo_wait(P))) return rc;
    if ((rc = launch_stream_collide(L, parent, t_sub, u_curr, parent_tau, temporal_weight, fl, LUDWIG_PART_BOUNDARY))) return rc;
    if (L->has_post) {
        // the correction rewrites f_out from post-collision values of neighbour cells (src/bouzidi_kernel.jl:44-77): the few that
        // live across a cut are fetched in between, and waited for
        if (P->g[2].n_send || P->g[2].n_recv) {
            // a few thousand elements, needed at once: on the level's own stream (two cross-stream hand-overs cost more than the messages)
            const int32_t grp = 2, fld = LUDWIG_F_POST;
            const bool mode = P->in_stream;
            P->in_stream = true;
            rc = ludwig_halo_exchange(P, 1, &grp, &fld);
            P->in_stream = mode;
            if (rc) return rc;
        }
        if ((rc = launch_bouzidi(L, t_sub, fl->q_min_threshold))) return rc;
    }
    const bool out_temp = t_sub % 2 == 0;                    // reference src/solver_control.jl:35-41
    const int32_t grps[2] = {0, 1}, flds[2] = {out_temp ? LUDWIG_F_TEMP : LUDWIG_F, out_temp ? LUDWIG_VEL_TEMP : LUDWIG_VEL};
    return ludwig_halo_exchange(P, 2, grps, flds);           // left in flight: the next call's interior blocks run under it
}

}  // extern "C"
