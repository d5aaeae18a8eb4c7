// Device kernels of libludwig_hip.so (gfx950 / CDNA4 only).
//
// stream-collide  : reference src/physics_kernels.jl:9-358 (+ src/physics_utils.jl, src/physics_interpolation.jl)
// bouzidi         : reference src/bouzidi_kernel.jl:13-92
//
// Arithmetic contract: every floating-point expression keeps the reference's operand order and is
// compiled with -ffp-contract=off, so results are bit-identical to the scalar CPU restatement for
// finite inputs. Multiplications by the lattice constants 0/+1/-1 are resolved at compile time
// (x*1 = x, x*-1 = -x exactly; a dropped x*0 term only changes the sign of an exact zero).
//
// Mapping: one 64-lane wavefront = one 8x8 z-plane of one 8^3 block (lane = x + 8y); a 256-thread
// workgroup = 4 such planes chosen by the host's work list (by default the same plane of 4 x-consecutive
// blocks, which the library keeps consecutive in memory, see ludwig_hip.hip "Block order"). The block index and z
// are wave-uniform, so the 27 neighbour block ids come through the scalar cache and each population load is one
// coalesced, aligned 256-B access; the +-1 shift in x is a lane shift plus an LDS column between neighbouring waves.
//
// Storage (round 3): the device arrays are BLOCK-major - element (cell, block b, component k) of a K-component field lives
// at ((b * K + k) * 512 + cell): the 27 populations of a block are one contiguous 54-KiB piece. The reference's arrays are
// population-major, [8,8,8,n_blocks,K] (src/blocks.jl:118-150): 27 + 27 concurrent streams n_blocks x 2 KiB apart, and at
// some distances (which depend on nothing but n_blocks) they load MI355X's memory system unevenly - 5-30 % of the step
// (profiles/r03_stride_*). With block-major storage there is no such distance; the ABI translates (ludwig_hip.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "lattice.hpp"
#include "jl_math.h"

namespace lw {

struct SCParams {
    const float *f_in;
    float *f_out;
    float *f_post;            // nullptr unless store_post_collision
    const uint32_t *post_rows; // [n_blocks][2]: bit z*8+y of a block's 64 = the x-row (y, z) holds a cell f_post_collision is read at;
                              // nullptr = every row of a block flagged FLAG_STORE_POST
    const float *vel_in;
    float *vel_out;
    float *rho;
    const uint8_t *obstacle;
    const float *sponge;
    const float *wall_dist;
    const int32_t *meta;      // [n_blocks][NBR_STRIDE]
    const int32_t *items;     // work list, one entry per wave: (block << 3) | z, or -1
    // parent level (coarse -> fine interface), unused on level 1
    const float *pf_new, *pf_old, *prho_new, *prho_old, *pvel_new, *pvel_old;
    float tau, tau_parent, c_wale, nu_bg, u_inlet, inlet_turbulence, temporal_weight;
    int32_t is_level_1, is_symmetric, nx_g, ny_g, nz_g;
    int32_t wall_model, seed, use_temporal, sponge_blend;
    // coarse -> fine interface pass: values of interpolate_with_rescaling for every (cell, population) link of this
    // level that needs one, precomputed densely by k_interface_links: f_iface[(k * n_iface_blocks + gbi) * 512 + cell]
    float *f_iface;
    int32_t n_iface_blocks;
    // 0: this launch leaves `rho` unwritten - nobody reads it before the level's next step unless asked, and then
    // k_stream_collide_xrun<.., RHO_ONLY> recomputes it from the same inputs (ludwig_hip.hip "lazy rho")
    int32_t store_rho;
    // non-null: copy_to_old!'s rho part fused into this launch - every cell saves its old rho here before storing the new one
    // (whole-level launches of a level without ghost blocks only; ludwig_hip.hip "rho_old in the step")
    float *rho_old_save;
    // non-null (k_records_from_populations, k_step_records): the step stores each cell's 11-float collision record here and leaves f_out, vel_out
    // and rho unwritten ("Record step" below)
    float *rec_out;
    const float *rec_in;      // k_step_records, k_materialise: the records read
};

template <int K, int N, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (K < N) {
        f(std::integral_constant<int, K>{});
        static_for<K + 1, N>(f);
    }
}

// Julia's max() propagates NaN (reference uses Base.max throughout)
__device__ __forceinline__ float jl_max(float a, float b)
{
    return (a != a) ? a : ((b != b) ? b : (a > b ? a : b));
}
__device__ __forceinline__ float jl_clamp(float x, float lo, float hi)
{
    return x > hi ? hi : (x < lo ? lo : x);
}
// Base.^(::Float32, ::Float32) and Base.log(::Float32) evaluate in Float64 and round once. The double log2 / exp2 / log are
// jl_math.h's (IEEE +,-,*,/ only), the same source the CPU oracle compiles: identical bits on both sides.
__device__ __forceinline__ float jl_pow(float x, float y) { return lw_powf(x, y); }
__device__ __forceinline__ float jl_log(float x) { return lw_logf(x); }

// c * v for c in {-1,0,1} resolved at compile time; `first` says whether the running sum is empty
template <int C>
__device__ __forceinline__ void acc_signed(float &sum, bool &empty, float v)
{
    if constexpr (C != 0) {
        const float t = C > 0 ? v : -v;
        sum = empty ? t : sum + t;
        empty = false;
    }
}
// cx*a + cy*b + cz*c, left-associated like the reference, zero terms dropped
template <int K>
__device__ __forceinline__ float cdot(float a, float b, float c)
{
    float s = 0.0f;
    bool empty = true;
    acc_signed<CX(K)>(s, empty, a);
    acc_signed<CY(K)>(s, empty, b);
    acc_signed<CZ(K)>(s, empty, c);
    return s;
}

// reference src/physics_utils.jl:17-28 (Int32 products wrap)
__device__ __forceinline__ float gradient_noise(int32_t gx, int32_t gy, int32_t gz, int32_t seed)
{
    uint32_t h = (uint32_t)gx * 374761393u + (uint32_t)gy * 668265263u + (uint32_t)gz * 1274126177u + (uint32_t)seed;
    h = (h ^ (h >> 16)) * 0x85ebca6bu;
    h = (h ^ (h >> 13)) * 0xc2b2ae35u;
    h = h ^ (h >> 16);
    return ((float)(h & 0xFFFFu) / 32768.0f) - 1.0f;
}

// ---- coarse -> fine interface value, reference src/physics_interpolation.jl:16-138: the trilinear kernel; the corner
// fetch, the blend in time and the rescaling live in k_interface_sources / k_interface_links below ----
// Not probe_trilinear below: the reference's interface pass weights as a (1 - w) + b w and its probes as (1 - w) a + w b; the products
// are the same, the operands of each multiply are swapped, and the step's machine code is kept as it is.
__device__ __forceinline__ float trilin(float v000, float v100, float v010, float v110, float v001, float v101,
                                        float v011, float v111, float wx, float wy, float wz)
{
    const float c00 = v000 * (1.0f - wx) + v100 * wx;
    const float c01 = v001 * (1.0f - wx) + v101 * wx;
    const float c10 = v010 * (1.0f - wx) + v110 * wx;
    const float c11 = v011 * (1.0f - wx) + v111 * wx;
    const float c0 = c00 * (1.0f - wy) + c10 * wy;
    const float c1 = c01 * (1.0f - wy) + c11 * wy;
    return c0 * (1.0f - wz) + c1 * wz;
}

// ---- wall-model force, reference src/physics_kernels.jl:206-236 ----
#ifndef LW_WALL_INLINE
#define LW_WALL_INLINE __noinline__
#endif
// Returns the magnitude of the force, or -1 where the reference leaves F = 0; the caller turns it into F = -mag u / |u|.
// (One float in registers each way: with F returned through three references the call went through the stack - 16 B of
// scratch per lane - and the kernel lost a wave per SIMD.)
__device__ LW_WALL_INLINE float wall_model_force_mag(float dist_wall, float tau_molecular, float rho, float u_mag)
{
    float force_mag = -1.0f;
    if (dist_wall > 0.0f && dist_wall < 10.0f) {
        const float nu_visc = (tau_molecular - 0.5f) / 3.0f;
        if (u_mag > 1.0e-6f && nu_visc > 1.0e-10f) {
            float u_tau = u_mag * jl_pow(nu_visc / (dist_wall * u_mag + 1.0e-10f), 1.0f / 7.0f) *
                          jl_pow(2.0f * 8.3f, -1.0f / 7.0f);
            u_tau = jl_max(u_tau, 1.0e-6f);
            const float y_p = u_tau * dist_wall / nu_visc;
            if (y_p > 11.81f) {
                const float u_plus_law = (1.0f / KAPPA) * jl_log(y_p) + 5.2f;
                if (u_plus_law > 0.1f) {
                    u_tau = u_tau * ((u_mag / u_tau) / u_plus_law);
                    u_tau = jl_max(u_tau, 1.0e-6f);
                }
            }
            const float tau_wall = rho * u_tau * u_tau;
            const float tau_res = rho * nu_visc * (u_mag / dist_wall);
            if (tau_wall > tau_res) force_mag = (tau_wall - tau_res) / dist_wall;
        }
    }
    return force_mag;
}

// ---- addressing helpers -------------------------------------------------------------------------------------
// Block-major storage: byte offset of (cell, block b, component k) of a K-component float field = b * K * 2048 + k * 2048 + cell * 4.
// The wave's own block is wave-uniform, so its accesses are `SGPR base + 32-bit per-lane byte offset`
// (global_load/store_dword v, v_off, s[base:base+1]); only the populations pulled across a y face choose between two blocks per
// lane. NARROW (levels below 77 672 blocks = 4 GiB of f): that choice is a 32-bit byte offset from the array base too;
// WIDE: a 64-bit per-lane address (v_mad_u64_u32). Same loads, same values.
constexpr uint32_t F_BLOCK_BYTES = Q * CELLS * 4, V_BLOCK_BYTES = 3 * CELLS * 4, S_BLOCK_BYTES = CELLS * 4;
constexpr uint32_t COMP_BYTES = CELLS * 4;

template <bool WIDE>
__device__ __forceinline__ const float *cell_ptr(const float *base, int blk, uint32_t block_bytes, uint32_t inner)
{
    if constexpr (WIDE) return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + (uint64_t)(uint32_t)blk * block_bytes + inner);
    else return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + (uint32_t)((uint32_t)blk * block_bytes + inner));
}
template <bool WIDE>
__device__ __forceinline__ float ld_f32(const float *base, int blk, uint32_t block_bytes, uint32_t inner)
{
    return *cell_ptr<WIDE>(base, blk, block_bytes, inner);
}
// the wave's own block (wave-uniform id): uniform 64-bit base, 32-bit per-lane offset, at any level size
__device__ __forceinline__ float ld_own(const float *base, int blk, uint32_t block_bytes, uint32_t inner)
{
    return *reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + (uint64_t)(uint32_t)blk * block_bytes + inner);
}
// stores go to the wave's own block only: uniform 64-bit base, 32-bit per-lane offset, at any level size
__device__ __forceinline__ void st_f32(float *base, int blk, uint32_t block_bytes, uint32_t inner, float v)
{
    float *q = reinterpret_cast<float *>(reinterpret_cast<char *>(base) + (uint64_t)(uint32_t)blk * block_bytes + inner);
#ifdef LW_NT_STORES
    __builtin_nontemporal_store(v, q);
#else
    *q = v;
#endif
}
// the wave's own cell: block (wave-uniform), plane and lane
struct Own {
    int b;            // block
    uint32_t cell4;   // (x + 8 y + 64 z) * 4
};

// The 27 neighbour block ids of the wave's block, held in SGPRs, regrouped by source z-layer:
// id[g][j] for g = 0 (cz=+1: source plane z-1), 1 (cz=0), 2 (cz=-1: source plane z+1), j = (ox+1) + 3(oy+1).
struct NeighbourIds {
    int id[3][9];
    int zs[3];      // source plane index inside the source block
};

__device__ __forceinline__ NeighbourIds load_neighbour_ids(const int32_t *__restrict__ meta, int z)
{
    int nb[27];
#pragma unroll
    for (int d = 0; d < 27; ++d) nb[d] = meta[d];            // wave-uniform -> scalar loads, one burst
    NeighbourIds n;
    const bool z_lo = z == 0, z_hi = z == 7;                 // wave-uniform
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int lo = nb[j], mid = nb[9 + j], hi = nb[18 + j];   // values, not lvalues (see source_block)
        n.id[0][j] = z_lo ? lo : mid;
        n.id[1][j] = mid;
        n.id[2][j] = z_hi ? hi : mid;
    }
    n.zs[0] = (z - 1) & 7; n.zs[1] = z; n.zs[2] = (z + 1) & 7;
    return n;
}

// per-lane position inside the 8x8 plane and the face flags the pull needs
struct LanePos {
    int x, y;
    bool x0, x7, y0, y7;
};

// source block id (per lane) of population k: own block or the x / y / xy neighbour in the layer cz selects
template <int K>
__device__ __forceinline__ int source_block(const NeighbourIds &n, const LanePos &l)
{
    constexpr int cx = CX(K), cy = CY(K), g = 1 - CZ(K);
    const bool xo = cx == 1 ? l.x0 : (cx == -1 ? l.x7 : false);
    const bool yo = cy == 1 ? l.y0 : (cy == -1 ? l.y7 : false);
    // copy to values first: a ?: between array ELEMENTS is an lvalue select, which keeps the table in scratch memory
    const int c00 = n.id[g][4], cX = n.id[g][4 - cx], cY = n.id[g][4 - 3 * cy], cXY = n.id[g][4 - cx - 3 * cy];
    int sel = c00;
    if constexpr (cx != 0 && cy != 0) sel = xo ? (yo ? cXY : cX) : (yo ? cY : c00);
    else if constexpr (cx != 0) sel = xo ? cX : c00;
    else if constexpr (cy != 0) sel = yo ? cY : c00;
    return sel;
}
// ---- the WALE model, reference src/physics_kernels.jl:251-300: ONE source for the step (finish_cell takes nu_eddy and the compiler
// drops s2 and code) and for the observers (k_subgrid), so both get the same bits from the same gradient ----
// nu_eddy: the effective value after the floor, what the step turns into tau_turb. s2 = 2 OP2 = |S|^2 = 2 S_ij S_ij (the doubling is
// exact). code: SUBGRID_NO_OP1 - OP1 <= 1e-12 (or NaN), SUBGRID_NO_DENOM - denom <= 1e-12 (or NaN), SUBGRID_FLOOR - the model is
// evaluated and is not above nu_bg, so the floor wins (a NaN model value, which jl_max propagates, is here too), SUBGRID_MODEL - the
// model is above the floor.
constexpr int SUBGRID_NO_OP1 = 0, SUBGRID_NO_DENOM = 1, SUBGRID_FLOOR = 2, SUBGRID_MODEL = 3;
struct WaleState {
    float nu_eddy, s2;
    int code;
};
__device__ __forceinline__ WaleState wale_state(float g11, float g12, float g13, float g21, float g22, float g23, float g31, float g32,
                                                float g33, float c_wale, float nu_bg)
{
    const float gsq11 = g11 * g11 + g12 * g21 + g13 * g31;
    const float gsq12 = g11 * g12 + g12 * g22 + g13 * g32;
    const float gsq13 = g11 * g13 + g12 * g23 + g13 * g33;
    const float gsq21 = g21 * g11 + g22 * g21 + g23 * g31;
    const float gsq22 = g21 * g12 + g22 * g22 + g23 * g32;
    const float gsq23 = g21 * g13 + g22 * g23 + g23 * g33;
    const float gsq31 = g31 * g11 + g32 * g21 + g33 * g31;
    const float gsq32 = g31 * g12 + g32 * g22 + g33 * g32;
    const float gsq33 = g31 * g13 + g32 * g23 + g33 * g33;

    const float tr_gsq = gsq11 + gsq22 + gsq33;
    const float tr_term = tr_gsq / 3.0f;
    const float Sd11 = gsq11 - tr_term, Sd22 = gsq22 - tr_term, Sd33 = gsq33 - tr_term;
    const float Sd12 = 0.5f * (gsq12 + gsq21), Sd13 = 0.5f * (gsq13 + gsq31), Sd23 = 0.5f * (gsq23 + gsq32);
    const float S12 = 0.5f * (g12 + g21), S13 = 0.5f * (g13 + g31), S23 = 0.5f * (g23 + g32);
    const float OP1 = Sd11 * Sd11 + Sd22 * Sd22 + Sd33 * Sd33 + 2.0f * (Sd12 * Sd12 + Sd13 * Sd13 + Sd23 * Sd23);
    const float OP2 = g11 * g11 + g22 * g22 + g33 * g33 + 2.0f * (S12 * S12 + S13 * S13 + S23 * S23);

    WaleState w;
    w.code = SUBGRID_NO_OP1;
    float nu_eddy = 0.0f;
    if (OP1 > 1.0e-12f) {
        const float OP1_32 = OP1 * sqrtf(OP1);
        const float OP2_52 = OP2 * OP2 * sqrtf(jl_max(OP2, 1.0e-12f));
        const float denom = OP2_52 + OP1 * sqrtf(sqrtf(jl_max(OP1, 1.0e-12f)));
        w.code = SUBGRID_NO_DENOM;
        if (denom > 1.0e-12f) {
            nu_eddy = (c_wale * c_wale) * OP1_32 / denom;
            w.code = nu_eddy > nu_bg ? SUBGRID_MODEL : SUBGRID_FLOOR;
        }
    }
    w.nu_eddy = jl_max(nu_eddy, nu_bg);
    w.s2 = 2.0f * OP2;
    return w;
}

// The regularized post-collision value of population K, reference src/physics_kernels.jl:324-349 without the wall-model term: a
// function of the cell's 11 collision values and nothing else. ONE source for the three places that form it - finish_cell (which
// stores it), the record step (which evaluates it at the source cell instead of loading it) and k_materialise - so under
// -ffp-contract=off all three give the same bits.
// Two floats in an even-aligned register pair: + - * on it are one v_pk_*_f32 each, IEEE per half like the scalar instruction (and
// measured to issue at the scalar instruction's cost, profiles/packed_f32_issue_cost.txt). A per-half negation is an operand modifier.
typedef float f32x2 __attribute__((ext_vector_type(2)));

// The equilibrium of a population with weight w_k and c . u = cu, reference src/physics_kernels.jl:310-313 / :330-333. ONE expression
// for T = float (one population) and T = f32x2 (two populations of the same weight at once, finish_cell's opposite directions).
template <class T>
__device__ __forceinline__ T equilibrium_value(float rho, float w_k, T cu, float usq_eq)
{
    return rho * w_k * (1.0f + 3.0f * cu + 4.5f * cu * cu - 1.5f * usq_eq);
}
// reference src/physics_utils.jl:34-39: the same with c . u and u . u formed from run-time c (sponge target, interface pass, warm start)
__device__ __forceinline__ float calculate_equilibrium(float rho, float ux, float uy, float uz, float w_k,
                                                       float cx, float cy, float cz)
{
    return equilibrium_value<float>(rho, w_k, cx * ux + cy * uy + cz * uz, ux * ux + uy * uy + uz * uz);
}
// The equilibrium at rho = 1 of the flow (u, 0, 0): what patch_missing_sources pulls across the inlet and the outlet, reference
// src/physics_kernels.jl:99-113. Not a call of equilibrium_value: the reference writes the last term as 1.5 * u * u here, which is
// (1.5 u) u, and 1.5 * usq there - other bits.
template <int K>
__device__ __forceinline__ float edge_equilibrium(float u)
{
    const float cu = (float)CX(K) * u;
    return WEIGHT(K) * (1.0f + 3.0f * cu + 4.5f * cu * cu - 1.5f * u * u);
}

// Two running sums that finish_cell advances side by side. PACKED: one register pair - a term for both is one packed add, a term
// for one a scalar add on its half. Otherwise two floats. Either way each sum receives its own terms in its own order: the same bits.
template <bool PACKED>
struct Chain2;
template <>
struct Chain2<true> {
    f32x2 v = {0.0f, 0.0f};
    __device__ __forceinline__ void add_both(float a, float b) { v += f32x2{a, b}; }
    __device__ __forceinline__ void add_first(float a) { v.x += a; }
    __device__ __forceinline__ void add_second(float b) { v.y += b; }
    __device__ __forceinline__ float first() const { return v.x; }
    __device__ __forceinline__ float second() const { return v.y; }
};
template <>
struct Chain2<false> {
    float s0 = 0.0f, s1 = 0.0f;
    __device__ __forceinline__ void add_both(float a, float b) { s0 += a; s1 += b; }
    __device__ __forceinline__ void add_first(float a) { s0 += a; }
    __device__ __forceinline__ void add_second(float b) { s1 += b; }
    __device__ __forceinline__ float first() const { return s0; }
    __device__ __forceinline__ float second() const { return s1; }
};

// The direction a population moves in, as collide_value takes it. DirConst<K>: all three components known at compile time - zero
// terms are dropped by `if constexpr`. DirLaneFace: cx = +1 with cy, cz per-lane values (the record step's outer face column, where
// one wave evaluates the rows of all nine (cy, cz) at once); a zero term is dropped by selecting the unchanged partial sum, never by
// adding a product with zero, so every lane performs the operations DirConst of its (1, cy, cz) performs: the same bits.
template <int K>
struct DirConst {
    static constexpr int cx = CX(K), cy = CY(K), cz = CZ(K);
    __device__ __forceinline__ float weight() const { return WEIGHT(K); }
    __device__ __forceinline__ float q_xx() const { return (float)cx * (float)cx - CS2_PHYSICS; }
    __device__ __forceinline__ float q_yy() const { return (float)cy * (float)cy - CS2_PHYSICS; }
    __device__ __forceinline__ float q_zz() const { return (float)cz * (float)cz - CS2_PHYSICS; }
    // cx*a + cy*b + cz*c, left-associated, zero terms dropped
    __device__ __forceinline__ float dot(float a, float b, float c) const { return cdot<K>(a, b, c); }
    // inner + 2 (xy*cx*cy + yz*cy*cz + zx*cz*cx), the sum left-associated, zero terms dropped; all three zero: + 2*0 is an exact no-op
    __device__ __forceinline__ float add_off_diagonal(float inner, float xy, float yz, float zx) const
    {
        float od = 0.0f;
        bool od_empty = true;
        acc_signed<cx * cy>(od, od_empty, xy);
        acc_signed<cy * cz>(od, od_empty, yz);
        acc_signed<cz * cx>(od, od_empty, zx);
        if constexpr (cx * cy != 0 || cy * cz != 0 || cz * cx != 0) inner = inner + 2.0f * od;
        return inner;
    }
};
// acc_signed with a per-lane c
__device__ __forceinline__ void acc_signed_lane(int c, float &sum, bool &empty, float v)
{
    const float t = c > 0 ? v : -v;
    const float next = empty ? t : sum + t;
    sum = c != 0 ? next : sum;
    empty = empty && c == 0;
}
struct DirLaneFace {
    int cy, cz;
    __device__ __forceinline__ float weight() const
    {
        const int n = (cy != 0 ? 1 : 0) + (cz != 0 ? 1 : 0);
        return n == 0 ? WEIGHT(DIR(1, 0, 0)) : (n == 1 ? WEIGHT(DIR(1, 1, 0)) : WEIGHT(DIR(1, 1, 1)));
    }
    __device__ __forceinline__ float q_xx() const { return 1.0f * 1.0f - CS2_PHYSICS; }
    __device__ __forceinline__ float q_yy() const { return cy != 0 ? 1.0f * 1.0f - CS2_PHYSICS : 0.0f * 0.0f - CS2_PHYSICS; }
    __device__ __forceinline__ float q_zz() const { return cz != 0 ? 1.0f * 1.0f - CS2_PHYSICS : 0.0f * 0.0f - CS2_PHYSICS; }
    __device__ __forceinline__ float dot(float a, float b, float c) const
    {
        float s = a;
        bool empty = false;
        acc_signed_lane(cy, s, empty, b);
        acc_signed_lane(cz, s, empty, c);
        return s;
    }
    __device__ __forceinline__ float add_off_diagonal(float inner, float xy, float yz, float zx) const
    {
        float od = 0.0f;
        bool od_empty = true;
        acc_signed_lane(cy, od, od_empty, xy);
        acc_signed_lane(cy * cz, od, od_empty, yz);
        acc_signed_lane(cz, od, od_empty, zx);
        return od_empty ? inner : inner + 2.0f * od;
    }
};
template <class DIRECTION>
__device__ __forceinline__ float collide_value(const DIRECTION d, float rho, float ux_eq, float uy_eq, float uz_eq, float Pi_xx, float Pi_yy,
                                               float Pi_zz, float Pi_xy, float Pi_yz, float Pi_zx, float one_m_omega)
{
    const float w_k = d.weight();
    const float usq_eq = ux_eq * ux_eq + uy_eq * uy_eq + uz_eq * uz_eq;
    const float cu = d.dot(ux_eq, uy_eq, uz_eq);
    const float feq = equilibrium_value<float>(rho, w_k, cu, usq_eq);
    const float inner = d.add_off_diagonal(Pi_xx * d.q_xx() + Pi_yy * d.q_yy() + Pi_zz * d.q_zz(), Pi_xy, Pi_yz, Pi_zx);
    const float f_neq_reg = (w_k * 4.5f) * inner;
    return feq + one_m_omega * f_neq_reg;
}
template <int K>
__device__ __forceinline__ float collide_value(float rho, float ux_eq, float uy_eq, float uz_eq, float Pi_xx, float Pi_yy, float Pi_zz,
                                               float Pi_xy, float Pi_yz, float Pi_zx, float one_m_omega)
{
    return collide_value(DirConst<K>{}, rho, ux_eq, uy_eq, uz_eq, Pi_xx, Pi_yy, Pi_zz, Pi_xy, Pi_yz, Pi_zx, one_m_omega);
}

// ---- Record step: storage ----
// A plain cell's post-collision state is collide_value of 11 floats: rho, u (= u_eq without the wall model), the six Pi and
// 1 - omega. A level that qualifies (ludwig_hip.hip "record step") keeps those instead of the 27 populations, the velocity and the
// density: 44 B written and 44 B read per cell update against 240. Layout rec[block][z][11][64], plane-major: a wave's plane is one
// contiguous 2 816-B piece and all 11 components sit at immediate offsets of one per-lane address.
constexpr int R_COMP = 11;
constexpr uint32_t R_PLANE_BYTES = R_COMP * 64 * 4, R_BLOCK_BYTES = 8 * R_PLANE_BYTES;
enum { R_RHO, R_UX, R_UY, R_UZ, R_PXX, R_PYY, R_PZZ, R_PXY, R_PYZ, R_PZX, R_OMO };

__device__ __forceinline__ const char *record_plane(const float *base, int blk, int z)      // wave-uniform arguments -> scalar
{
    return reinterpret_cast<const char *>(base) + (uint64_t)(uint32_t)blk * R_BLOCK_BYTES + (uint32_t)z * R_PLANE_BYTES;
}
__device__ __forceinline__ void load_record(float (&r)[R_COMP], const char *plane, uint32_t lane4)
{
    const float *q = reinterpret_cast<const float *>(plane + lane4);
#pragma unroll
    for (int c = 0; c < R_COMP; ++c) r[c] = q[c * 64];
}
// Byte offset of plane z of block blk from the array base, as the step kernel addresses a record whose block differs from lane to lane
// (the y neighbour for the lanes of a face row): 32 bits while the array is below 4 GiB (190 650 blocks), 64 bits (WIDE) beyond. The
// narrow form is `SGPR base + one VGPR`; a 64-bit per-lane address costs two registers for each of the 15 records a wave may touch.
template <bool WIDE>
using record_off_t = std::conditional_t<WIDE, uint64_t, uint32_t>;
template <bool WIDE>
__device__ __forceinline__ record_off_t<WIDE> record_offset(int blk, int z)
{
    return (record_off_t<WIDE>)(uint32_t)blk * R_BLOCK_BYTES + (uint32_t)z * R_PLANE_BYTES;
}
template <class OFF>
__device__ __forceinline__ void load_record_at(float (&r)[R_COMP], const float *base, OFF off)
{
    const float *q = reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + off);
#pragma unroll
    for (int c = 0; c < R_COMP; ++c) r[c] = q[c * 64];
}
__device__ __forceinline__ void store_record(float *base, const Own own, float rho, float ux, float uy, float uz, float Pi_xx, float Pi_yy,
                                             float Pi_zz, float Pi_xy, float Pi_yz, float Pi_zx, float one_m_omega)
{
    // own.cell4 = (lane + 64 z) * 4: plane z, lane
    char *plane = const_cast<char *>(record_plane(base, own.b, __builtin_amdgcn_readfirstlane((int)(own.cell4 >> 8))));
    float *q = reinterpret_cast<float *>(plane + (own.cell4 & 255u));
    const float v[R_COMP] = {rho, ux, uy, uz, Pi_xx, Pi_yy, Pi_zz, Pi_xy, Pi_yz, Pi_zx, one_m_omega};
#pragma unroll
    for (int c = 0; c < R_COMP; ++c) {
#ifdef LW_NT_STORES
        __builtin_nontemporal_store(v[c], q + c * 64);
#else
        q[c * 64] = v[c];
#endif
    }
}
// the three populations (cx = -1, 0, +1) that leave the record's cell in the (CY, CZ) row, into fs
template <int CY_, int CZ_>
__device__ __forceinline__ void record_row(float (&fs)[Q], const float (&r)[R_COMP])
{
    static_for<0, 3>([&](auto ic) {
        constexpr int k = decltype(ic)::value + 3 * (CY_ + 1) + 9 * (CZ_ + 1);
        fs[k] = collide_value<k>(r[R_RHO], r[R_UX], r[R_UY], r[R_UZ], r[R_PXX], r[R_PYY], r[R_PZZ], r[R_PXY], r[R_PYZ], r[R_PZX], r[R_OMO]);
    });
}
// The one population that crosses an x face out of the record's cell: cx = +1 (plus) or cx = -1. c * v for c = -1 is -v exactly, so
// the cx = -1 value is the cx = +1 expression on (-ux, -Pi_xy, -Pi_zx): the same operands meet in the same operations.
template <class DIRECTION>
__device__ __forceinline__ float record_face(const DIRECTION d, const float (&r)[R_COMP], bool plus)
{
    return collide_value(d, r[R_RHO], plus ? r[R_UX] : -r[R_UX], r[R_UY], r[R_UZ], r[R_PXX], r[R_PYY], r[R_PZZ],
                         plus ? r[R_PXY] : -r[R_PXY], r[R_PYZ], plus ? r[R_PZX] : -r[R_PZX], r[R_OMO]);
}

// Everything after the loads: moments, obstacle bounce, sponge, wall model, WALE, regularized collision, stores.
// reference src/physics_kernels.jl:144-354. fs = the 27 pulled populations, u?_? = previous-step velocity of the six
// face neighbours. Shared by the per-wave kernel and the x-run kernel.
// PACKED: the moment and stress sums and the 27 equilibria in packed FP32 (Chain2, equilibrium_value<f32x2>) - k_step_records. The f
// path's instantiations are memory-bound and sit at their register limit (96 VGPRs for 5 waves), where the pairs' alignment costs
// scratch or a wave (k_records_from_populations: 88 VGPRs, 5 waves instead of 6), so they instantiate the same expressions on float.
template <bool POST, bool WALL, bool REC_OUT = false, bool PACKED = false>
__device__ __forceinline__ void finish_cell(const SCParams &p, const int flags, const Own own, float (&fs)[Q],
                                            const float ux_E, const float uy_E, const float uz_E, const float ux_W, const float uy_W, const float uz_W,
                                            const float ux_N, const float uy_N, const float uz_N, const float ux_S, const float uy_S, const float uz_S,
                                            const float ux_T, const float uy_T, const float uz_T, const float ux_B, const float uy_B, const float uz_B)
{
    // moments in the reference's order: rho += f_k; j += f_k * c_k for k = 1..27. Four serial chains, each in k order, advanced as
    // the pairs (rho, jx) and (jy, jz). a - b and a + (-b) are the same operation, so a c = -1 term is the negated value.
    Chain2<PACKED> m_rx, m_yz;
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        constexpr int cx = CX(k), cy = CY(k), cz = CZ(k);
        const float val = fs[k];
        if constexpr (cx != 0) m_rx.add_both(val, cx > 0 ? val : -val);
        else m_rx.add_first(val);
        if constexpr (cy != 0 && cz != 0) m_yz.add_both(cy > 0 ? val : -val, cz > 0 ? val : -val);
        else if constexpr (cy != 0) m_yz.add_first(cy > 0 ? val : -val);
        else if constexpr (cz != 0) m_yz.add_second(cz > 0 ? val : -val);
    });
    float rho = m_rx.first();
    const float jx = m_rx.second(), jy = m_yz.first(), jz = m_yz.second();

    // the reference stores f_post_collision for every cell of a Bouzidi level (src/physics_kernels.jl:350-352); its only
    // reader is the Bouzidi kernel, at boundary cells and their link neighbours, so blocks that neither hold nor touch a
    // boundary cell skip the dead store (wave-uniform flag; 108 of 357 B per cell update)
    // Round 3: inside such a block only the x-rows (8 cells = one 32-B sector per population) that hold a Bouzidi cell or the
    // cell one step behind a link are stored (`post_rows`, one bit per row; the word is wave-uniform: block and plane are).
    bool store_post = false;
    if constexpr (POST) {
        if (flags & FLAG_STORE_POST) {
            store_post = true;
            if (p.post_rows) {
                const int zu = __builtin_amdgcn_readfirstlane((int)(own.cell4 >> 8));
                const uint32_t w = p.post_rows[(size_t)own.b * 2 + (zu >> 2)];
                store_post = ((w >> ((zu & 3) * 8 + ((own.cell4 >> 5) & 7))) & 1u) != 0;
            }
        }
    }
    // ---- obstacle cell: full-way bounce-back of the pulled set, reference :154-166 ----
    bool is_obs = false;
    if (flags & FLAG_HAS_OBSTACLE) is_obs = p.obstacle[(size_t)own.b * CELLS + (own.cell4 >> 2)] != 0;
    if (is_obs) {
        st_f32(p.vel_out, own.b, V_BLOCK_BYTES, own.cell4, 0.0f);
        st_f32(p.vel_out, own.b, V_BLOCK_BYTES, COMP_BYTES + own.cell4, 0.0f);
        st_f32(p.vel_out, own.b, V_BLOCK_BYTES, 2 * COMP_BYTES + own.cell4, 0.0f);
        if (p.rho_old_save) st_f32(p.rho_old_save, own.b, S_BLOCK_BYTES, own.cell4, ld_own(p.rho, own.b, S_BLOCK_BYTES, own.cell4));
        if (p.store_rho) st_f32(p.rho, own.b, S_BLOCK_BYTES, own.cell4, 1.0f);
        static_for<0, Q>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const float f_coll = fs[OPP(k)];
            st_f32(p.f_out, own.b, F_BLOCK_BYTES, k * COMP_BYTES + own.cell4, f_coll);
            if constexpr (POST) { if (store_post) st_f32(p.f_post, own.b, F_BLOCK_BYTES, k * COMP_BYTES + own.cell4, f_coll); }
        });
        return;
    }

    // ---- macroscopic moments, reference :172-176 ----
    rho = jl_max(rho, 0.01f);
    const float inv_rho = 1.0f / rho;
    float ux = jx * inv_rho, uy = jy * inv_rho, uz = jz * inv_rho;

    // ---- sponge, reference :181-199 ----
    if (flags & FLAG_HAS_SPONGE) {
        const float sp = ld_own(p.sponge, own.b, S_BLOCK_BYTES, own.cell4);
        if (sp > 0.0f) {
            const float rho_target = 1.0f, ux_target = p.u_inlet;
            rho = rho * (1.0f - sp) + rho_target * sp;
            ux = ux * (1.0f - sp) + ux_target * sp;
            uy = uy * (1.0f - sp);
            uz = uz * (1.0f - sp);
            if (p.sponge_blend == 1) {
                static_for<0, Q>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    const float feq_target = calculate_equilibrium(rho_target, ux_target, 0.0f, 0.0f, WEIGHT(k),
                                                                   (float)CX(k), (float)CY(k), (float)CZ(k));
                    fs[k] = fs[k] * (1.0f - sp) + feq_target * sp;
                });
            }
        }
    }

    // ---- wall-model force, reference :202-241 ----
    float Fx = 0.0f, Fy = 0.0f, Fz = 0.0f;
    float ux_eq = ux, uy_eq = uy, uz_eq = uz;          // u + 0.5 F / rho with F = 0
    if constexpr (WALL) {
        if (flags & FLAG_HAS_NEAR_WALL) {
            const float u_mag = sqrtf(ux * ux + uy * uy + uz * uz);
            const float force_mag = wall_model_force_mag(ld_own(p.wall_dist, own.b, S_BLOCK_BYTES, own.cell4), p.tau, rho, u_mag);
            if (force_mag >= 0.0f) {
                Fx = -force_mag * ux / u_mag;
                Fy = -force_mag * uy / u_mag;
                Fz = -force_mag * uz / u_mag;
            }
        }
        ux_eq = ux + 0.5f * Fx * inv_rho;
        uy_eq = uy + 0.5f * Fy * inv_rho;
        uz_eq = uz + 0.5f * Fz * inv_rho;
    }
    const float usq_eq = ux_eq * ux_eq + uy_eq * uy_eq + uz_eq * uz_eq;

    if constexpr (!REC_OUT) {
        st_f32(p.vel_out, own.b, V_BLOCK_BYTES, own.cell4, ux);
        st_f32(p.vel_out, own.b, V_BLOCK_BYTES, COMP_BYTES + own.cell4, uy);
        st_f32(p.vel_out, own.b, V_BLOCK_BYTES, 2 * COMP_BYTES + own.cell4, uz);
        if (p.rho_old_save) st_f32(p.rho_old_save, own.b, S_BLOCK_BYTES, own.cell4, ld_own(p.rho, own.b, S_BLOCK_BYTES, own.cell4));
        if (p.store_rho) st_f32(p.rho, own.b, S_BLOCK_BYTES, own.cell4, rho);
    }

    // ---- WALE eddy viscosity (wale_state) from the previous step's velocity, reference :251-300 ----
    const float g11 = 0.5f * (ux_E - ux_W), g12 = 0.5f * (ux_N - ux_S), g13 = 0.5f * (ux_T - ux_B);
    const float g21 = 0.5f * (uy_E - uy_W), g22 = 0.5f * (uy_N - uy_S), g23 = 0.5f * (uy_T - uy_B);
    const float g31 = 0.5f * (uz_E - uz_W), g32 = 0.5f * (uz_N - uz_S), g33 = 0.5f * (uz_T - uz_B);

    const float nu_eddy = wale_state(g11, g12, g13, g21, g22, g23, g31, g32, g33, p.c_wale, p.nu_bg).nu_eddy;
    const float tau_turb = p.tau + nu_eddy * 3.0f;
    const float omega = 1.0f / jl_max(tau_turb, 0.500001f);

    // ---- non-equilibrium stress, reference :305-322 ----
    // Six serial chains in k order, advanced as the pairs (Pi_xx, Pi_xy), (Pi_yy, Pi_yz), (Pi_zz, Pi_zx): the second of a pair takes a
    // term only where the first does, and it is the same f_neq up to the sign.
    // PACKED: directions k and 26 - k share the weight and have opposite c, so their two equilibria are evaluated at once, at k < 13, on
    // (cu, -cu), and f_neq of 26 - k waits in fs for its turn. c_opp . u negates every term of c_k . u, and rounding is symmetric in
    // sign, so it is -cu - except that a sum that cancels is +0 either way, where -cu is -0; 1 + 3 cu and 4.5 cu cu are the same
    // bits for either zero.
    Chain2<PACKED> P_x, P_y, P_z;
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value, ko = OPP(k);
        constexpr int cx = CX(k), cy = CY(k), cz = CZ(k);
        float f_neq;
        if constexpr (PACKED && k < ko) {
            const float cu = cdot<k>(ux_eq, uy_eq, uz_eq);
            const f32x2 both = f32x2{fs[k], fs[ko]} - equilibrium_value<f32x2>(rho, WEIGHT(k), f32x2{cu, -cu}, usq_eq);
            f_neq = both.x;
            fs[ko] = both.y;
        } else if constexpr (PACKED && k > ko) {
            f_neq = fs[k];
        } else {
            f_neq = fs[k] - equilibrium_value<float>(rho, WEIGHT(k), cdot<k>(ux_eq, uy_eq, uz_eq), usq_eq);
        }
        if constexpr (cx * cy != 0) P_x.add_both(f_neq, cx * cy > 0 ? f_neq : -f_neq);
        else if constexpr (cx != 0) P_x.add_first(f_neq);
        if constexpr (cy * cz != 0) P_y.add_both(f_neq, cy * cz > 0 ? f_neq : -f_neq);
        else if constexpr (cy != 0) P_y.add_first(f_neq);
        if constexpr (cz * cx != 0) P_z.add_both(f_neq, cz * cx > 0 ? f_neq : -f_neq);
        else if constexpr (cz != 0) P_z.add_first(f_neq);
    });
    const float Pi_xx = P_x.first(), Pi_xy = P_x.second(), Pi_yy = P_y.first(), Pi_yz = P_y.second(), Pi_zz = P_z.first(), Pi_zx = P_z.second();

    // ---- regularized collision + write, reference :324-354 ----
    const float one_m_omega = 1.0f - omega;
    const float one_m_half_omega = 1.0f - 0.5f * omega;
    if constexpr (REC_OUT) {      // eligible levels only (no wall model: u_eq = u is the stored velocity too), see "Record step"
        store_record(p.rec_out, own, rho, ux_eq, uy_eq, uz_eq, Pi_xx, Pi_yy, Pi_zz, Pi_xy, Pi_yz, Pi_zx, one_m_omega);
        return;
    }
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        float f_coll = collide_value<k>(rho, ux_eq, uy_eq, uz_eq, Pi_xx, Pi_yy, Pi_zz, Pi_xy, Pi_yz, Pi_zx, one_m_omega);
        if constexpr (WALL) {
            constexpr float w_k = WEIGHT(k);
            constexpr float cx_f = (float)CX(k), cy_f = (float)CY(k), cz_f = (float)CZ(k);
            const float cu = cdot<k>(ux_eq, uy_eq, uz_eq);
            const float force_term = (w_k * 3.0f) * ((cx_f - ux + 3.0f * cu * cx_f) * Fx + (cy_f - uy + 3.0f * cu * cy_f) * Fy +
                                                     (cz_f - uz + 3.0f * cu * cz_f) * Fz);
            f_coll = f_coll + one_m_half_omega * force_term;
        }
        if constexpr (POST) { if (store_post) st_f32(p.f_post, own.b, F_BLOCK_BYTES, k * COMP_BYTES + own.cell4, f_coll); }
        st_f32(p.f_out, own.b, F_BLOCK_BYTES, k * COMP_BYTES + own.cell4, f_coll);
    });
}

// The density finish_cell would have stored for this cell, and nothing else: the same sums in the same order (reference
// src/physics_kernels.jl:144-148, :154-158 obstacle, :172 clamp, :181-186 sponge). Used to produce `rho` on demand after a
// step that skipped the store.
__device__ __forceinline__ void finish_rho_only(const SCParams &p, const int flags, const Own own, const float (&fs)[Q])
{
    float rho = 0.0f;
    static_for<0, Q>([&](auto kc) { rho += fs[decltype(kc)::value]; });
    bool is_obs = false;
    if (flags & FLAG_HAS_OBSTACLE) is_obs = p.obstacle[(size_t)own.b * CELLS + (own.cell4 >> 2)] != 0;
    if (is_obs) { st_f32(p.rho, own.b, S_BLOCK_BYTES, own.cell4, 1.0f); return; }
    rho = jl_max(rho, 0.01f);
    if (flags & FLAG_HAS_SPONGE) {
        const float sp = ld_own(p.sponge, own.b, S_BLOCK_BYTES, own.cell4);
        if (sp > 0.0f) rho = rho * (1.0f - sp) + 1.0f * sp;
    }
    st_f32(p.rho, own.b, S_BLOCK_BYTES, own.cell4, rho);
}

// Lanes whose source block is missing: the domain-edge chain of reference src/physics_kernels.jl:88-140 (1-based global
// coords) decides what replaces the pulled value - inlet / outlet equilibrium, mirror of the own cell, the coarse->fine
// interface value, or the weight. Runs after all loads were issued (the lane read a valid dummy address meanwhile).
__device__ __forceinline__ void patch_missing_sources(const SCParams &p, const int32_t *__restrict__ meta, const NeighbourIds &nbr,
                                                      const LanePos &l, const int z, const Own own, float (&fs)[Q])
{
    const int gx = (meta[NBR_BX] - 1) * BS + l.x + 1, gy = (meta[NBR_BY] - 1) * BS + l.y + 1, gz = (meta[NBR_BZ] - 1) * BS + z + 1;
    const float *iface_own = p.is_level_1 == 0 ? p.f_iface + (size_t)meta[NBR_GBI] * CELLS + (own.cell4 >> 2) : nullptr;
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        constexpr int cx = CX(k), cy = CY(k), cz = CZ(k);
        if constexpr (k != 13) {
            if (source_block<k>(nbr, l) < 0) {
                const int src_gx = gx - cx, src_gy = gy - cy, src_gz = gz - cz;
                const bool is_inlet = src_gx < 1, is_outlet = src_gx > p.nx_g;
                const bool is_y_min = src_gy < 1, is_y_max = src_gy > p.ny_g;
                const bool is_z_min = src_gz < 1, is_z_max = src_gz > p.nz_g;
                float val;
                if (is_inlet) {
                    const float noise = p.inlet_turbulence > 0.0f
                                            ? gradient_noise(gy, gz, p.seed, 1234) * p.inlet_turbulence * p.u_inlet
                                            : 0.0f;
                    const float u_inst = p.u_inlet + noise;
                    val = edge_equilibrium<k>(u_inst);
                } else if (is_outlet) {
                    val = edge_equilibrium<k>(p.u_inlet);
                } else if (is_y_min && p.is_symmetric == 1) {
                    val = ld_own(p.f_in, own.b, F_BLOCK_BYTES, MIRROR_Y(k) * COMP_BYTES + own.cell4);
                } else if (is_y_min || is_y_max) {
                    val = ld_own(p.f_in, own.b, F_BLOCK_BYTES, MIRROR_Y(k) * COMP_BYTES + own.cell4);
                } else if (is_z_min || is_z_max) {
                    val = ld_own(p.f_in, own.b, F_BLOCK_BYTES, MIRROR_Z(k) * COMP_BYTES + own.cell4);
                } else if (p.is_level_1 == 0) {
                    // value computed by k_interface_links for exactly this (cell, k) link (same function, same inputs)
                    val = iface_own[(size_t)k * p.n_iface_blocks * CELLS];
                } else {
                    val = WEIGHT(k);
                }
                fs[k] = val;
            }
        }
    });
}

// ---- the stream-collide kernel --------------------------------------------------------------------------------
// GENERAL: blocks with a missing neighbour (domain edge / refinement interface); POST: also store f_post_collision
// (level has Bouzidi cells); WALL: wall model active; RHO_ONLY: reproduce an elided rho; WIDE: 64-bit per-lane addresses.
// Workgroup = the SAME z-plane of NW x-consecutive blocks (host guarantees: items 0..NW-1 of the group are valid,
// share z, item i+1 is the +x neighbour of item i, all blocks have their 26 neighbours). Every global access is an
// aligned 256-B plane row set (x unshifted; the y / z shift only changes the row / plane, i.e. stays 16-B aligned);
// the +-1 shift in x is a DPP lane shift, and the face column each block needs from its x neighbour is handed over
// between neighbouring waves through 24 x 8 floats of LDS. Only the two outer faces of the run are still read as
// strided columns from global memory. Measured motivation: DESIGN.md section 3.1 (the x-face column and the 4-byte
// misalignment are what separate the pull from an aligned copy on MI355X).
__device__ __forceinline__ float dpp_from_lower_lane(float v)   // lane i <- lane i-1 inside 16-lane rows (row_shr:1)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x111, 0xF, 0xF, false));
}
__device__ __forceinline__ float dpp_from_upper_lane(float v)   // lane i <- lane i+1 inside 16-lane rows (row_shl:1)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x101, 0xF, 0xF, false));
}
// slot of population k in the exchange buffer: cx=+1 populations publish their x=7 column in slots 0..8,
// cx=-1 populations their x=0 column in slots 9..17 (k = (cx+1) + 3 j, j = 0..8)
__host__ __device__ constexpr int XSLOT(int k) { return CX(k) == 1 ? k / 3 : 9 + k / 3; }

// work item of the x-run kernel: (block << 3) | z in the low bits, plus which of its lateral faces are served by the
// neighbouring wave of the workgroup (LDS) rather than by a strided column read from global memory
constexpr int ITEM_LINK_W = 1 << 30;   // wave - 1 of this workgroup holds the -x neighbour block, same plane
constexpr int ITEM_LINK_E = 1 << 29;   // wave + 1 holds the +x neighbour block, same plane
constexpr int ITEM_ID_MASK = (1 << 29) - 1;

#ifndef LW_MIN_WAVES
#define LW_MIN_WAVES 5      // waves per SIMD the register allocator must leave room for (96 VGPRs)
#endif
// The body of the kernel; REC_OUT: the result is stored as 11-float records (k_records_from_populations), not as f, vel and rho.
template <int NW, bool GENERAL, bool POST, bool WALL, bool RHO_ONLY, bool WIDE, bool REC_OUT>
__device__ __forceinline__ void stream_collide_xrun(const SCParams p)
{
    __shared__ float xch[NW][24][8];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int raw = p.items[blockIdx.x * NW + wave];
    const bool active = raw >= 0;                             // -1 = idle wave (padding); it still meets the barrier
    const int item = active ? (raw & ITEM_ID_MASK) : 0;
    const int b = item >> 3;
    const int z = item & 7;
    const int lane = threadIdx.x & 63;
    LanePos l;
    l.x = lane & 7; l.y = lane >> 3;
    l.x0 = l.x == 0; l.x7 = l.x == 7; l.y0 = l.y == 0; l.y7 = l.y == 7;
    const int32_t *__restrict__ meta = p.meta + (size_t)b * NBR_STRIDE;
    const int flags = meta[NBR_FLAGS];
    const NeighbourIds nbr = load_neighbour_ids(meta, z);
    const Own own{b, (uint32_t)((l.x + 8 * l.y + 64 * z) * 4)};
    // wave-uniform: a run may be shorter than the workgroup (several short runs, or single blocks, share one)
    const bool first = !active || (raw & ITEM_LINK_W) == 0, last = !active || (raw & ITEM_LINK_E) == 0;
    float fs[Q];
    float halo[Q];                                            // outer-face column (run ends only)
    float uc[3], uT[3], uB[3], uy_edge[3], ux_edge_lo[3], ux_edge_hi[3];
    if (active) {
    // ---- aligned loads: value of population k at (x, y - cy, z - cz) ----
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        constexpr int cx = CX(k), cy = CY(k), g = 1 - CZ(k);
        const bool yo = cy == 1 ? l.y0 : (cy == -1 ? l.y7 : false);
        const int c00 = nbr.id[g][4], cY = nbr.id[g][4 - 3 * cy];
        int sel = cy != 0 ? (yo ? cY : c00) : c00;
        if constexpr (GENERAL) sel = sel >= 0 ? sel : b;      // missing block: in-bounds dummy, patched after the exchange
        const uint32_t rowz = (uint32_t)(k * COMP_BYTES) + (uint32_t)((8 * ((l.y - cy) & 7)) * 4) + (uint32_t)(nbr.zs[g] * 256);
        // populations with cy = 0: the block is wave-uniform (SGPR base) and the two lines of this plane are read by this wave
        // only (the x neighbours get their column through LDS, nobody shifts rows)
        if constexpr (cy == 0) fs[k] = ld_f32<true>(p.f_in, sel, F_BLOCK_BYTES, rowz + (uint32_t)(l.x * 4));
        else fs[k] = ld_f32<WIDE>(p.f_in, sel, F_BLOCK_BYTES, rowz + (uint32_t)(l.x * 4));
        halo[k] = 0.0f;
        if constexpr (cx != 0) {
            if (cx == 1 ? first : last) {                     // the run's outer face: strided column of the x / xy neighbour
                const int cX = nbr.id[g][4 - cx], cXY = nbr.id[g][4 - cx - 3 * cy];
                int selx = cy != 0 ? (yo ? cXY : cX) : cX;
                if constexpr (GENERAL) selx = selx >= 0 ? selx : b;
                if (cx == 1 ? l.x0 : l.x7)
                    halo[k] = ld_f32<(cy == 0) || WIDE>(p.f_in, selx, F_BLOCK_BYTES, rowz + (uint32_t)((cx == 1 ? 7 : 0) * 4));
            }
        }
    });
    // previous-step velocity: centre plane, planes z+-1 (aligned), y-face rows and outer x-face columns (masked)
    if constexpr (!RHO_ONLY) {
        int bT = z == 7 ? nbr.id[2][4] : b, bB = z == 0 ? nbr.id[0][4] : b;      // wave-uniform
        const uint32_t xy = (uint32_t)((l.x + 8 * l.y) * 4);
        uint32_t inT = xy + (uint32_t)(((z + 1) & 7) * 256), inB = xy + (uint32_t)(((z - 1) & 7) * 256);
        // lanes y==0 fetch row 7 of the -y neighbour, lanes y==7 row 0 of the +y neighbour (one masked load per component)
        int by_ = l.y0 ? nbr.id[1][4 - 3] : nbr.id[1][4 + 3];
        uint32_t inY = (uint32_t)((l.x + 8 * (l.y0 ? 7 : 0) + 64 * z) * 4);
        int bXlo = nbr.id[1][4 - 1], bXhi = nbr.id[1][4 + 1];                    // wave-uniform
        uint32_t inXlo = (uint32_t)((7 + 8 * l.y + 64 * z) * 4), inXhi = (uint32_t)((0 + 8 * l.y + 64 * z) * 4);
        if constexpr (GENERAL) {      // missing neighbour block -> the cell's own velocity (reference src/physics_utils.jl:45-70)
            if (bT < 0) { bT = b; inT = own.cell4; }
            if (bB < 0) { bB = b; inB = own.cell4; }
            if (by_ < 0) { by_ = b; inY = own.cell4; }
            if (bXlo < 0) { bXlo = b; inXlo = own.cell4; }
            if (bXhi < 0) { bXhi = b; inXhi = own.cell4; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t cb = (uint32_t)c * COMP_BYTES;
            uc[c] = ld_own(p.vel_in, b, V_BLOCK_BYTES, cb + own.cell4);
            uT[c] = ld_own(p.vel_in, bT, V_BLOCK_BYTES, cb + inT);
            uB[c] = ld_own(p.vel_in, bB, V_BLOCK_BYTES, cb + inB);
            uy_edge[c] = 0.0f; ux_edge_lo[c] = 0.0f; ux_edge_hi[c] = 0.0f;
            if (l.y0 || l.y7) uy_edge[c] = ld_f32<WIDE>(p.vel_in, by_, V_BLOCK_BYTES, cb + inY);
            if (first) { if (l.x0) ux_edge_lo[c] = ld_own(p.vel_in, bXlo, V_BLOCK_BYTES, cb + inXlo); }
            if (last) { if (l.x7) ux_edge_hi[c] = ld_own(p.vel_in, bXhi, V_BLOCK_BYTES, cb + inXhi); }
        }
    }

    // ---- publish the face columns the neighbouring waves need ----
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        constexpr int cx = CX(k);
        if constexpr (cx == 1) { if (l.x7) xch[wave][XSLOT(k)][l.y] = fs[k]; }
        if constexpr (cx == -1) { if (l.x0) xch[wave][XSLOT(k)][l.y] = fs[k]; }
    });
    if constexpr (!RHO_ONLY) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (l.x7) xch[wave][18 + c][l.y] = uc[c];
            if (l.x0) xch[wave][21 + c][l.y] = uc[c];
        }
    }
    }   // if (active)
    __syncthreads();
    if (!active) return;
    const int wlo = first ? 0 : wave - 1, whi = last ? NW - 1 : wave + 1;
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        constexpr int cx = CX(k);
        if constexpr (cx == 1) {
            const float inner = dpp_from_lower_lane(fs[k]);
            const float edge = first ? halo[k] : xch[wlo][XSLOT(k)][l.y];
            fs[k] = l.x0 ? edge : inner;
        }
        if constexpr (cx == -1) {
            const float inner = dpp_from_upper_lane(fs[k]);
            const float edge = last ? halo[k] : xch[whi][XSLOT(k)][l.y];
            fs[k] = l.x7 ? edge : inner;
        }
    });
    // merged launches run all-neighbour blocks through the GENERAL instantiation too: nothing to patch there (wave-uniform flag)
    const bool needs_patch = GENERAL && (flags & FLAG_ALL_NEIGHBOURS) == 0;
    if constexpr (RHO_ONLY) {
        if constexpr (GENERAL) { if (needs_patch) patch_missing_sources(p, meta, nbr, l, z, own, fs); }
        finish_rho_only(p, flags, own, fs);
        return;
    }
    float uE[3], uW[3], uN[3], uS[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float e_edge = last ? ux_edge_hi[c] : xch[whi][21 + c][l.y];
        const float w_edge = first ? ux_edge_lo[c] : xch[wlo][18 + c][l.y];
        // cross-lane reads must execute with ALL lanes active: never inside an arm of ?: (that arm runs under a
        // reduced EXEC mask and a DPP read of an inactive lane silently keeps the old value)
        const float e_in = dpp_from_upper_lane(uc[c]), w_in = dpp_from_lower_lane(uc[c]);
        uE[c] = l.x7 ? e_edge : e_in;
        uW[c] = l.x0 ? w_edge : w_in;
        const float n_in = __shfl_down(uc[c], 8, 64), s_in = __shfl_up(uc[c], 8, 64);
        uN[c] = l.y7 ? uy_edge[c] : n_in;
        uS[c] = l.y0 ? uy_edge[c] : s_in;
    }
    if constexpr (GENERAL) { if (needs_patch) patch_missing_sources(p, meta, nbr, l, z, own, fs); }
    finish_cell<POST, WALL, REC_OUT>(p, flags, own, fs, uE[0], uE[1], uE[2], uW[0], uW[1], uW[2], uN[0], uN[1], uN[2], uS[0], uS[1], uS[2],
                                     uT[0], uT[1], uT[2], uB[0], uB[1], uB[2]);
}
template <int NW, bool GENERAL, bool POST, bool WALL, bool RHO_ONLY = false, bool WIDE = false>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu((WIDE && GENERAL) ? LW_MIN_WAVES - 1 : LW_MIN_WAVES))) void k_stream_collide_xrun(const SCParams p)
{
    stream_collide_xrun<NW, GENERAL, POST, WALL, RHO_ONLY, WIDE, false>(p);
}
// The first record step after populations were written (upload, an f-path step, k_materialise): the f path's pull on an eligible
// level, stored as records. "Record step" below.
template <int NW, bool WIDE>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(LW_MIN_WAVES))) void k_records_from_populations(const SCParams p)
{
    stream_collide_xrun<NW, false, false, false, false, WIDE, true>(p);
}

// ---- Record step: the kernel that reads records ----
// Same mapping, same work list and same LDS / DPP x exchange as k_stream_collide_xrun<NW, false, false, false>; what differs is
// where the 27 pulled populations come from. Lane (x, y) of plane z loads the 9 records at (x, y - cy, z - cz) - the y shift is
// addressing, as for populations: row (y - cy) & 7 of the own block or of the y neighbour - and evaluates collide_value for the 3
// x directions of each; the x shift then is the usual lane shift plus face column. The previous step's velocity of the y and z
// neighbours is in those same records (the centre one, cy = +-1 and cz = +-1), so no velocity is loaded and nothing is shuffled
// in y. At the outer faces of a run the wave loads the x neighbour's 9 records of its face column, spread over all 64 lanes, and
// evaluates the one population of each that crosses the face.
// Order: pull, publish (the face columns the neighbouring waves need, into LDS), the outer faces' loads, workgroup barrier, the
// outer faces' evaluation, x shift, finish_cell. Only the first and last wave of a run have outer faces (~150 instructions); what
// they make is written and read by that one wave, so it needs no workgroup barrier - in front of the barrier it kept the waves in
// between waiting, behind it the four waves reach the barrier together, and the loads, issued in front of it once the pull's
// registers are free, are in flight while the wave waits (profiles/paired_pull_vs_parent.txt).
// Every block is all-neighbour, carries no obstacle / sponge / near-wall flag, and the level has no
// wall model (the host's eligibility rule), so this is finish_cell<false, false> with flags = 0 - the f path's arithmetic, operation
// by operation - and the result is stored as a record again.
#ifndef LW_REC_WAVES
#define LW_REC_WAVES 4      // waves per SIMD the register allocator must leave room for: 128 VGPRs, 125 used (at 96 the allocator spills)
#endif
#ifndef LW_REC_AHEAD
#define LW_REC_AHEAD 3      // records whose loads are in flight while one is evaluated (11 registers each)
#endif
template <int NW, bool WIDE>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(LW_REC_WAVES))) void k_step_records(const SCParams p)
{
    __shared__ float xch[NW][24][8];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int raw = p.items[blockIdx.x * NW + wave];
    const bool active = raw >= 0;
    const int item = active ? (raw & ITEM_ID_MASK) : 0;
    const int b = item >> 3;
    const int z = item & 7;
    const int lane = threadIdx.x & 63;
    LanePos l;
    l.x = lane & 7; l.y = lane >> 3;
    l.x0 = l.x == 0; l.x7 = l.x == 7; l.y0 = l.y == 0; l.y7 = l.y == 7;
    const int32_t *__restrict__ meta = p.meta + (size_t)b * NBR_STRIDE;
    const NeighbourIds nbr = load_neighbour_ids(meta, z);
    const Own own{b, (uint32_t)((l.x + 8 * l.y + 64 * z) * 4)};
    const bool first = !active || (raw & ITEM_LINK_W) == 0, last = !active || (raw & ITEM_LINK_E) == 0;
    // what crosses the run's outer faces, per wave and side (0: from -x, 1: from +x): slots 0..8 the population of row
    // j = (cy+1) + 3 (cz+1), 9..11 the velocity. Through LDS, not registers: they would be held across the whole pull otherwise.
    __shared__ float xedge[NW][2][12][8];
    float fs[Q];
    float uc[3], uT[3], uB[3], uN[3], uS[3];
    // ---- the run's outer faces: the first wave needs column 7 of the -x neighbour, the last wave column 0 of the +x neighbour (a
    // lone block both): per face 9 records x 8 rows, of each the one population that crosses the face ----
    // Spread over the whole wave: lane (x', y) takes row y of record j = x', j = (cy+1) + 3 (cz+1) = 0..7, so (cy, cz), the source
    // plane and the block - the x neighbour, or for the row that leaves it in y the y neighbour of the x neighbour - are per-lane
    // selections among wave-uniform values, and the population is collide_value in its per-lane form (DirLaneFace). 11 loads and one
    // evaluation with 64 lanes active, where eight lanes used to walk through nine records. Loads (face_load, ninth_load: in front of
    // the workgroup barrier) and evaluation (face_eval, ninth_eval: behind it) are separate steps; rf and r9 carry the records across.
    auto face_dir = [&](int &cy, int &cz) {
        const int j = l.x;
        const int jz = (j >= 3 ? 1 : 0) + (j >= 6 ? 1 : 0);         // j / 3
        cy = j - 3 * jz - 1;
        cz = jz - 1;
    };
    float rf[2][R_COMP], r9[R_COMP];
    auto face_load = [&](auto sc) {
        constexpr int side = decltype(sc)::value;                     // 0: from -x, 1: from +x
        constexpr int jx = side == 0 ? 4 - 1 : 4 + 1;
        int cy, cz;
        face_dir(cy, cz);
        const int g = 1 - cz;
        auto by_g = [&](int v0, int v1, int v2) { return g == 0 ? v0 : (g == 1 ? v1 : v2); };      // values, not lvalues (see source_block)
        const int bX = by_g(nbr.id[0][jx], nbr.id[1][jx], nbr.id[2][jx]);
        const int bXlo = by_g(nbr.id[0][jx - 3], nbr.id[1][jx - 3], nbr.id[2][jx - 3]);            // its -y neighbour: cy = +1 rows of y = 0
        const int bXhi = by_g(nbr.id[0][jx + 3], nbr.id[1][jx + 3], nbr.id[2][jx + 3]);            // its +y neighbour: cy = -1 rows of y = 7
        const int blk = (cy == 1 && l.y0) ? bXlo : ((cy == -1 && l.y7) ? bXhi : bX);
        const int zsrc = by_g(nbr.zs[0], nbr.zs[1], nbr.zs[2]);
        load_record_at(rf[side], p.rec_in, record_offset<WIDE>(blk, zsrc) + (uint32_t)(((side == 0 ? 7 : 0) + 8 * ((l.y - cy) & 7)) * 4));
    };
    auto face_eval = [&](auto sc) {
        constexpr int side = decltype(sc)::value;
        int cy, cz;
        face_dir(cy, cz);
        const int j = l.x;
        const float(&r)[R_COMP] = rf[side];
        float(&mine)[12][8] = xedge[wave][side];
        mine[j][l.y] = record_face(DirLaneFace{cy, cz}, r, side == 0);
        if (j == 4) { mine[9][l.y] = r[R_UX]; mine[10][l.y] = r[R_UY]; mine[11][l.y] = r[R_UZ]; }      // cy = cz = 0: the face neighbour itself
    };
    // the ninth record (cy = cz = +1), in the lanes of the face column: four wave-uniform offsets, one chosen per lane; both sides of
    // a lone block in one masked evaluation
    const bool ninth = (first && l.x0) || (last && l.x7);
    auto ninth_load = [&]() {
        constexpr int cy = 1, g = 0;
        const int wX = nbr.id[g][4 - 1], wXY = nbr.id[g][4 - 1 - 3 * cy], eX = nbr.id[g][4 + 1], eXY = nbr.id[g][4 + 1 - 3 * cy];
        const auto oW = record_offset<WIDE>(wX, nbr.zs[g]), oWY = record_offset<WIDE>(wXY, nbr.zs[g]);
        const auto oE = record_offset<WIDE>(eX, nbr.zs[g]), oEY = record_offset<WIDE>(eXY, nbr.zs[g]);
        const auto off = l.x0 ? (l.y0 ? oWY : oW) : (l.y0 ? oEY : oE);
        load_record_at(r9, p.rec_in, off + (uint32_t)(((l.x0 ? 7 : 0) + 8 * ((l.y - cy) & 7)) * 4));
    };
    auto ninth_eval = [&]() { xedge[wave][l.x0 ? 0 : 1][8][l.y] = record_face(DirConst<DIR(1, 1, 1)>{}, r9, l.x0); };
    auto outer_face_loads = [&]() {
        if (first) face_load(std::integral_constant<int, 0>{});
        if (last) face_load(std::integral_constant<int, 1>{});
        if (ninth) ninth_load();
    };
    auto outer_face_evals = [&]() {
        if (first) face_eval(std::integral_constant<int, 0>{});
        if (last) face_eval(std::integral_constant<int, 1>{});
        if (ninth) ninth_eval();
    };
    if (active) {
    // ---- the 9 records at (x, y - cy, z - cz) ----
    {
        float r[9][R_COMP];
        auto load_pulled = [&](auto jc) {
            constexpr int j = decltype(jc)::value;
            constexpr int cy = j % 3 - 1, g = 1 - (j / 3 - 1);
            const uint32_t lane4 = (uint32_t)((l.x + 8 * ((l.y - cy) & 7)) * 4);
            if constexpr (cy == 0) {       // the block is wave-uniform: scalar base, the lane's offset inside the plane
                load_record(r[j], record_plane(p.rec_in, nbr.id[g][4], nbr.zs[g]), lane4);
            } else {
                const bool yo = cy == 1 ? l.y0 : l.y7;
                const auto o0 = record_offset<WIDE>(nbr.id[g][4], nbr.zs[g]), oY = record_offset<WIDE>(nbr.id[g][4 - 3 * cy], nbr.zs[g]);
                load_record_at(r[j], p.rec_in, (yo ? oY : o0) + lane4);
            }
        };
        static_for<0, LW_REC_AHEAD>(load_pulled);
        static_for<0, 9>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            constexpr int cy = j % 3 - 1, cz = j / 3 - 1;
            if constexpr (j + LW_REC_AHEAD < 9) load_pulled(std::integral_constant<int, j + LW_REC_AHEAD>{});
            __builtin_amdgcn_sched_barrier(0);
            const float(&q)[R_COMP] = r[j];
            record_row<cy, cz>(fs, q);
            if constexpr (cy == 0 && cz == 0) { uc[0] = q[R_UX]; uc[1] = q[R_UY]; uc[2] = q[R_UZ]; }
            if constexpr (cy == 0 && cz == 1) { uB[0] = q[R_UX]; uB[1] = q[R_UY]; uB[2] = q[R_UZ]; }
            if constexpr (cy == 0 && cz == -1) { uT[0] = q[R_UX]; uT[1] = q[R_UY]; uT[2] = q[R_UZ]; }
            if constexpr (cy == 1 && cz == 0) { uS[0] = q[R_UX]; uS[1] = q[R_UY]; uS[2] = q[R_UZ]; }
            if constexpr (cy == -1 && cz == 0) { uN[0] = q[R_UX]; uN[1] = q[R_UY]; uN[2] = q[R_UZ]; }
            __builtin_amdgcn_sched_barrier(0);
        });
    }
    // ---- publish the face columns the neighbouring waves need ----
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        constexpr int cx = CX(k);
        if constexpr (cx == 1) { if (l.x7) xch[wave][XSLOT(k)][l.y] = fs[k]; }
        if constexpr (cx == -1) { if (l.x0) xch[wave][XSLOT(k)][l.y] = fs[k]; }
    });
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (l.x7) xch[wave][18 + c][l.y] = uc[c];
        if (l.x0) xch[wave][21 + c][l.y] = uc[c];
    }
    outer_face_loads();      // 11 registers a side and 11 for the ninth record, live only after the pull's records are dead
    }   // if (active)
    __syncthreads();
    if (!active) return;
    outer_face_evals();
    // xedge is written and read by different lanes of this one wave: the LDS serves a wave's accesses in order, so wavefront-scope
    // release / acquire (no instruction) and a barrier the compiler moves nothing across are all the reads below need - no second
    // workgroup barrier
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int wlo = first ? 0 : wave - 1, whi = last ? NW - 1 : wave + 1;
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        constexpr int cx = CX(k);
        if constexpr (cx == 1) {
            const float inner = dpp_from_lower_lane(fs[k]);
            const float edge = first ? xedge[wave][0][k / 3][l.y] : xch[wlo][XSLOT(k)][l.y];
            fs[k] = l.x0 ? edge : inner;
        }
        if constexpr (cx == -1) {
            const float inner = dpp_from_upper_lane(fs[k]);
            const float edge = last ? xedge[wave][1][k / 3][l.y] : xch[whi][XSLOT(k)][l.y];
            fs[k] = l.x7 ? edge : inner;
        }
    });
    float uE[3], uW[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float e_edge = last ? xedge[wave][1][9 + c][l.y] : xch[whi][21 + c][l.y];
        const float w_edge = first ? xedge[wave][0][9 + c][l.y] : xch[wlo][18 + c][l.y];
        const float e_in = dpp_from_upper_lane(uc[c]), w_in = dpp_from_lower_lane(uc[c]);   // all lanes active, see k_stream_collide_xrun
        uE[c] = l.x7 ? e_edge : e_in;
        uW[c] = l.x0 ? w_edge : w_in;
    }
    finish_cell<false, false, true, true>(p, 0, own, fs, uE[0], uE[1], uE[2], uW[0], uW[1], uW[2], uN[0], uN[1], uN[2], uS[0], uS[1], uS[2],
                                    uT[0], uT[1], uT[2], uB[0], uB[1], uB[2]);
}

// A record back into what the f path keeps: the cell's 27 post-collision populations (un-streamed, as f_out holds them), its velocity
// and its density. One thread per cell; the same collide_value the f path's writer evaluates, so the same bits.
__global__ __launch_bounds__(256) void k_materialise(const SCParams p, int64_t n_cells)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cells) return;
    const int b = (int)(i >> 9);
    const uint32_t cell = (uint32_t)(i & 511);
    float r[R_COMP];
    load_record(r, record_plane(p.rec_in, b, (int)(cell >> 6)), (cell & 63u) * 4);
    const Own own{b, cell * 4};
    st_f32(p.vel_out, b, V_BLOCK_BYTES, own.cell4, r[R_UX]);
    st_f32(p.vel_out, b, V_BLOCK_BYTES, COMP_BYTES + own.cell4, r[R_UY]);
    st_f32(p.vel_out, b, V_BLOCK_BYTES, 2 * COMP_BYTES + own.cell4, r[R_UZ]);
    if (p.rho) st_f32(p.rho, b, S_BLOCK_BYTES, own.cell4, r[R_RHO]);      // null: a later step's density is the level's rho
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        st_f32(p.f_out, b, F_BLOCK_BYTES, k * COMP_BYTES + own.cell4,
               collide_value<k>(r[R_RHO], r[R_UX], r[R_UY], r[R_UZ], r[R_PXX], r[R_PYY], r[R_PZZ], r[R_PXY], r[R_PYZ], r[R_PZX], r[R_OMO]));
    });
}

// ---- coarse -> fine interface pass (reference src/physics_kernels.jl:122-137 + src/physics_interpolation.jl) ----
// The reference evaluates interpolate_with_rescaling inline, for the few lanes of a refinement-edge block whose source
// block is missing. Done that way on a 64-wide wavefront it is 27 divergent call sites at ~12 % lane utilisation and
// took 86 % of the GPU time of a 3-level case (profiles/r01_ball1m_kernel_stats_before_interface_pass.csv). The links
// that need it are a static property of the level (topology + global box), so the host lists them once and two small
// kernels evaluate them (per source cell, then per link); the stream-collide kernel loads the value. Same expressions on
// the same inputs as the reference's interpolate_with_rescaling: bit-identical.
__device__ __forceinline__ float weight_rt(int k)
{
    const int cx = k % 3 - 1, cy = (k / 3) % 3 - 1, cz = k / 9 - 1;
    const int d2 = cx * cx + cy * cy + cz * cz;
    return d2 == 0 ? WEIGHT(13) : d2 == 1 ? WEIGHT(12) : d2 == 2 ? WEIGHT(9) : WEIGHT(0);
}

// The two sub-steps a child level takes per parent step see the SAME parent buffers and differ only in the temporal
// weight (0.0 then 0.5, reference src/solver_control.jl:63-83). With TWO = true both values are produced from one set of
// loads (second outputs mac2 / f_iface2 for weight tw2); the second sub-step then skips the pass.
struct InterfaceArgs {
    const int4 *corners;      // 2 per source: parent-cell offsets of the 8 stencil corners, -1 = absent (static, host)
    const float4 *weights;    // per source: wx, wy, wz (static)
    float4 *mac, *mac2;       // per source: interpolated rho, ux, uy, uz for tw / tw2
    const int4 *links;        // per link: (block << 9) | cell, (gbi << 5) | k, source index
    float *f_iface2;
    float tw2;
    int n_sources, n_links;
};

__device__ __forceinline__ float blend_in_time(bool blend, float v_old, float v_new, float tw)
{
    return blend ? v_old * (1.0f - tw) + v_new * tw : v_new;      // reference src/physics_interpolation.jl:83-93
}

// Pass 1, one thread per SOURCE cell (a fine-grid cell just outside this level's blocks): trilinear rho / u of
// reference src/physics_interpolation.jl:64-124 - the same for every population pulled from that cell, so evaluated once.
template <bool TWO>
__global__ __launch_bounds__(256) void k_interface_sources(const SCParams p, const InterfaceArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_sources) return;
    const int4 c0 = a.corners[2 * i], c1 = a.corners[2 * i + 1];
    const int cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float4 w = a.weights[i];
    const float tw = p.temporal_weight, tw2 = a.tw2;
    const bool blend = p.use_temporal == 1 && tw < 0.99f, blend2 = TWO && p.use_temporal == 1 && tw2 < 0.99f;
    float v1[4][8], v2[4][8];                                  // rho, ux, uy, uz at the 8 corners
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        v1[0][n] = 1.0f; v1[1][n] = 0.0f; v1[2][n] = 0.0f; v1[3][n] = 0.0f;      // (w_k, 1, 0, 0, 0, false) default
        v2[0][n] = 1.0f; v2[1][n] = 0.0f; v2[2][n] = 0.0f; v2[3][n] = 0.0f;
        if (cc[n] >= 0) {
            const int c = cc[n];                                 // parent cell: block * 512 + cell
            const size_t cv = (size_t)(c >> 9) * (3 * CELLS) + (c & 511);      // component 0 of the block-major velocity array
            const float vn[4] = {p.prho_new[c], p.pvel_new[cv], p.pvel_new[cv + CELLS], p.pvel_new[cv + 2 * CELLS]};
            float vo[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (blend || blend2) { vo[0] = p.prho_old[c]; vo[1] = p.pvel_old[cv]; vo[2] = p.pvel_old[cv + CELLS]; vo[3] = p.pvel_old[cv + 2 * CELLS]; }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v1[q][n] = blend_in_time(blend, vo[q], vn[q], tw);
                if (TWO) v2[q][n] = blend_in_time(blend2, vo[q], vn[q], tw2);
            }
        }
    }
    // invalid corners take corner 000's tuple (which may itself be the default), reference :100-107
#pragma unroll
    for (int n = 1; n < 8; ++n)
        if (cc[n] < 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) { v1[q][n] = v1[q][0]; v2[q][n] = v2[q][0]; }
        }
#define LW_TL(v, q) trilin(v[q][0], v[q][1], v[q][2], v[q][3], v[q][4], v[q][5], v[q][6], v[q][7], w.x, w.y, w.z)
    a.mac[i] = make_float4(LW_TL(v1, 0), LW_TL(v1, 1), LW_TL(v1, 2), LW_TL(v1, 3));
    if (TWO) a.mac2[i] = make_float4(LW_TL(v2, 0), LW_TL(v2, 1), LW_TL(v2, 2), LW_TL(v2, 3));
#undef LW_TL
}

// Pass 2, one thread per LINK (cell, population k): f_k interpolated over the same 8 corners, equilibrium from pass 1's
// moments, non-equilibrium rescaled (reference src/physics_interpolation.jl:110-135). Expression by expression the
// reference's interpolate_with_rescaling, so the value is bit-identical to the inline call.
template <bool TWO>
__global__ __launch_bounds__(256) void k_interface_links(const SCParams p, const InterfaceArgs a)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n_links) return;
    const int4 l = a.links[j];
    const int cell = l.x & 511, k = l.y & 31, gbi = l.y >> 5, src = l.z;
    const int4 c0 = a.corners[2 * src], c1 = a.corners[2 * src + 1];
    const int cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float4 w = a.weights[src];
    const float tw = p.temporal_weight, tw2 = a.tw2;
    const bool blend = p.use_temporal == 1 && tw < 0.99f, blend2 = TWO && p.use_temporal == 1 && tw2 < 0.99f;
    const float w_k = weight_rt(k);
    float fc[8], fc2[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        fc[n] = w_k; fc2[n] = w_k;
        if (cc[n] >= 0) {
            const size_t cf = ((size_t)(cc[n] >> 9) * Q + k) * CELLS + (cc[n] & 511);      // population k of the parent cell
            const float fn = p.pf_new[cf];
            float fo = 0.0f;
            if (blend || blend2) fo = p.pf_old[cf];
            fc[n] = blend_in_time(blend, fo, fn, tw);
            if (TWO) fc2[n] = blend_in_time(blend2, fo, fn, tw2);
        }
    }
#pragma unroll
    for (int n = 1; n < 8; ++n)
        if (cc[n] < 0) { fc[n] = fc[0]; fc2[n] = fc2[0]; }
    const float cxf = (float)(k % 3 - 1), cyf = (float)((k / 3) % 3 - 1), czf = (float)(k / 9 - 1);
    const float tau_c = p.tau_parent - 0.5f, tau_f = p.tau - 0.5f;
    const float scale = tau_c > 1.0e-6f ? jl_clamp(tau_f / tau_c, 0.01f, 100.0f) : 1.0f;
    const size_t out = ((size_t)k * p.n_iface_blocks + gbi) * CELLS + cell;
    {
        const float4 m = a.mac[src];
        const float f_int = trilin(fc[0], fc[1], fc[2], fc[3], fc[4], fc[5], fc[6], fc[7], w.x, w.y, w.z);
        const float feq_int = calculate_equilibrium(m.x, m.y, m.z, m.w, w_k, cxf, cyf, czf);
        const float f_neq = f_int - feq_int;
        p.f_iface[out] = feq_int + f_neq * scale;
    }
    if (TWO) {
        const float4 m = a.mac2[src];
        const float f_int = trilin(fc2[0], fc2[1], fc2[2], fc2[3], fc2[4], fc2[5], fc2[6], fc2[7], w.x, w.y, w.z);
        const float feq_int = calculate_equilibrium(m.x, m.y, m.z, m.w, w_k, cxf, cyf, czf);
        const float f_neq = f_int - feq_int;
        a.f_iface2[out] = feq_int + f_neq * scale;
    }
}

// (Round 3 tried both passes in ONE kernel, one thread per source cell walking the populations pulled from it: nine dependent rounds
// of loads per thread at 100 VGPRs - 97 us against 42 + 22 on the wing. profiles/r03_interface_pass_fused_experiment.txt; not kept.)

// ---- Bouzidi correction, reference src/bouzidi_kernel.jl:13-92 ----
struct BouzidiParams {
    float *f_out;
    const float *f_post;
    const _Float16 *q_map;
    const int32_t *cell_block;   // 0-based
    const int8_t *cell_x, *cell_y, *cell_z;   // 0-based
    const int32_t *meta;
    int32_t n_cells;
    float q_min;
    const int4 *links;           // compact list of the links with q > 0, everything static about one link in one record:
                                 // (block * 512 + cell, k, bits of q as Float32, block' * 512 + cell' of the cell one step behind or -1)
    int32_t n_links;
};

// one thread per (listed cell, link k): the 27 links of a cell are independent (each writes its own f_out[cell][opp k]
// and reads only f_post_collision), so spreading them over lanes changes nothing but the latency that is exposed
// With a link list (the q map is static, so the host lists the links with q > 0 once) the threads that would only find
// q = 0 - four out of five - do not exist; q_min is still applied here, per call.
__global__ __launch_bounds__(256) void k_bouzidi(const BouzidiParams p)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    auto at = [](int blk, int kk, int c) { return ((size_t)blk * Q + kk) * CELLS + c; };      // block-major f / q map
    if (p.links) {
        // the link list: one dependent load less than reading q from the map and the neighbour block from the table -
        // record -> two independent f_post loads -> store (this kernel is a few microseconds of pure latency, four times per coarse step)
        if (i >= p.n_links) return;
        const int4 l = p.links[i];
        const float q = __int_as_float(l.z);                  // (float)q_map[...]: Float16 -> Float32 is exact, done on the host
        if (!(q > p.q_min && q <= 1.0f)) return;
        const int b = l.x >> 9, cell = l.x & 511, k = l.y, opp_k = 26 - k;
        const float f_k = p.f_post[at(b, k, cell)];
        if (q < 0.5f) {
            const float f_ff = l.w >= 0 ? p.f_post[at(l.w >> 9, k, l.w & 511)] : f_k;
            const float coeff1 = 2.0f * q;
            p.f_out[at(b, opp_k, cell)] = coeff1 * f_k + (1.0f - coeff1) * f_ff;
        } else {
            const float f_opp_post = p.f_post[at(b, opp_k, cell)];
            const float inv_2q = 1.0f / (2.0f * q);
            const float coeff2 = (2.0f * q - 1.0f) * inv_2q;
            p.f_out[at(b, opp_k, cell)] = inv_2q * f_k + coeff2 * f_opp_post;
        }
        return;
    }
    int b, x, y, z, k;
    {
        if (i >= p.n_cells * Q) return;
        const int c = i / Q;
        k = i - c * Q;
        b = p.cell_block[c];
        x = p.cell_x[c]; y = p.cell_y[c]; z = p.cell_z[c];
    }
    const int opp_k = 26 - k;
    const int cell = x + 8 * y + 64 * z;
    const float q = (float)p.q_map[at(b, k, cell)];
    if (q > p.q_min && q <= 1.0f) {
        const float f_k = p.f_post[at(b, k, cell)];
        if (q < 0.5f) {
            const int nx = x + (opp_k % 3 - 1), ny = y + ((opp_k / 3) % 3 - 1), nz = z + (opp_k / 9 - 1);
            float f_ff = f_k;
            if (nx >= 0 && nx < BS && ny >= 0 && ny < BS && nz >= 0 && nz < BS) {
                f_ff = p.f_post[at(b, k, nx + 8 * ny + 64 * nz)];
            } else {
                const int ox = nx < 0 ? -1 : (nx >= BS ? 1 : 0);
                const int oy = ny < 0 ? -1 : (ny >= BS ? 1 : 0);
                const int oz = nz < 0 ? -1 : (nz >= BS ? 1 : 0);
                const int nbb = p.meta[(int64_t)b * NBR_STRIDE + DIR(ox, oy, oz)];
                if (nbb >= 0) f_ff = p.f_post[at(nbb, k, (nx & 7) + 8 * (ny & 7) + 64 * (nz & 7))];
            }
            const float coeff1 = 2.0f * q;
            p.f_out[at(b, opp_k, cell)] = coeff1 * f_k + (1.0f - coeff1) * f_ff;
        } else {
            const float f_opp_post = p.f_post[at(b, opp_k, cell)];
            const float inv_2q = 1.0f / (2.0f * q);
            const float coeff2 = (2.0f * q - 1.0f) * inv_2q;
            p.f_out[at(b, opp_k, cell)] = inv_2q * f_k + coeff2 * f_opp_post;
        }
    }
}

// ---- init_eq!, reference src/main.jl:109-124 ----
__global__ void k_fill_weights(float *f, int64_t n_cells)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // cell index: block * 512 + cell
    if (i >= n_cells) return;
    float *q = f + (i >> 9) * (int64_t)(Q * CELLS) + (i & 511);
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        q[k * CELLS] = WEIGHT(k);
    });
}
__global__ void k_fill(float *a, int64_t n, float v)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = v;
}

// ---- surface stresses, reference src/forces/surface.jl:32-76 (compute_stress_from_cell) and :138-266 (map_stresses_kernel!) ----
struct SurfaceParams {
    const float *rho, *vel;
    const uint8_t *obstacle;
    const int32_t *block_pointer;    // [gdx,gdy,gdz] 1-based, 0 = absent
    int32_t gdx, gdy, gdz, n_tri, radius;
    float dx, tau, off_x, off_y, off_z, pressure_scale, stress_scale;
    const float *centers, *normals;  // [n_tri * 3]
    float *p, *tx, *ty, *tz;         // [n_tri]
};

// compute_stress_from_cell (src/forces/surface.jl:32-96) of one winning cell: pressure and wall shear stress, Float32 [Pa]
__device__ __forceinline__ void wall_stress(float rho, float ux, float uy, float uz, float nx, float ny, float nz, float wd, float tau,
                                            float pressure_scale, float stress_scale, float &p, float &sx, float &sy, float &sz)
{
    const float wall_dist = fmaxf(wd, 0.5f);
    p = ((rho - 1.0f) / 3.0f) * pressure_scale;
    const float udn = ux * nx + uy * ny + uz * nz;
    const float utx = ux - udn * nx, uty = uy - udn * ny, utz = uz - udn * nz;
    const float umag = sqrtf(utx * utx + uty * uty + utz * utz);
    const float nu_lat = (tau - 0.5f) / 3.0f;
    sx = 0.0f; sy = 0.0f; sz = 0.0f;
    if (umag > 1.0e-10f && wall_dist > 0.01f) {
        const float tmag = (rho * nu_lat * umag / wall_dist) * stress_scale;
        sx = (utx / umag) * tmag; sy = (uty / umag) * tmag; sz = (utz / umag) * tmag;
    }
}

__global__ __launch_bounds__(128) void k_map_stresses(const SurfaceParams s)
{
    const int i = blockIdx.x * 128 + threadIdx.x;
    if (i >= s.n_tri) return;
    const float tx = s.centers[3 * i] + s.off_x, ty = s.centers[3 * i + 1] + s.off_y, tz = s.centers[3 * i + 2] + s.off_z;
    const float nx = s.normals[3 * i], ny = s.normals[3 * i + 1], nz = s.normals[3 * i + 2];
    const int g_x = (int)floorf(tx / s.dx) + 1, g_y = (int)floorf(ty / s.dx) + 1, g_z = (int)floorf(tz / s.dx) + 1;
    float best_d = 1.0e10f, best_rho = 1.0f, ux = 0.0f, uy = 0.0f, uz = 0.0f, best_wd = 0.5f;
    bool found = false;
    for (int radius = 0; radius <= s.radius; ++radius) {
        if (found && radius > 1) break;
        for (int dz = -radius; dz <= radius; ++dz)
            for (int dy = -radius; dy <= radius; ++dy)
                for (int dx = -radius; dx <= radius; ++dx) {
                    if (radius > 0 && !(abs(dx) == radius || abs(dy) == radius || abs(dz) == radius)) continue;   // the shell only
                    const int cgx = g_x + dx, cgy = g_y + dy, cgz = g_z + dz;
                    if (cgx < 1 || cgy < 1 || cgz < 1) continue;
                    const int bx = (cgx - 1) / BS + 1, by = (cgy - 1) / BS + 1, bz = (cgz - 1) / BS + 1;
                    if (bx > s.gdx || by > s.gdy || bz > s.gdz) continue;
                    const int32_t b = s.block_pointer[(size_t)(bx - 1) + (size_t)s.gdx * ((size_t)(by - 1) + (size_t)s.gdy * (bz - 1))];
                    if (b <= 0) continue;
                    const int64_t c = (int64_t)((cgx - 1) % BS) + 8 * ((cgy - 1) % BS) + 64 * ((cgz - 1) % BS) + 512 * (int64_t)(b - 1);
                    if (s.obstacle[c]) continue;
                    const float ccx = ((float)cgx - 0.5f) * s.dx, ccy = ((float)cgy - 0.5f) * s.dx, ccz = ((float)cgz - 0.5f) * s.dx;
                    const float ex = tx - ccx, ey = ty - ccy, ez = tz - ccz;
                    const float d2 = ex * ex + ey * ey + ez * ez;
                    if (d2 < best_d) {
                        best_d = d2;
                        best_rho = s.rho[c];
                        const int64_t cv = (c >> 9) * (int64_t)(3 * CELLS) + (c & 511);      // block-major velocity
                        ux = s.vel[cv]; uy = s.vel[cv + CELLS]; uz = s.vel[cv + 2 * CELLS];
                        best_wd = sqrtf(d2) / s.dx;
                        found = true;
                    }
                }
    }
    float p = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (found) wall_stress(best_rho, ux, uy, uz, nx, ny, nz, best_wd, s.tau, s.pressure_scale, s.stress_scale, p, sx, sy, sz);
    s.p[i] = p; s.tx[i] = sx; s.ty[i] = sy; s.tz[i] = sz;
}

// ---- surface statistics (ludwig_surface_stats_*; no reference counterpart) ----
// One lane per triangle of the set. cell[i] = internal block * 512 + (x + 8 y + 64 z) of the triangle's nearest fluid cell (-1: none
// found); rec = [4][n] floats: wall distance (lattice units), normal x, y, z. rho: [block][512], vel: [block][3][512] floats
// (block-major). p, tau are wall_stress's float32 values (those of k_map_stresses), |tau| = sqrt((tx tx + ty ty) + tz tz) in float32;
// sums = [SURFACE_STAT_COMPONENTS][n] doubles, S_p, S_pp, S_tx, S_ty, S_tz, S_|tau|, S_|tau|^2: each a plain sequential addition in
// sample order, and a product of two floats is exact in double. A triangle is owned by its lane: no atomics, deterministic.
// Launch-bound for any real mesh: about 150 B per triangle (20 B record, 16 B gathered, 56 B of sums read and written).
constexpr int SURFACE_STAT_COMPONENTS = 7;
__global__ __launch_bounds__(256) void k_accumulate_surface_stats(double *__restrict__ sums, const int32_t *__restrict__ cell,
                                                                  const float *__restrict__ rec, int n, const float *__restrict__ rho,
                                                                  const float *__restrict__ vel, float tau, float pressure_scale,
                                                                  float stress_scale)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int32_t c = cell[i];
    float p = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (c >= 0) {
        const int64_t b = c >> 9, cc = c & 511;
        const float *v = vel + b * (3 * CELLS) + cc;
        wall_stress(rho[c], v[0], v[CELLS], v[2 * CELLS], rec[n + i], rec[2 * n + i], rec[3 * n + i], rec[i], tau, pressure_scale,
                    stress_scale, p, sx, sy, sz);
    }
    const float mag = sqrtf((sx * sx + sy * sy) + sz * sz);
    const double dp = p, dm = mag;
    const int64_t N = n;
    double *s = sums + i;
    s[0] += dp;
    s[N] += dp * dp;
    s[2 * N] += (double)sx;
    s[3 * N] += (double)sy;
    s[4 * N] += (double)sz;
    s[5 * N] += dm;
    s[6 * N] += dm * dm;
}

// ---- compute_flow_stats, reference src/diagnostics.jl:56-94 (CUDA branch): minimum of rho over non-obstacle cells ----
// Finite rho is > 0 (clamped at 0.01, obstacle cells hold 1), so the IEEE bit pattern orders like the value and an integer
// atomicMin does the job; a minimum does not depend on the order of its operands: identical to any host reduction.
// A diverged run holds NaN, and the reference's minimum() PROPAGATES it (Julia's min, like jl_max above) where fminf and the
// integer compare would silently drop it: a NaN in any counted cell raises out[1], and the caller reports NaN.
__global__ __launch_bounds__(256) void k_rho_min(const float *__restrict__ rho, const uint8_t *__restrict__ obstacle, int64_t n, int *__restrict__ out)
{
    float m = __int_as_float(0x7f800000);   // +inf
    bool nan = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        if (!obstacle[i]) {
            const float v = rho[i];
            nan = nan || v != v;
            m = fminf(m, v);
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
    const bool any_nan = __any(nan);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(out, __float_as_int(m));
        if (any_nan) atomicOr(out + 1, 1);
    }
}

// ---- time-averaged statistics (ludwig_level_stats_*; no reference counterpart) ----
// stats: [internal block][STAT_COMPONENTS][512] doubles - S_rho, S_u (x, y, z), S_uu (xx, yy, zz, xy, yz, xz: VTK's symmetric-tensor
// order); rho: [block][512], vel: [block][3][512] floats (block-major). One workgroup per owned block, two x-consecutive cells per
// lane: a wave covers two 8x8 planes of a component, 512 B of floats in and 1 KiB of doubles in and out, contiguous. Every sum is a
// plain sequential addition per cell in sample order; a product of two floats is exact in double, so contraction cannot change a bit.
constexpr int STAT_COMPONENTS = 10;
__global__ __launch_bounds__(256) void k_accumulate_stats(double *__restrict__ stats, const float *__restrict__ rho,
                                                          const float *__restrict__ vel)
{
    const int64_t b = blockIdx.x;
    const int c = 2 * (int)threadIdx.x;
    const float2 r = *(const float2 *)(rho + b * CELLS + c);
    const float *v = vel + b * 3 * CELLS + c;
    const float2 vx = *(const float2 *)v, vy = *(const float2 *)(v + CELLS), vz = *(const float2 *)(v + 2 * CELLS);
    const double x0 = vx.x, x1 = vx.y, y0 = vy.x, y1 = vy.y, z0 = vz.x, z1 = vz.y;
    const double add[STAT_COMPONENTS][2] = {{r.x, r.y}, {x0, x1}, {y0, y1}, {z0, z1}, {x0 * x0, x1 * x1}, {y0 * y0, y1 * y1},
                                            {z0 * z0, z1 * z1}, {x0 * y0, x1 * y1}, {y0 * z0, y1 * z1}, {x0 * z0, x1 * z1}};
    double *s = stats + b * STAT_COMPONENTS * CELLS + c;
#pragma unroll
    for (int m = 0; m < STAT_COMPONENTS; ++m) {
        double2 *p = (double2 *)(s + m * CELLS);
        double2 a = *p;
        a.x += add[m][0];
        a.y += add[m][1];
        *p = a;
    }
}

// ---- Fourier modes (ludwig_modes_*; no reference counterpart) ----
// sums: [internal block][M][MODE_FIELDS][512] doubles - per weight column m the running sums of rho, ux, uy, uz times w[m]; w: the M
// weights of this sample, one row of the set's table; rho, vel as k_accumulate_stats reads them, and the same shape: one workgroup per
// owned block, two x-consecutive cells per lane, float2 loads, double2 read-modify-writes, no LDS, no atomics. w is read with an index
// every lane shares, so a row sits in scalar registers. Per sum one float64 multiply and then one float64 add (the library is built
// without contraction): acc = acc + w[m] * double(v) on the host reproduces every bit, non-finite values included.
constexpr int MODE_FIELDS = 4;
constexpr int MODE_MAX_COLUMNS = 33;
__global__ __launch_bounds__(256) void k_accumulate_modes(double *__restrict__ sums, const double *__restrict__ w, int n_columns,
                                                          const float *__restrict__ rho, const float *__restrict__ vel)
{
    const int64_t b = blockIdx.x;
    const int c = 2 * (int)threadIdx.x;
    const float2 r = *(const float2 *)(rho + b * CELLS + c);
    const float *v = vel + b * 3 * CELLS + c;
    const float2 vx = *(const float2 *)v, vy = *(const float2 *)(v + CELLS), vz = *(const float2 *)(v + 2 * CELLS);
    const double val[MODE_FIELDS][2] = {{r.x, r.y}, {vx.x, vx.y}, {vy.x, vy.y}, {vz.x, vz.y}};
    double *s = sums + b * n_columns * (MODE_FIELDS * CELLS) + c;
    for (int m = 0; m < n_columns; ++m) {
        const double wm = w[m];
#pragma unroll
        for (int q = 0; q < MODE_FIELDS; ++q) {
            double2 *p = (double2 *)(s + (m * MODE_FIELDS + q) * CELLS);
            double2 a = *p;
            a.x = a.x + wm * val[q][0];
            a.y = a.y + wm * val[q][1];
            *p = a;
        }
    }
}

// ---- velocity-gradient fields (ludwig_level_gradient_fields_*; the gradient is compute_velocity_gradients, reference
// src/physics_utils.jl:44-82, the one the WALE model uses) ----
// out: [internal block][GRAD_COMPONENTS][512] floats - vorticity x, y, z and Q; vel: [block][3][512]; obstacle: [block][512].
// One workgroup per owned block. The block and a one-cell face halo of every component are staged in LDS, [3][10][10][10] floats
// (12 KB): a face neighbour block that exists gives its adjacent layer, a missing one (meta entry -1: domain edge, level boundary)
// the block's own edge layer, which is get_velocity_neighbor's own-value rule. Then two x-consecutive cells per lane, float2 stores.
// g_ij = du_i/dx_j = (0.5 (u_i(+e_j) - u_i(-e_j))) scale, the WALE expression times one multiply; vorticity = (g32 - g23,
// g13 - g31, g21 - g12), Q = -0.5 (((g11^2 + g22^2) + g33^2) + 2 ((g12 g21 + g13 g31) + g23 g32)) = (|Omega|^2 - |S|^2) / 2,
// in exactly this order (-ffp-contract=off: a float32 restatement reproduces every bit). Obstacle cells get 0.
constexpr int GRAD_COMPONENTS = 4;
constexpr int GRAD_TILE = 10;                                   // 8 cells + one halo layer on each side
constexpr int GRAD_HALO = 6 * 3 * 64;                           // faces x components x cells of a face layer
// The staging both stencil kernels share (k_velocity_gradient_fields, k_subgrid): block b of `vel` and its face halo into u, lane t's two
// cells at `at` and `at + 1`. The caller synchronizes the workgroup before it reads u.
__device__ __forceinline__ void stage_velocity_tile(float *u, const float *__restrict__ vel, const int32_t *__restrict__ meta,
                                                    const int64_t b, const int t, const int c, const int at)
{
    constexpr int T = GRAD_TILE, T2 = GRAD_TILE * GRAD_TILE, T3 = T2 * GRAD_TILE;
    const float *vb = vel + b * 3 * CELLS;
    float2 own[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) own[k] = *(const float2 *)(vb + k * CELLS + c);
    // face layers: element i = (face * 3 + component) * 64 + cell of the face; 64 consecutive i are one wave, so face and component
    // are wave-uniform and the neighbour id is a scalar load. Faces: -x, +x, -y, +y, -z, +z.
    float h[5];
    int hat[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int i = t + 256 * r;
        hat[r] = -1;
        h[r] = 0.0f;
        if (i < GRAD_HALO) {
            const int g = __builtin_amdgcn_readfirstlane(i >> 6);
            const int face = g / 3, k = g - 3 * face, axis = face >> 1, up = face & 1;
            const int p = i & 7, q = (i >> 3) & 7;
            const int step = axis == 0 ? 1 : (axis == 1 ? 3 : 9);
            const int nb = meta[b * NBR_STRIDE + 13 + (up ? step : -step)];
            const int src = nb >= 0 ? (up ? 0 : 7) : (up ? 7 : 0);   // the neighbour's adjacent layer, or the block's own edge layer
            const int dst = up ? T - 1 : 0;
            int sx, sy, sz, lx, ly, lz;
            if (axis == 0) { sx = src; sy = p; sz = q; lx = dst; ly = p + 1; lz = q + 1; }
            else if (axis == 1) { sx = p; sy = src; sz = q; lx = p + 1; ly = dst; lz = q + 1; }
            else { sx = p; sy = q; sz = src; lx = p + 1; ly = q + 1; lz = dst; }
            const int64_t sb = nb >= 0 ? (int64_t)nb : b;
            h[r] = vel[(sb * 3 + k) * CELLS + sx + 8 * sy + 64 * sz];
            hat[r] = k * T3 + lx + T * ly + T2 * lz;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u[k * T3 + at] = own[k].x;
        u[k * T3 + at + 1] = own[k].y;
    }
#pragma unroll
    for (int r = 0; r < 5; ++r)
        if (hat[r] >= 0) u[hat[r]] = h[r];
}

// vorticity and Q of g[i][j] = du_i/dx_j in the order stated above: ONE source for k_velocity_gradient_fields and k_slice_sample<true>
__device__ __forceinline__ void vorticity_q(float (&q)[GRAD_COMPONENTS], const float (&g)[3][3])
{
    q[0] = g[2][1] - g[1][2];
    q[1] = g[0][2] - g[2][0];
    q[2] = g[1][0] - g[0][1];
    q[3] = -0.5f * (((g[0][0] * g[0][0] + g[1][1] * g[1][1]) + g[2][2] * g[2][2]) +
                    2.0f * ((g[0][1] * g[1][0] + g[0][2] * g[2][0]) + g[1][2] * g[2][1]));
}

__global__ __launch_bounds__(256) void k_velocity_gradient_fields(float *__restrict__ out, const float *__restrict__ vel,
                                                                  const uint8_t *__restrict__ obstacle,
                                                                  const int32_t *__restrict__ meta, float scale)
{
    constexpr int T = GRAD_TILE, T2 = GRAD_TILE * GRAD_TILE, T3 = T2 * GRAD_TILE;
    __shared__ float u[3 * T3];
    const int64_t b = blockIdx.x;
    const int t = (int)threadIdx.x;
    const int c = 2 * t, x = c & 7, y = (c >> 3) & 7, z = c >> 6;
    const int at = (x + 1) + T * (y + 1) + T2 * (z + 1);
    stage_velocity_tile(u, vel, meta, b, t, c, at);
    const uint8_t ob0 = obstacle[b * CELLS + c], ob1 = obstacle[b * CELLS + c + 1];
    __syncthreads();
    float res[GRAD_COMPONENTS][2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int a = at + s;
        constexpr int step[3] = {1, T, T2};
        float g[3][3], q[GRAD_COMPONENTS];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) g[i][j] = (0.5f * (u[i * T3 + a + step[j]] - u[i * T3 + a - step[j]])) * scale;
        vorticity_q(q, g);
        const bool solid = (s == 0 ? ob0 : ob1) != 0;
#pragma unroll
        for (int m = 0; m < GRAD_COMPONENTS; ++m) res[m][s] = solid ? 0.0f : q[m];
    }
    float *o = out + b * GRAD_COMPONENTS * CELLS + c;
#pragma unroll
    for (int m = 0; m < GRAD_COMPONENTS; ++m) *(float2 *)(o + m * CELLS) = make_float2(res[m][0], res[m][1]);
}

// ---- subgrid model (ludwig_level_subgrid_*; no reference counterpart for the output; the model is the step's, wale_state above) ----
// One workgroup per owned block, staged like k_velocity_gradient_fields (stage_velocity_tile), two x-consecutive cells per lane. The
// gradient is the step's, in lattice units with no scale: g_ij = 0.5f (u_i(+e_j) - u_i(-e_j)), a missing face neighbour block giving
// the cell's own value. Evaluated on the velocity sub-step t wrote, nu_eddy is therefore exactly the value sub-step t + 1 collides
// with (that step reads this buffer as vel_in). Obstacle cells take no part: 0 and code 0, +0.0 into the sums.
//   <SUBGRID_FIELDS> out: [internal block][2][512] floats - nu_eddy (after the floor) and the code as a float.
//   <SUBGRID_SUMS>   out: [internal block][3][512] doubles - S_nu += nu, S_nunu += nu nu, S_eps += nu s2 with nu, s2 widened first: a
//                    product of two floats is exact in double, every sum a plain sequential += per cell in sample order, no atomics.
constexpr int SUBGRID_FIELDS = 0, SUBGRID_SUMS = 1;
constexpr int SUBGRID_FIELD_COMPONENTS = 2, SUBGRID_SUM_COMPONENTS = 3;
template <int MODE>
__global__ __launch_bounds__(256) void k_subgrid(std::conditional_t<MODE == SUBGRID_SUMS, double, float> *__restrict__ out,
                                                 const float *__restrict__ vel, const uint8_t *__restrict__ obstacle,
                                                 const int32_t *__restrict__ meta, float c_wale, float nu_bg)
{
    constexpr int T = GRAD_TILE, T2 = GRAD_TILE * GRAD_TILE, T3 = T2 * GRAD_TILE;
    __shared__ float u[3 * T3];
    const int64_t b = blockIdx.x;
    const int t = (int)threadIdx.x;
    const int c = 2 * t, x = c & 7, y = (c >> 3) & 7, z = c >> 6;
    const int at = (x + 1) + T * (y + 1) + T2 * (z + 1);
    stage_velocity_tile(u, vel, meta, b, t, c, at);
    const uint8_t ob0 = obstacle[b * CELLS + c], ob1 = obstacle[b * CELLS + c + 1];
    __syncthreads();
    WaleState w[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int a = at + s;
        const float *ux = u, *uy = u + T3, *uz = u + 2 * T3;
        w[s] = wale_state(0.5f * (ux[a + 1] - ux[a - 1]), 0.5f * (ux[a + T] - ux[a - T]), 0.5f * (ux[a + T2] - ux[a - T2]),
                          0.5f * (uy[a + 1] - uy[a - 1]), 0.5f * (uy[a + T] - uy[a - T]), 0.5f * (uy[a + T2] - uy[a - T2]),
                          0.5f * (uz[a + 1] - uz[a - 1]), 0.5f * (uz[a + T] - uz[a - T]), 0.5f * (uz[a + T2] - uz[a - T2]), c_wale, nu_bg);
    }
    const bool solid0 = ob0 != 0, solid1 = ob1 != 0;
    if constexpr (MODE == SUBGRID_FIELDS) {
        float *o = out + b * SUBGRID_FIELD_COMPONENTS * CELLS + c;
        *(float2 *)o = make_float2(solid0 ? 0.0f : w[0].nu_eddy, solid1 ? 0.0f : w[1].nu_eddy);
        *(float2 *)(o + CELLS) = make_float2(solid0 ? 0.0f : (float)w[0].code, solid1 ? 0.0f : (float)w[1].code);
    } else {
        const double n0 = w[0].nu_eddy, n1 = w[1].nu_eddy, e0 = w[0].s2, e1 = w[1].s2;
        const double add[SUBGRID_SUM_COMPONENTS][2] = {{solid0 ? 0.0 : n0, solid1 ? 0.0 : n1},
                                                       {solid0 ? 0.0 : n0 * n0, solid1 ? 0.0 : n1 * n1},
                                                       {solid0 ? 0.0 : n0 * e0, solid1 ? 0.0 : n1 * e1}};
        double *sm = out + b * SUBGRID_SUM_COMPONENTS * CELLS + c;
#pragma unroll
        for (int m = 0; m < SUBGRID_SUM_COMPONENTS; ++m) {
            double2 *p = (double2 *)(sm + m * CELLS);
            double2 v = *p;
            v.x += add[m][0];
            v.y += add[m][1];
            *p = v;
        }
    }
}

// ---- probes (ludwig_probes_*; no reference counterpart) ----
// One lane per probe of one level. cell[8 p + c] = internal block * 512 + (x + 8 y + 64 z) of stencil corner c = dx + 2 dy + 4 dz;
// w[3 p + a] = the weights along x, y, z; col[p] = the probe's place in the set. rho: [block][512], vel: [block][3][512] floats
// (block-major). Trilinear in float32 in ONE fixed order - x first (corners 0-1, 2-3, 4-5, 6-7), then y, then z, every lerp
// (1 - w) a + w b - with -ffp-contract=off, so open_ludwig_amd/probes.py (trilinear) restates it bit for bit. out = the slot,
// [n_set][4]: rho, ux, uy, uz. Bounded by a launch latency, not by bandwidth: 128 B gathered per probe.
__device__ __forceinline__ float probe_lerp(float a, float b, float w) { return (1.0f - w) * a + w * b; }
// corner c = dx + 2 dy + 4 dz: x, then y, then z. ONE source for the probes, slices, flux planes and the renderer.
__device__ __forceinline__ float probe_trilinear(const float (&v)[8], float wx, float wy, float wz)
{
    const float x00 = probe_lerp(v[0], v[1], wx), x10 = probe_lerp(v[2], v[3], wx);
    const float x01 = probe_lerp(v[4], v[5], wx), x11 = probe_lerp(v[6], v[7], wx);
    const float y0 = probe_lerp(x00, x10, wy), y1 = probe_lerp(x01, x11, wy);
    return probe_lerp(y0, y1, wz);
}
// res = rho, ux, uy, uz at point p of a planned set: the eight corners cell[8 p ..] gathered, then probe_trilinear with w[3 p ..]
__device__ __forceinline__ void stencil_sample(float (&res)[4], int64_t p, const int32_t *__restrict__ cell, const float *__restrict__ w,
                                               const float *__restrict__ rho, const float *__restrict__ vel)
{
    int64_t e[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) e[c] = cell[8 * p + c];
    const float wx = w[3 * p], wy = w[3 * p + 1], wz = w[3 * p + 2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int64_t b = e[c] >> 9, cc = e[c] & 511;
            v[c] = k == 0 ? rho[e[c]] : vel[(b * 3 + (k - 1)) * CELLS + cc];
        }
        res[k] = probe_trilinear(v, wx, wy, wz);
    }
}

__global__ __launch_bounds__(64) void k_probe_sample(float *__restrict__ out, const int32_t *__restrict__ cell, const float *__restrict__ w,
                                                     const int32_t *__restrict__ col, int n, const float *__restrict__ rho,
                                                     const float *__restrict__ vel)
{
    const int p = (int)(blockIdx.x * 64 + threadIdx.x);
    if (p >= n) return;
    float res[4];
    stencil_sample(res, p, cell, w, rho, vel);
    *(float4 *)(out + 4 * (int64_t)col[p]) = make_float4(res[0], res[1], res[2], res[3]);
}

// ---- slices (ludwig_slices_*; no reference counterpart) ----
// One lane per point of one level; lanes run in the order of their base cells (the host sorts them), the output index is col[p].
// base[p] = internal block * 512 + (x + 8 y + 64 z) of the base cell; its block is OWNED, so its neighbour row is complete, and every
// cell the point reads - the 8 corners i0 + {0,1}^3 and their 6 face neighbours, i0 - 1 .. i0 + 2 per axis - lies in that block's
// 3 x 3 x 3 neighbourhood: slice_locate finds it through meta[base block][DIR] (-1: no block there). rep[p] bit c: corner c was
// replaced by the base cell (the probes' rule). w[3 p + a]: weights along x, y, z. Rows of out, [row][n_set]: rho, ux, uy, uz, |u|,
// and with GRAD vorticity x, y, z, Q. |u| = sqrt((ux^2 + uy^2) + uz^2) of the interpolated components. Vorticity and Q at a
// corner are k_velocity_gradient_fields' cell values, computed here from the same six neighbours (a missing neighbour block: the
// corner's own value) in the same expressions; the corners are fluid cells, so its obstacle rule never applies. Then the probes'
// trilinear (probe_lerp, x, y, z) of every quantity. -ffp-contract=off: open_ludwig_amd/slices.py restates it bit for bit.
constexpr int SLICE_ROWS_BASIC = 5, SLICE_ROWS_GRAD = 9;

__device__ __forceinline__ int64_t slice_locate(const int32_t *__restrict__ meta, int64_t b0, int x, int y, int z)
{
    // x, y, z relative to the base block's origin, -1 .. 9
    const int ox = x >> 3, oy = y >> 3, oz = z >> 3;   // arithmetic shift: -1, 0 or 1
    int64_t b = b0;
    if (ox | oy | oz) {
        b = meta[b0 * NBR_STRIDE + DIR(ox, oy, oz)];
        if (b < 0) return -1;
    }
    return b * CELLS + ((x & 7) + 8 * (y & 7) + 64 * (z & 7));
}

__device__ __forceinline__ float slice_vel(const float *__restrict__ vel, int64_t e, int k)
{
    return vel[((e >> 9) * 3 + k) * CELLS + (e & 511)];
}

template <bool GRAD>
__global__ __launch_bounds__(64) void k_slice_sample(float *__restrict__ out, int64_t n_set, const int32_t *__restrict__ base,
                                                     const float *__restrict__ w, const uint8_t *__restrict__ rep,
                                                     const int32_t *__restrict__ col, int n, const float *__restrict__ rho,
                                                     const float *__restrict__ vel, const int32_t *__restrict__ meta, float scale)
{
    const int p = (int)(blockIdx.x * 64 + threadIdx.x);
    if (p >= n) return;
    const int64_t e0 = base[p], b0 = e0 >> 9;
    const int x0 = (int)(e0 & 7), y0 = (int)((e0 >> 3) & 7), z0 = (int)((e0 >> 6) & 7);
    const unsigned r = rep[p];
    const float wx = w[3 * p], wy = w[3 * p + 1], wz = w[3 * p + 2];
    constexpr int NQ = GRAD ? 8 : 4;           // rho, ux, uy, uz (+ wx, wy, wz, Q) at the corners
    float v[NQ][8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool keep = !((r >> c) & 1u);
        const int cx = x0 + (keep ? (c & 1) : 0), cy = y0 + (keep ? ((c >> 1) & 1) : 0), cz = z0 + (keep ? (c >> 2) : 0);
        int64_t e = slice_locate(meta, b0, cx, cy, cz);
        if (e < 0) e = e0;                     // (the set's creation has checked that a kept corner exists)
        v[0][c] = rho[e];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[1 + k][c] = slice_vel(vel, e, k);
        if constexpr (GRAD) {
            float g[3][3];                     // g[i][j] = du_i/dx_j
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                int64_t hi = slice_locate(meta, b0, cx + (j == 0), cy + (j == 1), cz + (j == 2));
                int64_t lo = slice_locate(meta, b0, cx - (j == 0), cy - (j == 1), cz - (j == 2));
                if (hi < 0) hi = e;
                if (lo < 0) lo = e;
#pragma unroll
                for (int i = 0; i < 3; ++i) g[i][j] = (0.5f * (slice_vel(vel, hi, i) - slice_vel(vel, lo, i))) * scale;
            }
            float q[GRAD_COMPONENTS];
            vorticity_q(q, g);
#pragma unroll
            for (int m = 0; m < GRAD_COMPONENTS; ++m) v[4 + m][c] = q[m];
        }
    }
    float res[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) res[k] = probe_trilinear(v[k], wx, wy, wz);
    const int64_t o = col[p];
    out[o] = res[0];
    out[n_set + o] = res[1];
    out[2 * n_set + o] = res[2];
    out[3 * n_set + o] = res[3];
    out[4 * n_set + o] = sqrtf((res[1] * res[1] + res[2] * res[2]) + res[3] * res[3]);
    if constexpr (GRAD) {
#pragma unroll
        for (int k = 4; k < 8; ++k) out[(k + 1) * n_set + o] = res[k];
    }
}

// ---- streamlines (ludwig_streamlines_*; no reference counterpart; include/ludwig_hip.h states the definition and
// open_ludwig_amd/streamlines.py restates it in numpy bit for bit) ----
// The one observer whose points move: nothing is planned on the host, the kernel locates every point on the level hierarchy itself
// (stream_sample). Eight lanes per line, one wave = eight lines. A pass is a chain of dependent loads - block_pointer of every level,
// block_pointer of the corner, obstacle, then rho and u - 2 max_steps samples long, so the lanes of a group split what is independent:
//   locate: lane c tests level n_levels - 1 - c (8 levels per round; all lookups in flight together), the finest hit wins through a
//           shuffle maximum;
//   gather: lane c finds stencil corner c = dx + 2 dy + 4 dz on the chosen level and loads its obstacle flag and its four values; a
//           corner that is no fluid cell of the level takes the base cell's values from lane 0 (the probes' rule);
//   lerp:   three rounds of __shfl_xor (1: x, 2: y, 4: z), every lane evaluating probe_lerp on its pair, so that after the third all
//           eight hold the probes' result; the position update is then computed by all eight alike.
// The lanes of a group run the same control flow on the same bits, so a shuffle always meets its seven partners. No index depends on
// unchecked data: a coordinate is converted to an integer only after the float range test, a block index is used only when the
// block_pointer entry is positive (the set's creation has checked every entry against the level's block count). Lanes 0 and 1 write a
// vertex's 32-byte record as one float4 each. Nothing but the set's own buffers is written.
struct StreamLevel {
    const int32_t *bp;           // [gx][gy][gz], x fastest: internal block + 1, 0 = absent
    const uint8_t *obstacle;     // [block][512]
    const float *rho;            // [block][512]
    const float *vel[2];         // vel, vel_temp: [block][3][512]
    int32_t gx, gy, gz;          // blocks per axis
    int32_t n_blocks;
};

struct StreamArgs {
    const StreamLevel *lv;       // [n_levels] in device memory: a lane indexes it with its own level
    int32_t n_levels;
    uint32_t temp_mask;          // bit li: level li's newest velocity is vel_temp
    const float *seeds;          // [n_lines][3]
    const float *sign;           // [n_lines] +-1
    int32_t n_lines, max_steps;
    float step, min_speed;
    float *rec;                  // [n_lines][max_steps + 1][8]
    int32_t *counts, *codes;     // [n_lines]
};

constexpr int STREAM_END_STEPS = 0, STREAM_END_OUTSIDE = 1, STREAM_END_OBSTACLE = 2, STREAM_END_SLOW = 3;
constexpr int STREAM_REC_FLOATS = 8;

__device__ __forceinline__ float stream_group_lerp(float v, int c, int bit, float w)
{
    const float o = __shfl_xor(v, bit, 8);
    return (c & bit) ? probe_lerp(o, v, w) : probe_lerp(v, o, w);
}

// cell coordinate of P on level li and whether the level's grid holds it: g, then base cell i0 (valid only if true is returned)
__device__ __forceinline__ bool stream_cell(const StreamLevel &L, int li, float px, float py, float pz, float g[3], int i0[3])
{
    const float sc = ldexpf(1.0f, li);                               // exact
    g[0] = px * sc - 0.5f;
    g[1] = py * sc - 0.5f;
    g[2] = pz * sc - 0.5f;
    const float fx = floorf(g[0]), fy = floorf(g[1]), fz = floorf(g[2]);
    // NaN fails every comparison, an infinity the upper one
    const bool in = g[0] >= 0.0f && g[1] >= 0.0f && g[2] >= 0.0f && fx <= (float)(8 * L.gx - 1) && fy <= (float)(8 * L.gy - 1) &&
                    fz <= (float)(8 * L.gz - 1);
    i0[0] = in ? (int)fx : 0;
    i0[1] = in ? (int)fy : 0;
    i0[2] = in ? (int)fz : 0;
    return in;
}

// internal block of the cell (x, y, z) of level L, -1: outside the grid or no block there
__device__ __forceinline__ int stream_block(const StreamLevel &L, int x, int y, int z)
{
    if (x < 0 || y < 0 || z < 0 || x >= 8 * L.gx || y >= 8 * L.gy || z >= 8 * L.gz) return -1;
    return L.bp[(x >> 3) + (int64_t)L.gx * ((y >> 3) + (int64_t)L.gy * (z >> 3))] - 1;
}

// sample(P) by the group of eight; c = the lane's corner. Returns the end code (0: found) - the same in all eight lanes - and
// rho, ux, uy, uz in q, the level index in li.
// `mine` = the table entry of level n_levels - 1 - c (the lane's level in the first round of the locate), kept in registers.
// RHO = false (the tracers) leaves rho out of the gather and the lerp: q[0] is then not written and the level's rho is never read.
template <bool RHO = true>
__device__ __forceinline__ int stream_sample(const StreamArgs &a, const StreamLevel &mine, int c, float px, float py, float pz, float q[4],
                                             int &li)
{
    // locate: the finest level whose active blocks hold the base cell
    int found = -1;
    for (int top = a.n_levels - 1; top >= 0 && found < 0; top -= 8) {
        const int l = top - c;
        int hit = -1;
        if (l >= 0) {
            float g[3];
            int i0[3];
            if (top == a.n_levels - 1) {
                if (stream_cell(mine, l, px, py, pz, g, i0) && stream_block(mine, i0[0], i0[1], i0[2]) >= 0) hit = l;
            } else {
                const StreamLevel &L = a.lv[l];
                if (stream_cell(L, l, px, py, pz, g, i0) && stream_block(L, i0[0], i0[1], i0[2]) >= 0) hit = l;
            }
        }
        hit = max(hit, __shfl_xor(hit, 1, 8));
        hit = max(hit, __shfl_xor(hit, 2, 8));
        hit = max(hit, __shfl_xor(hit, 4, 8));
        found = hit;
    }
    if (found < 0) return STREAM_END_OUTSIDE;
    li = found;
    // gather: this lane's corner on the chosen level
    const StreamLevel &L = a.lv[found];
    float g[3];
    int i0[3];
    (void)stream_cell(L, found, px, py, pz, g, i0);
    const int x = i0[0] + (c & 1), y = i0[1] + ((c >> 1) & 1), z = i0[2] + (c >> 2);
    const int b = stream_block(L, x, y, z);
    bool fluid = false;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (b >= 0) {
        const int cell = (x & 7) + 8 * (y & 7) + 64 * (z & 7);
        fluid = L.obstacle[(int64_t)b * CELLS + cell] == 0;
        if (fluid) {
            const float *vel = L.vel[(a.temp_mask >> found) & 1u];
            if (RHO) v[0] = L.rho[(int64_t)b * CELLS + cell];
#pragma unroll
            for (int k = 0; k < 3; ++k) v[1 + k] = vel[((int64_t)b * 3 + k) * CELLS + cell];
        }
    }
    const int base_fluid = __shfl((int)fluid, 0, 8);
    if (!base_fluid) return STREAM_END_OBSTACLE;
    const float wx = g[0] - floorf(g[0]), wy = g[1] - floorf(g[1]), wz = g[2] - floorf(g[2]);
#pragma unroll
    for (int k = RHO ? 0 : 1; k < 4; ++k) {
        const float v0 = __shfl(v[k], 0, 8);
        float t = fluid ? v[k] : v0;
        t = stream_group_lerp(t, c, 1, wx);
        t = stream_group_lerp(t, c, 2, wy);
        q[k] = stream_group_lerp(t, c, 4, wz);
    }
    return 0;
}

__global__ __launch_bounds__(64) void k_streamlines(const StreamArgs a)
{
    const int lane = (int)(blockIdx.x * 64 + threadIdx.x);
    const int line = lane >> 3, c = lane & 7;
    if (line >= a.n_lines) return;                                   // a whole group leaves together
    float px = a.seeds[3 * line], py = a.seeds[3 * line + 1], pz = a.seeds[3 * line + 2];
    const float s = a.sign[line];
    float4 *rec = (float4 *)(a.rec + (int64_t)line * (a.max_steps + 1) * STREAM_REC_FLOATS);
    const StreamLevel mine = a.lv[max(a.n_levels - 1 - c, 0)];
    int k = 0, code = -1;
    while (code < 0) {
        float q[4], qm[4];
        int li = 0, lm = 0;
        const int r = stream_sample(a, mine, c, px, py, pz, q, li);
        if (r) { code = r; break; }
        if (c == 0) rec[2 * k] = make_float4(px, py, pz, q[0]);
        if (c == 1) rec[2 * k + 1] = make_float4(q[1], q[2], q[3], (float)li);
        ++k;
        if (k > a.max_steps) { code = STREAM_END_STEPS; break; }
        const float m = sqrtf((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]);
        if (!(m >= a.min_speed)) { code = STREAM_END_SLOW; break; }
        const float h = ldexpf(a.step, -li);                         // exact
        const float hh = 0.5f * h;
        const float mx = px + hh * ((q[1] / m) * s), my = py + hh * ((q[2] / m) * s), mz = pz + hh * ((q[3] / m) * s);
        const int rm = stream_sample(a, mine, c, mx, my, mz, qm, lm);
        if (rm) { code = rm; break; }
        const float mm = sqrtf((qm[1] * qm[1] + qm[2] * qm[2]) + qm[3] * qm[3]);
        if (!(mm >= a.min_speed)) { code = STREAM_END_SLOW; break; }
        px = px + h * ((qm[1] / mm) * s);
        py = py + h * ((qm[2] / mm) * s);
        pz = pz + h * ((qm[3] / mm) * s);
    }
    if (c == 0) {
        a.counts[line] = k;
        a.codes[line] = code;
    }
}

// ---- tracers (ludwig_tracers_*; no reference counterpart; include/ludwig_hip.h states the definition and open_ludwig_amd/tracers.py
// restates it in numpy bit for bit) ----
// Particles that live across coarse steps: slot g n_seeds + s holds generation g of seed s, a position and a state (-1 empty, 0 alive,
// 1 outside, 2 obstacle, 3 non-finite). An advance is two samples (start and midpoint), each the streamlines' chain of dependent loads,
// so the streamlines' mapping is kept: eight lanes per slot, locate split over levels, one corner per lane, three shuffle rounds; the
// sample is stream_sample<false> (velocity only: the finest level's rho store is elided inside a batch and is never read here). A slot
// belongs to one group of eight lanes and nothing else writes it: no atomics, no compaction, the result depends on no scheduling. The
// state is read before anything else and is the same word in all eight lanes, so a group leaves or stays together and a shuffle always
// meets its partners. Writes: pos and state of the own slot (lane 0), rec of the own slot (lanes 0 and 1); every index into them is
// slot < n_slots, and the seed index is slot % n_seeds.
struct TracerArgs {
    StreamArgs s;                // lv, n_levels, temp_mask; the rest unused
    const float *seeds;          // [n_seeds][3]
    float *pos;                  // [n_slots][3]
    int32_t *state;              // [n_slots]
    float *rec;                  // [n_slots][8] (snapshot)
    int32_t n_seeds, n_slots;
    int32_t released;            // the generation this advance releases, -1: none
    float dt;
};

constexpr int TRACER_EMPTY = -1, TRACER_ALIVE = 0, TRACER_NONFINITE = 3;

__global__ __launch_bounds__(64) void k_tracers_advance(const TracerArgs a)
{
    const int64_t lane = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t slot64 = lane >> 3;
    const int c = (int)(lane & 7);
    if (slot64 >= a.n_slots) return;                                 // a whole group leaves together
    const int slot = (int)slot64;
    const int gen = slot / a.n_seeds, seed = slot - gen * a.n_seeds;
    if (gen == a.released) {                                         // overwritten, not advanced, whatever the slot held
        if (c < 3) a.pos[3 * (int64_t)slot + c] = a.seeds[3 * seed + c];
        if (c == 3) a.state[slot] = TRACER_ALIVE;
        return;
    }
    if (a.state[slot] != TRACER_ALIVE) return;                       // a dead or empty slot is not touched
    const float px = a.pos[3 * (int64_t)slot], py = a.pos[3 * (int64_t)slot + 1], pz = a.pos[3 * (int64_t)slot + 2];
    const StreamLevel mine = a.s.lv[max(a.s.n_levels - 1 - c, 0)];
    float q[4], qm[4];
    int li = 0, lm = 0;
    int code = stream_sample<false>(a.s, mine, c, px, py, pz, q, li);
    if (!code) {
        const float hh = 0.5f * a.dt;
        const float mx = px + hh * q[1], my = py + hh * q[2], mz = pz + hh * q[3];
        code = stream_sample<false>(a.s, mine, c, mx, my, mz, qm, lm);
    }
    if (code) {                                                      // P stays
        if (c == 0) a.state[slot] = code;
        return;
    }
    const float nx = px + a.dt * qm[1], ny = py + a.dt * qm[2], nz = pz + a.dt * qm[3];
    if (c != 0) return;
    if (!(isfinite(nx) && isfinite(ny) && isfinite(nz))) {
        a.state[slot] = TRACER_NONFINITE;
        return;
    }
    a.pos[3 * (int64_t)slot] = nx;
    a.pos[3 * (int64_t)slot + 1] = ny;
    a.pos[3 * (int64_t)slot + 2] = nz;
}

// rec[slot] = x, y, z, ux, uy, uz, level index, code: an alive slot sampled at P (code 0; a failed sample: zeros, level -1, its code),
// any other slot zeros, level -1 and its state. Changes nothing of the set's state.
__global__ __launch_bounds__(64) void k_tracers_snapshot(const TracerArgs a)
{
    const int64_t lane = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t slot64 = lane >> 3;
    const int c = (int)(lane & 7);
    if (slot64 >= a.n_slots) return;
    const int slot = (int)slot64;
    const float px = a.pos[3 * (int64_t)slot], py = a.pos[3 * (int64_t)slot + 1], pz = a.pos[3 * (int64_t)slot + 2];
    int code = a.state[slot];
    float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int li = -1;
    if (code == TRACER_ALIVE) {
        const StreamLevel mine = a.s.lv[max(a.s.n_levels - 1 - c, 0)];
        code = stream_sample<false>(a.s, mine, c, px, py, pz, q, li);
        if (code) {
            q[1] = q[2] = q[3] = 0.0f;
            li = -1;
        }
    }
    float4 *rec = (float4 *)(a.rec + (int64_t)slot * STREAM_REC_FLOATS);
    if (c == 0) rec[0] = make_float4(px, py, pz, q[1]);
    if (c == 1) rec[1] = make_float4(q[2], q[3], (float)li, (float)code);
}

// ---- volume images (ludwig_render_*; no reference counterpart; include/ludwig_hip.h states the definition and
// open_ludwig_amd/render.py restates it in numpy bit for bit) ----
// One lane per ray, one wavefront per 8 x 8 pixel tile: the rays of a wave stay within a few cells of each other, so their block_pointer
// entries, obstacle bytes and scalar values share cache lines, and a frame has millions of independent rays to hide the chain of dependent
// loads of one sample (block_pointer, then obstacle, then values) - unlike a streamline set, where eight lanes share a point because the
// points are few. Within a lane the eight corners are eight independent loads at each link of the chain.
// The locate loop runs over the levels with a wave-uniform counter, so a level's table entry is read with scalar loads; a lane that
// finds its level keeps what it needs of the entry in registers. Guards are the streamlines' (stream_cell, stream_block): a coordinate
// becomes an integer only after the float range test, a block index is used only when the block_pointer entry is positive. The colour
// table index comes from a value clamped to [0, 1]. A pixel is written by its own lane and by nothing else: no atomics.
struct RenderScalar {
    const float *s;              // the scalar of cell c of internal block b: s[b * stride + c]
    int64_t stride;
};

struct RenderArgs {
    const StreamLevel *lv;       // [n_levels]: bp, obstacle and the grid's extent are read, rho and vel are not
    const RenderScalar *sc;      // [n_levels]
    int32_t n_levels;
    int32_t width, height, perspective;
    float eye[3], corner[3], du[3], dv[3], dir[3];
    float hi[3];                 // the box's upper corner
    float step, lo, inv, t_min;
    int32_t max_samples;
    float bg[3], body[3];
    const float4 *table;         // [256] r, g, b, kappa
    float4 *rgba;                // [height][width]
    int32_t *codes, *samples;    // [height][width]
};

constexpr int RENDER_EXIT = 0, RENDER_MISS = 1, RENDER_BODY = 2, RENDER_OPAQUE = 3, RENDER_SAMPLES = 4;
constexpr int RENDER_FOUND = 0, RENDER_OUTSIDE = 1, RENDER_OBSTACLE = 2;

// what a lane keeps of the level it found: the part of the table entry stream_block reads, and the scalar
struct RenderHit {
    StreamLevel L;               // bp, obstacle, gx, gy, gz
    const float *s;
    int64_t stride;
    int i0[3];                   // base cell
    int b0;                      // its internal block
};

// sample(P) of one lane: RENDER_FOUND with the value in s, RENDER_OBSTACLE or RENDER_OUTSIDE; li = the level index (0 when outside);
// h describes the base cell unless outside
__device__ __forceinline__ int render_sample(const RenderArgs &a, float px, float py, float pz, float &s, int &li, RenderHit &h)
{
    int found = -1;
    float g[3] = {0.0f, 0.0f, 0.0f};
    for (int l = a.n_levels - 1; l >= 0; --l) {                      // l is the same in every lane
        if (found < 0) {
            const StreamLevel &L = a.lv[l];
            float gl[3];
            int il[3];
            if (stream_cell(L, l, px, py, pz, gl, il)) {
                const int b = stream_block(L, il[0], il[1], il[2]);
                if (b >= 0) {
                    found = l;
                    h.L.bp = L.bp; h.L.obstacle = L.obstacle;
                    h.L.gx = L.gx; h.L.gy = L.gy; h.L.gz = L.gz;
                    h.s = a.sc[l].s; h.stride = a.sc[l].stride;
                    h.b0 = b;
#pragma unroll
                    for (int k = 0; k < 3; ++k) { g[k] = gl[k]; h.i0[k] = il[k]; }
                }
            }
        }
        if (__ballot(found < 0) == 0) break;
    }
    li = max(found, 0);
    if (found < 0) return RENDER_OUTSIDE;
    // the eight corners: eight block_pointer entries, then eight obstacle bytes, then eight values, each set independent loads
    int bc[8], cell[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int x = h.i0[0] + (c & 1), y = h.i0[1] + ((c >> 1) & 1), z = h.i0[2] + (c >> 2);
        bc[c] = c == 0 ? h.b0 : stream_block(h.L, x, y, z);
        cell[c] = (x & 7) + 8 * (y & 7) + 64 * (z & 7);
    }
    bool fluid[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) fluid[c] = bc[c] >= 0 && h.L.obstacle[(int64_t)bc[c] * CELLS + cell[c]] == 0;
    if (!fluid[0]) return RENDER_OBSTACLE;
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {                                    // a corner that is no fluid cell of the level takes the base cell's value
        const int b = fluid[c] ? bc[c] : h.b0, ce = fluid[c] ? cell[c] : cell[0];
        v[c] = h.s[(int64_t)b * h.stride + ce];
    }
    const float wx = g[0] - floorf(g[0]), wy = g[1] - floorf(g[1]), wz = g[2] - floorf(g[2]);
    s = probe_trilinear(v, wx, wy, wz);
    return RENDER_FOUND;
}

// 1 if the cell (x, y, z) of the hit's level is an obstacle cell of an active block, else 0
__device__ __forceinline__ int render_solid(const RenderHit &h, int x, int y, int z)
{
    const int b = stream_block(h.L, x, y, z);
    if (b < 0) return 0;
    return h.L.obstacle[(int64_t)b * CELLS + (x & 7) + 8 * (y & 7) + 64 * (z & 7)] != 0 ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_render(const RenderArgs a)
{
    const int tiles_x = (a.width + 7) >> 3;
    const int tile = (int)blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int i = 8 * tx + ((int)threadIdx.x & 7), j = 8 * ty + ((int)threadIdx.x >> 3);
    if (i >= a.width || j >= a.height) return;
    const int64_t pixel = (int64_t)j * a.width + i;
    float o[3], d[3];
    bool miss = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = (a.corner[k] + (float)i * a.du[k]) + (float)j * a.dv[k];
    if (a.perspective) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            d[k] = o[k] - a.eye[k];
            o[k] = a.eye[k];
        }
        const float m = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        miss = !(m > 0.0f && m < __int_as_float(0x7f800000));       // zero, infinite or NaN
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = d[k] / m;
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = a.dir[k];
    }
    float t0 = 0.0f, t1 = __int_as_float(0x7f800000);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (d[k] == 0.0f) {
            if (!(0.0f <= o[k] && o[k] <= a.hi[k])) miss = true;
        } else {
            const float p = (0.0f - o[k]) / d[k], q = (a.hi[k] - o[k]) / d[k];
            t0 = fmaxf(t0, fminf(p, q));
            t1 = fminf(t1, fmaxf(p, q));
        }
    }
    if (!(t0 < t1)) miss = true;
    float T = 1.0f, R = 0.0f, G = 0.0f, B = 0.0f;
    int n = 0, code = RENDER_MISS;
    if (!miss) {
        float t = t0;
        for (;;) {
            if (!(t < t1)) { code = RENDER_EXIT; break; }
            if (n == a.max_samples) { code = RENDER_SAMPLES; break; }
            const float px = o[0] + t * d[0], py = o[1] + t * d[1], pz = o[2] + t * d[2];
            float s = 0.0f;
            int li = 0;
            RenderHit h{};
            const int kind = render_sample(a, px, py, pz, s, li, h);
            ++n;
            const float delta = ldexpf(a.step, -li);                 // exact
            if (kind == RENDER_OBSTACLE) {
                const int x = h.i0[0], y = h.i0[1], z = h.i0[2];
                const int nx = render_solid(h, x - 1, y, z) - render_solid(h, x + 1, y, z);
                const int ny = render_solid(h, x, y - 1, z) - render_solid(h, x, y + 1, z);
                const int nz = render_solid(h, x, y, z - 1) - render_solid(h, x, y, z + 1);
                const int nn = nx * nx + ny * ny + nz * nz;
                float shade = 1.0f;
                if (nn != 0) {
                    const float c = -(((float)nx * d[0] + (float)ny * d[1]) + (float)nz * d[2]) / sqrtf((float)nn);
                    shade = 0.3f + 0.7f * fmaxf(c, 0.0f);
                }
                R = R + T * (a.body[0] * shade);
                G = G + T * (a.body[1] * shade);
                B = B + T * (a.body[2] * shade);
                T = 0.0f;
                code = RENDER_BODY;
                break;
            }
            if (kind == RENDER_FOUND && s == s) {
                const float x = fminf(fmaxf((s - a.lo) * a.inv, 0.0f), 1.0f);    // fmaxf returns 0 for a NaN product
                const float4 e = a.table[(int)(x * 255.0f + 0.5f)];
                const float w = T * fminf(e.w * delta, 1.0f);
                R = R + w * e.x;
                G = G + w * e.y;
                B = B + w * e.z;
                T = T - w;
                if (T < a.t_min) { code = RENDER_OPAQUE; break; }
            }
            t = t + delta;
        }
    }
    if (code != RENDER_BODY) {
        R = R + T * a.bg[0];
        G = G + T * a.bg[1];
        B = B + T * a.bg[2];
    }
    a.rgba[pixel] = make_float4(R, G, B, 1.0f - T);
    a.codes[pixel] = code;
    a.samples[pixel] = n;
}

// ---- iso-surfaces (ludwig_level_isosurface_*; no reference counterpart; open_ludwig_amd/isosurface.py states the definition and
// restates it in numpy bit for bit) ----
// Workgroup r = reference block r of the owned ones (the output order), 256 lanes, two x-consecutive anchor cells per lane. The block's
// 9 x 9 x 9 tile of the scalar - the block and the first layer of its +x, +y, +z face, edge and corner neighbours - is staged in LDS
// (2.9 KB); a corner that cannot take part (no block there, an obstacle cell, a non-finite value) is staged as NaN, so "all eight
// corners finite" is the whole liveness test of a cube once its anchor passes (block not skipped, global cell in [lo, hi)).
// k_iso_count writes the block's triangle count; the host scans the counts (int64) into block offsets; k_iso_emit recomputes the per-cell
// counts, scans them in cell order (wave scan with shuffles, the four wave totals through LDS) and writes every triangle at its place with
// plain stores: no atomics, so the order depends on neither the internal block order nor scheduling.
// The eight corner values stay in registers: the tetrahedra are unrolled with compile-time corner numbers, and what depends on the case
// (which tetrahedron edge a vertex sits on) selects among four registers, never indexes an array.
constexpr int ISO_TILE = 9, ISO_TILE2 = 81, ISO_TILE3 = 729;
enum { ISO_DENSITY = 0, ISO_VELOCITY_MAGNITUDE = 1, ISO_Q_CRITERION = 2, ISO_VORTICITY_MAGNITUDE = 3 };
constexpr int ISO_POS_FLOATS = 9, ISO_ATT_FLOATS = 12, ISO_KEY_INTS = 6;      // per triangle: 3 x (3 | 4 | 2)

struct IsoArgs {
    const float *s;            // the scalar of cell c of internal block b: s[b * s_stride + c]
    int64_t s_stride;
    const uint8_t *obstacle;
    const int32_t *meta;
    const int32_t *ref2int;    // nullptr: the reference order is kept
    const uint8_t *skip;       // [n_owned], reference order: non-zero = no cube is anchored in the block
    int32_t lo[3], hi[3];
    float value;
};

// the corners of tetrahedron k: 0, then two consecutive corners of the cycle 1 3 2 6 4 5 around the diagonal, then 7
__host__ __device__ constexpr int iso_tet_corner(int k, int j)
{
    constexpr int cyc[6] = {1, 3, 2, 6, 4, 5};
    return j == 0 ? 0 : j == 3 ? 7 : cyc[(k + j - 1) % 6];
}
__device__ __forceinline__ int iso_case_triangles(int m)
{
    const int n = __popc((unsigned)m);
    return (n == 1 || n == 3) ? 1 : (n == 2 ? 2 : 0);
}
__device__ __forceinline__ bool iso_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
template <class T>
__device__ __forceinline__ T iso_sel4(T a, T b, T c, T d, int i) { return i == 0 ? a : (i == 1 ? b : (i == 2 ? c : d)); }

// value[c] = sqrtf((a^2 + b^2) + c^2) of the first three components of src [block][K][512]: the velocity (K = 3), or the vorticity
// of the gradient fields (K = 4). Every block of the level, ghosts included (their gradient fields are 0).
template <int WHICH>
__global__ __launch_bounds__(256) void k_iso_scalar(float *__restrict__ out, const float *__restrict__ src)
{
    static_assert(WHICH == ISO_VELOCITY_MAGNITUDE || WHICH == ISO_VORTICITY_MAGNITUDE, "the other scalars are read in place");
    constexpr int K = WHICH == ISO_VELOCITY_MAGNITUDE ? 3 : GRAD_COMPONENTS;
    const int64_t b = blockIdx.x;
    const int c = 2 * (int)threadIdx.x;
    const float *p = src + b * K * CELLS + c;
    const float2 x = *(const float2 *)p, y = *(const float2 *)(p + CELLS), z = *(const float2 *)(p + 2 * CELLS);
    *(float2 *)(out + b * CELLS + c) = make_float2(sqrtf((x.x * x.x + y.x * y.x) + z.x * z.x), sqrtf((x.y * x.y + y.y * y.y) + z.y * z.y));
}

// stage the tile of internal block b; returns bit 0: some staged value is inside (>= value), bit 1: some is outside
__device__ __forceinline__ int iso_stage_tile(float *tile, const IsoArgs &a, const int64_t b, const int t)
{
    int seen = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int i = t + 256 * r;
        if (i < ISO_TILE3) {
            const int tz = i / ISO_TILE2, ty = (i - tz * ISO_TILE2) / ISO_TILE, tx = i - tz * ISO_TILE2 - ty * ISO_TILE;
            const int ox = tx >> 3, oy = ty >> 3, oz = tz >> 3;
            int64_t nb = b;
            if (ox | oy | oz) nb = a.meta[b * NBR_STRIDE + DIR(ox, oy, oz)];
            float v = __int_as_float(0x7fc00000);
            if (nb >= 0) {
                const int cell = (tx & 7) + 8 * (ty & 7) + 64 * (tz & 7);
                const float q = a.s[nb * a.s_stride + cell];
                if (a.obstacle[nb * CELLS + cell] == 0 && iso_finite(q)) v = q;
            }
            tile[i] = v;
            seen |= (v >= a.value ? 1 : 0) | (v < a.value ? 2 : 0);
        }
    }
    return seen;
}

// the eight corners of the cube anchored at (x, y, z) and its triangle count (0 when the cube is not live)
__device__ __forceinline__ int iso_cube(float (&v)[8], const float *tile, const IsoArgs &a, const int32_t *row, int x, int y, int z)
{
    const int at = x + ISO_TILE * y + ISO_TILE2 * z;
    bool live = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        v[c] = tile[at + (c & 1) + ISO_TILE * ((c >> 1) & 1) + ISO_TILE2 * (c >> 2)];
        live = live && iso_finite(v[c]);
    }
    const int gx = (row[NBR_BX] - 1) * BS + x, gy = (row[NBR_BY] - 1) * BS + y, gz = (row[NBR_BZ] - 1) * BS + z;
    live = live && gx >= a.lo[0] && gx < a.hi[0] && gy >= a.lo[1] && gy < a.hi[1] && gz >= a.lo[2] && gz < a.hi[2];
    if (!live) return 0;
    int n = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) m |= (v[iso_tet_corner(k, j)] >= a.value ? 1 : 0) << j;
        n += iso_case_triangles(m);
    }
    return n;
}

__global__ __launch_bounds__(256) void k_iso_count(int32_t *__restrict__ counts, const IsoArgs a)
{
    __shared__ float tile[ISO_TILE3];
    __shared__ int wseen[4], wsum[4];
    const int r = (int)blockIdx.x, t = (int)threadIdx.x;
    if (a.skip[r]) {
        if (t == 0) counts[r] = 0;
        return;
    }
    const int64_t b = a.ref2int ? a.ref2int[r] : r;
    const int seen = iso_stage_tile(tile, a, b, t);
    const int s_in = __ballot(seen & 1) != 0, s_out = __ballot(seen & 2) != 0;
    if ((t & 63) == 0) wseen[t >> 6] = s_in | (s_out << 1);
    __syncthreads();
    if (((wseen[0] | wseen[1]) | (wseen[2] | wseen[3])) != 3) {      // the tile does not straddle the value
        if (t == 0) counts[r] = 0;
        return;
    }
    const int c = 2 * t, x = c & 7, y = (c >> 3) & 7, z = c >> 6;
    const int32_t *row = a.meta + b * NBR_STRIDE;
    float v[8];
    int n = iso_cube(v, tile, a, row, x, y, z);
    n += iso_cube(v, tile, a, row, x + 1, y, z);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) n += __shfl_xor(n, o, 64);
    if ((t & 63) == 0) wsum[t >> 6] = n;
    __syncthreads();
    if (t == 0) counts[r] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

struct IsoEmitArgs {
    const int32_t *counts;     // [n_owned] what k_iso_count wrote
    const int64_t *offsets;    // [n_owned] their exclusive scan
    int64_t n_triangles;       // the total: nothing is written at or beyond it
    const int32_t *int2ref;    // nullptr: the reference order is kept
    const float *rho, *vel;
    float *pos, *att;          // [n_triangles][3][3], [n_triangles][3][4]
    int32_t *keys;             // [n_triangles][3][2]
};

// vertex `slot` (3 * triangle + corner of the triangle) on edge e of tetrahedron K of the cube anchored at (x, y, z) of internal block b
template <int K>
__device__ __forceinline__ void iso_vertex(const IsoArgs &a, const IsoEmitArgs &o, const float (&v)[8], const int64_t b,
                                           const int32_t *row, int x, int y, int z, int e, int64_t slot)
{
    constexpr int c0 = iso_tet_corner(K, 0), c1 = iso_tet_corner(K, 1), c2 = iso_tet_corner(K, 2), c3 = iso_tet_corner(K, 3);
    // tetrahedron edges 0..5 = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), two bits per end
    const int i = (0x940 >> (2 * e)) & 3, j = (0xFB9 >> (2 * e)) & 3;
    const int ci = iso_sel4(c0, c1, c2, c3, i), cj = iso_sel4(c0, c1, c2, c3, j);
    const float si = iso_sel4(v[c0], v[c1], v[c2], v[c3], i), sj = iso_sel4(v[c0], v[c1], v[c2], v[c3], j);
    const bool fwd = ci < cj;
    const int ca = fwd ? ci : cj, cb = fwd ? cj : ci;
    const float sa = fwd ? si : sj, sb = fwd ? sj : si;
    float tt = (a.value - sa) / (sb - sa);
    tt = fminf(fmaxf(tt, 0.0f), 1.0f);
    const int ax = x + (ca & 1), ay = y + ((ca >> 1) & 1), az = z + (ca >> 2);
    const int bx = x + (cb & 1), by = y + ((cb >> 1) & 1), bz = z + (cb >> 2);
    const int gx = (row[NBR_BX] - 1) * BS, gy = (row[NBR_BY] - 1) * BS, gz = (row[NBR_BZ] - 1) * BS;
    float *p = o.pos + 3 * slot;
    p[0] = (float)(gx + ax) + tt * (float)(bx - ax);
    p[1] = (float)(gy + ay) + tt * (float)(by - ay);
    p[2] = (float)(gz + az) + tt * (float)(bz - az);
    // the cells of a and b: every corner block of a live cube exists
    int64_t na = b, nb = b;
    if ((ax | ay | az) >> 3) na = row[DIR(ax >> 3, ay >> 3, az >> 3)];
    if ((bx | by | bz) >> 3) nb = row[DIR(bx >> 3, by >> 3, bz >> 3)];
    const int xa = (ax & 7) + 8 * (ay & 7) + 64 * (az & 7), xb = (bx & 7) + 8 * (by & 7) + 64 * (bz & 7);
    const float ra = o.rho[na * CELLS + xa], rb = o.rho[nb * CELLS + xb];
    float4 q;
    q.x = ra + tt * (rb - ra);
    const float *va = o.vel + na * 3 * CELLS + xa, *vb = o.vel + nb * 3 * CELLS + xb;
    q.y = va[0] + tt * (vb[0] - va[0]);
    q.z = va[CELLS] + tt * (vb[CELLS] - va[CELLS]);
    q.w = va[2 * CELLS] + tt * (vb[2 * CELLS] - va[2 * CELLS]);
    *(float4 *)(o.att + 4 * slot) = q;
    const int32_t ka = (int32_t)(o.int2ref ? o.int2ref[na] : na) * CELLS + xa, kb = (int32_t)(o.int2ref ? o.int2ref[nb] : nb) * CELLS + xb;
    *(int2 *)(o.keys + 2 * slot) = make_int2(ka, kb);
}

// the triangles of one live cube, from triangle `tri` on
__device__ __forceinline__ void iso_emit_cube(const IsoArgs &a, const IsoEmitArgs &o, const float (&v)[8], const int64_t b,
                                              const int32_t *row, int x, int y, int z, int64_t tri)
{
    // case = sum of 2^j over the inside corners j of the tetrahedron -> its triangles: bits 18..19 how many, then 3 bits per vertex, the
    // tetrahedron edge it sits on; wound so that the normal points from the inside corners to the outside ones (every tetrahedron of
    // the split has positive orientation); case 15 - m is case m reversed (isosurface.CASE_TRIANGLES)
    const uint32_t cases[16] = {0x0, 0x40088, 0x400e0, 0x9c311, 0x40159, 0x95158, 0x8d160, 0x40162,
                                0x4012a, 0xa5148, 0x9d150, 0x400e9, 0x94319, 0x40118, 0x40050, 0x0};
#define LW_ISO_TET(K)                                                                                          \
    {                                                                                                          \
        int m = 0;                                                                                             \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) m |= (v[iso_tet_corner(K, j)] >= a.value ? 1 : 0) << j;  \
        const uint32_t w = cases[m];                                                                           \
        const int nv = 3 * (int)(w >> 18);                                                                     \
        if (tri + (nv / 3) <= o.n_triangles)                                                                   \
            for (int q = 0; q < nv; ++q) iso_vertex<K>(a, o, v, b, row, x, y, z, (int)((w >> (3 * q)) & 7u), 3 * tri + q); \
        tri += nv / 3;                                                                                         \
    }
    LW_ISO_TET(0) LW_ISO_TET(1) LW_ISO_TET(2) LW_ISO_TET(3) LW_ISO_TET(4) LW_ISO_TET(5)
#undef LW_ISO_TET
}

__global__ __launch_bounds__(256) void k_iso_emit(const IsoArgs a, const IsoEmitArgs o)
{
    __shared__ float tile[ISO_TILE3];
    __shared__ int wsum[4];
    const int r = (int)blockIdx.x, t = (int)threadIdx.x;
    if (o.counts[r] == 0) return;
    const int64_t b = a.ref2int ? a.ref2int[r] : r;
    (void)iso_stage_tile(tile, a, b, t);
    __syncthreads();
    const int c = 2 * t, x = c & 7, y = (c >> 3) & 7, z = c >> 6;
    const int32_t *row = a.meta + b * NBR_STRIDE;
    float v[8];
    const int n0 = iso_cube(v, tile, a, row, x, y, z), n1 = iso_cube(v, tile, a, row, x + 1, y, z);
    // exclusive scan over the block's 512 cells in cell order: lanes hold consecutive pairs, waves consecutive lanes
    int inc = n0 + n1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d, 64);
        if ((t & 63) >= d) inc += up;
    }
    if ((t & 63) == 63) wsum[t >> 6] = inc;
    __syncthreads();
    int before = inc - (n0 + n1);
#pragma unroll
    for (int w = 0; w < 3; ++w)
        if (w < (t >> 6)) before += wsum[w];
    const int64_t first = o.offsets[r] + before;
    if (n0 > 0) {
        (void)iso_cube(v, tile, a, row, x, y, z);
        iso_emit_cube(a, o, v, b, row, x, y, z, first);
    }
    if (n1 > 0) {
        (void)iso_cube(v, tile, a, row, x + 1, y, z);
        iso_emit_cube(a, o, v, b, row, x + 1, y, z, first + n0);
    }
}

// ---- internal storage (ludwig_hip.hip "block order", "block-major"): the caller's arrays keep the reference's layout,
// [8,8,8,n_blocks,K] with the reference's block order; the device arrays hold the blocks in the library's own order, block-major.
// ref2int[b_reference] = b_internal (nullptr = same order) ----
// element offset in the reference layout (cell + 512 b + 512 n_blocks k) -> the same element in the device array
__device__ __forceinline__ int64_t to_internal_offset(int64_t off, const int32_t *__restrict__ ref2int, int64_t n_cells, int K)
{
    const int64_t k = off / n_cells, r = off - k * n_cells;
    const int64_t blk = ref2int ? (int64_t)ref2int[r >> 9] : (r >> 9);
    return (blk * K + k) * CELLS + (r & 511);
}
// one component k of a K-component field: src / dst = that component in the reference layout, n = 512 n_blocks elements
template <class T>
__global__ __launch_bounds__(256) void k_component_to_internal(T *__restrict__ dev, const T *__restrict__ src, const int32_t *__restrict__ ref2int, int64_t n, int K, int k)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dev[((ref2int ? (int64_t)ref2int[i >> 9] : (i >> 9)) * K + k) * CELLS + (i & 511)] = src[i];
}
template <class T>
__global__ __launch_bounds__(256) void k_component_to_reference(T *__restrict__ dst, const T *__restrict__ dev, const int32_t *__restrict__ ref2int, int64_t n, int K, int k)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = dev[((ref2int ? (int64_t)ref2int[i >> 9] : (i >> 9)) * K + k) * CELLS + (i & 511)];
}

// ---- halo pack / unpack: index holds element offsets in the REFERENCE layout ----
__global__ void k_gather(const float *__restrict__ field, const int64_t *__restrict__ index, int64_t n, float *__restrict__ dst,
                         const int32_t *__restrict__ ref2int, int64_t n_cells, int K)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = field[to_internal_offset(index[i], ref2int, n_cells, K)];
}
__global__ void k_scatter(float *__restrict__ field, const int64_t *__restrict__ index, int64_t n, const float *__restrict__ src,
                          const int32_t *__restrict__ ref2int, int64_t n_cells, int K)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) field[to_internal_offset(index[i], ref2int, n_cells, K)] = src[i];
}

// ---- structured halo pack / unpack (ludwig_halo_plan_*): the elements of a message grouped into OCTETS - aligned groups of 8
// consecutive floats of the device array = one 32-B sector - with a mask of the members that travel. desc = (octet index in the
// field, position of the octet's first member in the message, mask, unused). Eight threads share a descriptor: the sector is
// read / written once, whole, and the message side is contiguous. A z face (whole 8x8 planes) and a y face (rows of 8) are full
// octets: 16 B of descriptor per 32 B of payload, against 8 B of index per 4 B with k_gather / k_scatter. Octets with one or two
// members (an x face: single cells 32 B apart) would waste six or seven of their eight threads: those members go to a second
// list, one thread each, single = (octet index, message position << 3 | member) - threads [8 n_oct, 8 n_oct + n_single). ----
__global__ __launch_bounds__(256) void k_pack_octets(const float *__restrict__ field, const uint4 *__restrict__ desc, int64_t n_oct,
                                                     const uint2 *__restrict__ single, int64_t n_single, float *__restrict__ msg)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, o = t >> 3;
    if (o < n_oct) {
        const int j = (int)(t & 7);
        const uint4 d = desc[o];
        if ((d.z >> j) & 1u) msg[(size_t)d.y + __popc(d.z & ((1u << j) - 1u))] = field[(size_t)d.x * 8 + j];
    } else {
        const int64_t i = t - n_oct * 8;
        if (i >= n_single) return;
        const uint2 d = single[i];
        msg[d.y >> 3] = field[(size_t)d.x * 8 + (d.y & 7u)];
    }
}
__global__ __launch_bounds__(256) void k_unpack_octets(float *__restrict__ field, const uint4 *__restrict__ desc, int64_t n_oct,
                                                       const uint2 *__restrict__ single, int64_t n_single, const float *__restrict__ msg)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, o = t >> 3;
    if (o < n_oct) {
        const int j = (int)(t & 7);
        const uint4 d = desc[o];
        if ((d.z >> j) & 1u) field[(size_t)d.x * 8 + j] = msg[(size_t)d.y + __popc(d.z & ((1u << j) - 1u))];
    } else {
        const int64_t i = t - n_oct * 8;
        if (i >= n_single) return;
        const uint2 d = single[i];
        field[(size_t)d.x * 8 + (d.y & 7u)] = msg[d.y >> 3];
    }
}

// ---- flow monitor (ludwig_level_monitor; compute_flow_stats of every level plus where, reference src/diagnostics.jl:56-94) ----
// One record per level from one streaming pass over rho, one velocity buffer and obstacle (17 B per cell). Per non-obstacle cell
// v2 = (ux ux + uy uy) + uz uz in float32 (-ffp-contract=off); the cell is COUNTED iff rho, ux, uy, uz and v2 are all finite, else
// BAD. Over the counted cells: min / max of rho and max of v2, IEEE < and >, among equal values the cell lowest in
// (bx, by, bz, cell) order - a key built from the block's own coordinates (meta), so neither the internal block order nor a rank's
// block list can show; over the bad cells the lowest such key. Two Float64 sums, rho and rho v2 (a product of two floats is exact in
// double), every other cell adding +0.0, in one fixed balanced tree: inside a block over the 512 cells in cell order, adjacent pairs
// halved nine times (the lane's two cells, an xor-butterfly over the wave, the four waves through LDS); across blocks the same
// halving over the per-block records in the reference block order, 512 records per workgroup and launch - missing records are +0.0,
// and adding +0.0 is exact, so the chunks give the bits of the one tree. open_ludwig_amd/monitor.py (host_monitor) restates all of it.
// k_monitor_blocks: workgroup r = reference block r of the owned ones, two x-consecutive cells per lane, one MonitorRecord per block
// into a slab with plain stores. k_monitor_combine: 512 records -> 1, until one is left. No atomics.
struct MonitorRecord {
    double sum_rho, sum_rho_v2;
    long long n_fluid, n_bad;
    unsigned long long key_rho_min, key_rho_max, key_v2_max, key_bad;   // MONITOR_NO_KEY: absent
    float rho_min, rho_max, v2_max, pad;
};
constexpr unsigned long long MONITOR_NO_KEY = ~0ull;
// the neutral record: what a level without fluid cells reports and what a missing record counts as
__device__ __forceinline__ MonitorRecord monitor_empty()
{
    MonitorRecord r;
    r.sum_rho = r.sum_rho_v2 = 0.0;
    r.n_fluid = r.n_bad = 0;
    r.key_rho_min = r.key_rho_max = r.key_v2_max = r.key_bad = MONITOR_NO_KEY;
    r.rho_min = __int_as_float(0x7f800000); r.rho_max = r.v2_max = __int_as_float(0xff800000); r.pad = 0.0f;
    return r;
}
constexpr int MONITOR_COORD_BITS = 18;                         // block coordinates 1 .. 2^18 - 1 per axis, 9 bits of cell
__device__ __forceinline__ unsigned long long monitor_block_key(int bx, int by, int bz)
{
    return ((((unsigned long long)(unsigned)bx << MONITOR_COORD_BITS | (unsigned)by) << MONITOR_COORD_BITS) | (unsigned)bz) << 9;
}
__device__ __forceinline__ bool monitor_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ double monitor_wave_sum(double x)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) x += __shfl_xor(x, o, 64);      // adjacent pairs first: the halving tree, every lane ends with the sum
    return x;
}
// the lowest lane whose flag is set, -1 if none (wave-uniform)
__device__ __forceinline__ int monitor_first_lane(bool flag)
{
    const unsigned long long m = __ballot(flag);
    return m ? (int)__builtin_ctzll(m) : -1;
}
// one extreme of a block's wave: every lane brings its better cell (has, v, cell; lanes hold cells in order, so the lowest lane among
// equal values holds the lowest cell). MIN: IEEE <, else >. Returns the winning lane or -1; v and cell become the winner's.
template <bool MIN>
__device__ __forceinline__ int monitor_wave_extreme(bool has, float &v, int &cell)
{
    float w = has ? v : (MIN ? __int_as_float(0x7f800000) : __int_as_float(0xff800000));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float q = __shfl_xor(w, o, 64);
        w = MIN ? (q < w ? q : w) : (q > w ? q : w);
    }
    const int lane = monitor_first_lane(has && v == w);              // == : -0.0 and +0.0 tie, the lowest cell takes it
    if (lane >= 0) {
        v = __shfl(v, lane, 64);
        cell = __shfl(cell, lane, 64);
    }
    return lane;
}

__global__ __launch_bounds__(256) void k_monitor_blocks(MonitorRecord *__restrict__ slab, const float *__restrict__ rho,
                                                        const float *__restrict__ vel, const uint8_t *__restrict__ obstacle,
                                                        const int32_t *__restrict__ meta, const int32_t *__restrict__ ref2int)
{
    struct WaveOut { double s0, s1; float lo, hi, v2; int c_lo, c_hi, c_v2, c_bad, n_fluid, n_bad; };
    __shared__ WaveOut part[4];
    const int r = (int)blockIdx.x;
    const int64_t b = ref2int ? ref2int[r] : r;
    const int t = (int)threadIdx.x, c = 2 * t;
    const float2 rh = *(const float2 *)(rho + b * CELLS + c);
    const float *v = vel + b * 3 * CELLS + c;
    const float2 vx = *(const float2 *)v, vy = *(const float2 *)(v + CELLS), vz = *(const float2 *)(v + 2 * CELLS);
    const uchar2 ob = *(const uchar2 *)(obstacle + b * CELLS + c);
    const float q0 = (vx.x * vx.x + vy.x * vy.x) + vz.x * vz.x, q1 = (vx.y * vx.y + vy.y * vy.y) + vz.y * vz.y;
    const bool f0 = ob.x == 0, f1 = ob.y == 0;
    const bool k0 = f0 && monitor_finite(rh.x) && monitor_finite(vx.x) && monitor_finite(vy.x) && monitor_finite(vz.x) && monitor_finite(q0);
    const bool k1 = f1 && monitor_finite(rh.y) && monitor_finite(vx.y) && monitor_finite(vy.y) && monitor_finite(vz.y) && monitor_finite(q1);
    const bool bad0 = f0 && !k0, bad1 = f1 && !k1, has = k0 || k1;
    // the lane's own pair: the first halving of the sums, the better of its two cells (the first one on a tie)
    const double s0 = monitor_wave_sum((k0 ? (double)rh.x : 0.0) + (k1 ? (double)rh.y : 0.0));
    const double s1 = monitor_wave_sum((k0 ? (double)rh.x * (double)q0 : 0.0) + (k1 ? (double)rh.y * (double)q1 : 0.0));
    const bool lo1 = k1 && (!k0 || rh.y < rh.x), hi1 = k1 && (!k0 || rh.y > rh.x), v21 = k1 && (!k0 || q1 > q0);
    float lo = lo1 ? rh.y : rh.x, hi = hi1 ? rh.y : rh.x, v2 = v21 ? q1 : q0;
    int c_lo = c + (lo1 ? 1 : 0), c_hi = c + (hi1 ? 1 : 0), c_v2 = c + (v21 ? 1 : 0);
    const int l_lo = monitor_wave_extreme<true>(has, lo, c_lo);
    monitor_wave_extreme<false>(has, hi, c_hi);
    monitor_wave_extreme<false>(has, v2, c_v2);
    const int l_bad = monitor_first_lane(bad0 || bad1);
    int c_bad = c + (bad0 ? 0 : 1);
    if (l_bad >= 0) c_bad = __shfl(c_bad, l_bad, 64);
    const int n_fluid = __popcll(__ballot(f0)) + __popcll(__ballot(f1)), n_bad = __popcll(__ballot(bad0)) + __popcll(__ballot(bad1));
    if ((t & 63) == 0) {
        WaveOut &w = part[t >> 6];
        w.s0 = s0; w.s1 = s1; w.lo = lo; w.hi = hi; w.v2 = v2;
        w.c_lo = l_lo >= 0 ? c_lo : -1; w.c_hi = l_lo >= 0 ? c_hi : -1; w.c_v2 = l_lo >= 0 ? c_v2 : -1;   // one `has` for all three
        w.c_bad = l_bad >= 0 ? c_bad : -1;
        w.n_fluid = n_fluid; w.n_bad = n_bad;
    }
    __syncthreads();
    if (t != 0) return;
    const int32_t *row = meta + b * NBR_STRIDE;
    const unsigned long long base = monitor_block_key(row[NBR_BX], row[NBR_BY], row[NBR_BZ]);
    MonitorRecord o = monitor_empty();
    o.sum_rho = (part[0].s0 + part[1].s0) + (part[2].s0 + part[3].s0);
    o.sum_rho_v2 = (part[0].s1 + part[1].s1) + (part[2].s1 + part[3].s1);
    int c0 = -1, c1 = -1, c2 = -1, cb = -1;
#pragma unroll
    for (int w = 0; w < 4; ++w) {                                    // waves in cell order: a strict comparison keeps the lowest cell
        const WaveOut &p = part[w];
        o.n_fluid += p.n_fluid; o.n_bad += p.n_bad;
        if (p.c_lo >= 0) {
            if (c0 < 0 || p.lo < o.rho_min) { o.rho_min = p.lo; c0 = p.c_lo; }
            if (c1 < 0 || p.hi > o.rho_max) { o.rho_max = p.hi; c1 = p.c_hi; }
            if (c2 < 0 || p.v2 > o.v2_max) { o.v2_max = p.v2; c2 = p.c_v2; }
        }
        if (cb < 0) cb = p.c_bad;
    }
    o.key_rho_min = c0 >= 0 ? base + (unsigned)c0 : MONITOR_NO_KEY;
    o.key_rho_max = c1 >= 0 ? base + (unsigned)c1 : MONITOR_NO_KEY;
    o.key_v2_max = c2 >= 0 ? base + (unsigned)c2 : MONITOR_NO_KEY;
    o.key_bad = cb >= 0 ? base + (unsigned)cb : MONITOR_NO_KEY;
    slab[r] = o;
}

// one extreme over the records of a wave: the value by IEEE < / >, among equal values the lowest key
template <bool MIN>
__device__ __forceinline__ void monitor_wave_extreme_keyed(float &v, unsigned long long &key)
{
    const bool has = key != MONITOR_NO_KEY;
    float w = has ? v : (MIN ? __int_as_float(0x7f800000) : __int_as_float(0xff800000));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float q = __shfl_xor(w, o, 64);
        w = MIN ? (q < w ? q : w) : (q > w ? q : w);
    }
    unsigned long long k = (has && v == w) ? key : MONITOR_NO_KEY;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long q = __shfl_xor(k, o, 64);
        k = q < k ? q : k;
    }
    const int lane = monitor_first_lane(has && key == k);
    if (lane >= 0) v = __shfl(v, lane, 64);                          // the winner's own value (the sign of a zero)
    else v = w;
    key = k;
}
template <bool MIN>
__device__ __forceinline__ void monitor_take(float &v, unsigned long long &key, float v2, unsigned long long key2)
{
    if (key2 == MONITOR_NO_KEY) return;
    if (key == MONITOR_NO_KEY || (MIN ? v2 < v : v2 > v) || (v2 == v && key2 < key)) { v = v2; key = key2; }
}

__global__ __launch_bounds__(256) void k_monitor_combine(MonitorRecord *__restrict__ out, const MonitorRecord *__restrict__ in, int64_t n)
{
    __shared__ MonitorRecord part[4];
    const int t = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * CELLS + 2 * t;
    MonitorRecord a = monitor_empty(), b = a;
    if (i < n) a = in[i];
    if (i + 1 < n) b = in[i + 1];
    a.sum_rho = monitor_wave_sum(a.sum_rho + b.sum_rho);
    a.sum_rho_v2 = monitor_wave_sum(a.sum_rho_v2 + b.sum_rho_v2);
    a.n_fluid += b.n_fluid; a.n_bad += b.n_bad;
    a.key_bad = b.key_bad < a.key_bad ? b.key_bad : a.key_bad;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        a.n_fluid += __shfl_xor(a.n_fluid, o, 64);
        a.n_bad += __shfl_xor(a.n_bad, o, 64);
        const unsigned long long q = __shfl_xor(a.key_bad, o, 64);
        a.key_bad = q < a.key_bad ? q : a.key_bad;
    }
    monitor_take<true>(a.rho_min, a.key_rho_min, b.rho_min, b.key_rho_min);
    monitor_take<false>(a.rho_max, a.key_rho_max, b.rho_max, b.key_rho_max);
    monitor_take<false>(a.v2_max, a.key_v2_max, b.v2_max, b.key_v2_max);
    monitor_wave_extreme_keyed<true>(a.rho_min, a.key_rho_min);
    monitor_wave_extreme_keyed<false>(a.rho_max, a.key_rho_max);
    monitor_wave_extreme_keyed<false>(a.v2_max, a.key_v2_max);
    if ((t & 63) == 0) part[t >> 6] = a;
    __syncthreads();
    if (t != 0) return;
    MonitorRecord o = part[0];
    o.sum_rho = (part[0].sum_rho + part[1].sum_rho) + (part[2].sum_rho + part[3].sum_rho);
    o.sum_rho_v2 = (part[0].sum_rho_v2 + part[1].sum_rho_v2) + (part[2].sum_rho_v2 + part[3].sum_rho_v2);
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const MonitorRecord &p = part[w];
        o.n_fluid += p.n_fluid; o.n_bad += p.n_bad;
        o.key_bad = p.key_bad < o.key_bad ? p.key_bad : o.key_bad;
        monitor_take<true>(o.rho_min, o.key_rho_min, p.rho_min, p.key_rho_min);
        monitor_take<false>(o.rho_max, o.key_rho_max, p.rho_max, p.key_rho_max);
        monitor_take<false>(o.v2_max, o.key_v2_max, p.v2_max, p.key_v2_max);
    }
    out[blockIdx.x] = o;
}

// ---- force series (ludwig_force_series_*; the nine sums of integrate_forces_kernel!, reference src/forces/surface.jl:282-366, per
// sampled coarse step) ----
// Triangle i reads cell[i] (internal block * 512 + cell, -1: none) and rec = [8][n] floats: wall distance, normal x, y, z, area, arm x,
// y, z. Per triangle, float32 with -ffp-contract=off: p, tau from wall_stress (zeros without a cell), dFp_j = ((-p) n_j) A,
// dFv_j = tau_j A, dF = dFp + dFv, dM = arm x dF in the operand order of forces.partial_force_sums; covered = (double)|p| > 1e-10,
// the reference's Float64 comparison (src/forces/surface.jl:430: float32(1e-10) itself counts). The nine
// values are widened to double and summed in ONE balanced tree over the triangles in the caller's order: adjacent pairs halved, +0.0
// where a length is odd, and no addition once one value is left - the tree over the triangles padded with +0.0 to the next power of
// two (forces.tree_sum_f64). A level of the tree that joins nodes of `half` elements adds iff count > half: below that the right-hand
// node is padding and the halving has already ended, so a total of -0.0 keeps its sign.
// k_force_chunks: one workgroup per 512 consecutive triangles, two per lane (tree level 1), an xor-butterfly over the wave, the four
// waves through LDS; one ForceRecord per chunk with plain stores. k_force_combine: 512 records -> 1 per workgroup and launch, until
// one is left; missing records are +0.0. No atomics.
struct ForceRecord {
    double s[9];                   // Fp(3), Fv(3), M(3)
    long long covered;
};
constexpr int FORCE_REC_ROWS = 8;
// the butterfly over a wave whose lanes each hold the sum of 2 elements of `count` (whole tree): lane 0 of each aligned group of 2^k
// lanes ends with the group's node; every lane takes part in every shuffle
__device__ __forceinline__ double force_wave_sum(double x, int64_t count)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double q = __shfl_xor(x, o, 64);
        if (count > 2 * o) x += q;
    }
    return x;
}
// the four wave nodes (128 elements each) of a workgroup -> its node
__device__ __forceinline__ double force_join_waves(double p0, double p1, double p2, double p3, int64_t count)
{
    const double a = count > 128 ? p0 + p1 : p0, b = p2 + p3;
    return count > 256 ? a + b : a;
}
__device__ __forceinline__ bool force_contributions(float c[9], int64_t i, int64_t n, const int32_t *__restrict__ cell,
                                                    const float *__restrict__ rec, const float *__restrict__ rho,
                                                    const float *__restrict__ vel, float tau, float pressure_scale, float stress_scale)
{
    const int32_t cc = cell[i];
    const float nx = rec[n + i], ny = rec[2 * n + i], nz = rec[3 * n + i], A = rec[4 * n + i];
    const float rx = rec[5 * n + i], ry = rec[6 * n + i], rz = rec[7 * n + i];
    float p = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (cc >= 0) {
        const int64_t b = cc >> 9, x = cc & 511;
        const float *v = vel + b * (3 * CELLS) + x;
        wall_stress(rho[cc], v[0], v[CELLS], v[2 * CELLS], nx, ny, nz, rec[i], tau, pressure_scale, stress_scale, p, sx, sy, sz);
    }
    c[0] = ((-p) * nx) * A; c[1] = ((-p) * ny) * A; c[2] = ((-p) * nz) * A;
    c[3] = sx * A; c[4] = sy * A; c[5] = sz * A;
    const float fx = c[0] + c[3], fy = c[1] + c[4], fz = c[2] + c[5];
    c[6] = ry * fz - rz * fy; c[7] = rz * fx - rx * fz; c[8] = rx * fy - ry * fx;
    return (double)fabsf(p) > 1.0e-10;
}

// The four waves of a workgroup through LDS: a.s = every wave's node, count = its integer count -> the caller's lane 0 (true) holds
// the workgroup's node in `a`. part / pc: LDS.
template <typename Rec, int ROWS, long long Rec::*CNT, typename PC>
__device__ __forceinline__ bool tree_join_waves(Rec &a, PC count, int64_t n, double (*part)[ROWS], PC *pc)
{
    const int t = (int)threadIdx.x;
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < ROWS; ++k) part[t >> 6][k] = a.s[k];
        pc[t >> 6] = count;
    }
    __syncthreads();
    if (t != 0) return false;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) a.s[k] = force_join_waves(part[0][k], part[1][k], part[2][k], part[3][k], n);
    a.*CNT = (long long)((pc[0] + pc[1]) + (pc[2] + pc[3]));
    return true;
}
// One workgroup's node of a tree of records {double s[ROWS]; long long <CNT>;} (the force series' and the flux planes'): records
// in[chunk * 512 ..] of n -> the caller's lane 0 (true) holds their node in `a`; missing records are +0.0. part / pc: LDS.
template <typename Rec, int ROWS, long long Rec::*CNT>
__device__ __forceinline__ bool tree_combine(Rec &a, const Rec *__restrict__ in, int64_t n, int64_t chunk, double (*part)[ROWS], long long *pc)
{
    const int t = (int)threadIdx.x;
    const int64_t i = chunk * CELLS + 2 * t;
    Rec b;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) a.s[k] = b.s[k] = 0.0;
    a.*CNT = b.*CNT = 0;
    if (i < n) a = in[i];
    if (i + 1 < n) b = in[i + 1];
    a.*CNT += b.*CNT;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) a.*CNT += __shfl_xor(a.*CNT, o, 64);
#pragma unroll
    for (int k = 0; k < ROWS; ++k) a.s[k] = force_wave_sum(n > 1 ? a.s[k] + b.s[k] : a.s[k], n);
    return tree_join_waves<Rec, ROWS, CNT>(a, a.*CNT, n, part, pc);
}
// The leaf level of the same tree: elements chunk * 512 .. of n, two per lane (tree level 1). fill(c, i) forms the ROWS float values
// of element i and says whether it counts; they are widened to double here. A missing element is +0.0 and does not count.
template <typename Rec, int ROWS, long long Rec::*CNT, class FILL>
__device__ __forceinline__ bool tree_leaf(Rec &a, int64_t n, int64_t chunk, double (*part)[ROWS], int *pc, FILL fill)
{
    const int64_t i = chunk * CELLS + 2 * (int)threadIdx.x;
    float c0[ROWS], c1[ROWS];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) c0[k] = c1[k] = 0.0f;
    bool k0 = false, k1 = false;
    if (i < n) k0 = fill(c0, i);
    if (i + 1 < n) k1 = fill(c1, i + 1);
    const int counted = __popcll(__ballot(k0)) + __popcll(__ballot(k1));
#pragma unroll
    for (int k = 0; k < ROWS; ++k) a.s[k] = force_wave_sum(n > 1 ? (double)c0[k] + (double)c1[k] : (double)c0[k], n);
    return tree_join_waves<Rec, ROWS, CNT>(a, counted, n, part, pc);
}

__global__ __launch_bounds__(256) void k_force_chunks(ForceRecord *__restrict__ slab, const int32_t *__restrict__ cell,
                                                      const float *__restrict__ rec, int n, const float *__restrict__ rho,
                                                      const float *__restrict__ vel, float tau, float pressure_scale, float stress_scale)
{
    __shared__ double part[4][9];
    __shared__ int cov[4];
    const int64_t N = n;
    ForceRecord o;
    const auto fill = [&](float (&c)[9], int64_t i) { return force_contributions(c, i, N, cell, rec, rho, vel, tau, pressure_scale, stress_scale); };
    if (tree_leaf<ForceRecord, 9, &ForceRecord::covered>(o, N, (int64_t)blockIdx.x, part, cov, fill)) slab[blockIdx.x] = o;
}

__global__ __launch_bounds__(256) void k_force_combine(ForceRecord *__restrict__ out, const ForceRecord *__restrict__ in, int64_t n)
{
    __shared__ double part[4][9];
    __shared__ long long cov[4];
    ForceRecord o;
    if (tree_combine<ForceRecord, 9, &ForceRecord::covered>(o, in, n, (int64_t)blockIdx.x, part, cov)) out[blockIdx.x] = o;
}

// ---- flux planes (ludwig_flux_planes_*; no reference counterpart) ----
// The points of one level lie in lists, one per (plane, level) pair that holds any: the plane's valid points on that level in point
// order. Point p has the probes' stencil: cell[8 p + c] = internal block * 512 + cell of corner c (a corner that is no fluid cell
// already replaced by the base cell), w[3 p + a] the weights. Per point, float32 with -ffp-contract=off: rho, ux, uy, uz by the probes'
// trilinear rule (probe_lerp: x, then y, then z), un = u[axis], m = rho * un, q = (ux ux + uy uy) + uz uz and the eight rows rho, un,
// m, m ux, m uy, m uz, rho q, m q. Each row is widened to double and summed over its list in the force series' balanced tree
// (force_wave_sum, force_join_waves: "add iff count > half"), the count of points is an integer sum. No atomics.
// A FluxChunk is one workgroup's work in either kernel: elements start + 512 chunk .. of a list of n - points of the level's
// arrays in k_flux_chunks, records of the slab in k_flux_combine - reduce to one record, written to slab[dst] or, where dst < 0 (the
// list's last stage), to the ring slot's record ~dst.
struct FluxRecord {
    double s[8];                   // sums of rho, un, m, m ux, m uy, m uz, rho q, m q
    long long count;
};
struct FluxChunk {
    int32_t start, n, chunk, dst, axis, pad;
};
constexpr int FLUX_ROWS = 8;

__device__ __forceinline__ void flux_contributions(float c[FLUX_ROWS], int64_t p, int axis, const int32_t *__restrict__ cell,
                                                   const float *__restrict__ w, const float *__restrict__ rho,
                                                   const float *__restrict__ vel)
{
    float res[4];
    stencil_sample(res, p, cell, w, rho, vel);
    const float r = res[0], ux = res[1], uy = res[2], uz = res[3];
    const float un = axis == 0 ? ux : (axis == 1 ? uy : uz);
    const float m = r * un;
    const float q = (ux * ux + uy * uy) + uz * uz;
    c[0] = r; c[1] = un; c[2] = m; c[3] = m * ux; c[4] = m * uy; c[5] = m * uz; c[6] = r * q; c[7] = m * q;
}

__device__ __forceinline__ void flux_store(FluxRecord *__restrict__ slab, FluxRecord *__restrict__ slot, int32_t dst, const FluxRecord &o)
{
    FluxRecord *out = dst >= 0 ? slab + dst : slot + ~dst;
    *out = o;
}

__global__ __launch_bounds__(256) void k_flux_chunks(FluxRecord *__restrict__ slab, FluxRecord *__restrict__ slot,
                                                     const FluxChunk *__restrict__ chunks, const int32_t *__restrict__ cell,
                                                     const float *__restrict__ w, const float *__restrict__ rho,
                                                     const float *__restrict__ vel)
{
    __shared__ double part[4][FLUX_ROWS];
    __shared__ int cnt[4];
    const FluxChunk d = chunks[blockIdx.x];
    FluxRecord o;
    const auto fill = [&](float (&c)[FLUX_ROWS], int64_t i) { flux_contributions(c, d.start + i, d.axis, cell, w, rho, vel); return true; };
    if (tree_leaf<FluxRecord, FLUX_ROWS, &FluxRecord::count>(o, d.n, d.chunk, part, cnt, fill)) flux_store(slab, slot, d.dst, o);
}

__global__ __launch_bounds__(256) void k_flux_combine(FluxRecord *__restrict__ slab, FluxRecord *__restrict__ slot,
                                                      const FluxChunk *__restrict__ chunks)
{
    __shared__ double part[4][FLUX_ROWS];
    __shared__ long long cnt[4];
    const FluxChunk d = chunks[blockIdx.x];
    FluxRecord o;
    if (tree_combine<FluxRecord, FLUX_ROWS, &FluxRecord::count>(o, slab + d.start, d.n, d.chunk, part, cnt)) flux_store(slab, slot, d.dst, o);
}

// ---- wall diagnostics (ludwig_level_wall_census, ludwig_wall_surface_*; no reference counterpart: the reference reads y_plus_target
// and never computes a y+) ----
// The state wall_model_force_mag passes through on its way to the force: a second copy of its chain (same operand order, jl_pow / jl_log,
// -ffp-contract=off), and the one formula this file still holds twice. Every form with one body for both - a template on "wants the
// state", a core the two call - cost the step's function two instructions and the order of two compares ("Single
// source"), and the step's machine code is not traded for source. A change to one goes into the other.
// code: WALL_FAR not near the wall (!(0 < d < 10)), WALL_SKIPPED near the wall but the model is skipped (u_mag <= 1e-6 or
// nu_visc <= 1e-10), WALL_POWER the power law's u_tau is kept (y_p <= 11.81 or u_plus_law <= 0.1), WALL_LOG the log law replaced it;
// WALL_FORCED is or-ed in where the step applies a force (tau_wall > tau_res). y_plus is the FINAL u_tau * dist_wall / nu_visc, not the
// provisional y_p that picks the branch. Codes below WALL_POWER give zeros.
constexpr int WALL_FAR = 0, WALL_SKIPPED = 1, WALL_POWER = 2, WALL_LOG = 3, WALL_FORCED = 4;
struct WallState {
    float u_tau, y_plus;
    int code;
};
__device__ __forceinline__ WallState wall_model_state(float dist_wall, float tau_molecular, float rho, float u_mag)
{
    WallState s;
    s.u_tau = 0.0f; s.y_plus = 0.0f; s.code = WALL_FAR;
    if (dist_wall > 0.0f && dist_wall < 10.0f) {
        s.code = WALL_SKIPPED;
        const float nu_visc = (tau_molecular - 0.5f) / 3.0f;
        if (u_mag > 1.0e-6f && nu_visc > 1.0e-10f) {
            float u_tau = u_mag * jl_pow(nu_visc / (dist_wall * u_mag + 1.0e-10f), 1.0f / 7.0f) *
                          jl_pow(2.0f * 8.3f, -1.0f / 7.0f);
            u_tau = jl_max(u_tau, 1.0e-6f);
            const float y_p = u_tau * dist_wall / nu_visc;
            s.code = WALL_POWER;
            if (y_p > 11.81f) {
                const float u_plus_law = (1.0f / KAPPA) * jl_log(y_p) + 5.2f;
                if (u_plus_law > 0.1f) {
                    u_tau = u_tau * ((u_mag / u_tau) / u_plus_law);
                    u_tau = jl_max(u_tau, 1.0e-6f);
                    s.code = WALL_LOG;
                }
            }
            const float tau_wall = rho * u_tau * u_tau;
            const float tau_res = rho * nu_visc * (u_mag / dist_wall);
            if (tau_wall > tau_res) s.code |= WALL_FORCED;
            s.u_tau = u_tau;
            s.y_plus = u_tau * dist_wall / nu_visc;
        }
    }
    return s;
}

// The census of one level: LudwigWallCensus of include/ludwig_hip.h, all integers. A cell is NEAR when it is no obstacle cell and
// 0 < wall_dist < 10; EVALUATED when the model ran (code >= WALL_POWER) and both its y+ and its wall shear rho u_tau u_tau are finite,
// NON_FINITE when the model ran and one of them is not (such a cell counts there and, NEAR apart, nowhere else). min / max are the float32
// bits of y+ over the evaluated cells - y+ is positive there, and positive floats order as unsigned integers. The histogram's bin is a
// shift of those bits: e8 = bits >> 20 is the exponent with the top three mantissa bits, eight bins per octave; bin 0 below 2^-10,
// bin 193 from 2^14 on. Integer sums commute: the record depends on neither block order, workgroup scheduling nor a rank's cut.
constexpr int WALL_BINS = 194, WALL_E8_FIRST = 936, WALL_E8_END = 1128;
struct WallCensusRecord {
    unsigned long long near_cells, evaluated, log_law, forced, non_finite;
    uint32_t min_bits, max_bits;
    unsigned long long hist[WALL_BINS];
};
__device__ __forceinline__ int wall_bin_of_bits(uint32_t bits)
{
    const int e8 = (int)(bits >> 20);
    return e8 < WALL_E8_FIRST ? 0 : (e8 >= WALL_E8_END ? WALL_BINS - 1 : 1 + (e8 - WALL_E8_FIRST));
}

// One workgroup per owned block (internal order: the owned blocks come first), two x-consecutive cells per lane; a block without
// FLAG_HAS_NEAR_WALL leaves at once (the whole workgroup: no barrier is skipped by a part of it). Counts in LDS, then the non-zero
// entries go to the global record with integer atomics. 21 B per cell of a flagged block.
__global__ __launch_bounds__(256) void k_wall_census(WallCensusRecord *__restrict__ rec, const float *__restrict__ rho,
                                                     const float *__restrict__ vel, const uint8_t *__restrict__ obstacle,
                                                     const float *__restrict__ wall_dist, const int32_t *__restrict__ meta, float tau)
{
    constexpr int N_NEAR = WALL_BINS, N_EVAL = WALL_BINS + 1, N_LOG = WALL_BINS + 2, N_FORCED = WALL_BINS + 3, N_BAD = WALL_BINS + 4,
                  N_COUNTS = WALL_BINS + 5;
    __shared__ uint32_t count[N_COUNTS];
    __shared__ uint32_t ext[2];
    const int64_t b = (int64_t)blockIdx.x;
    if (!(meta[b * NBR_STRIDE + NBR_FLAGS] & FLAG_HAS_NEAR_WALL)) return;
    const int t = (int)threadIdx.x, c = 2 * t;
    if (t < N_COUNTS) count[t] = 0u;
    if (t == 0) { ext[0] = 0xFFFFFFFFu; ext[1] = 0u; }
    __syncthreads();
    const float2 wd = *(const float2 *)(wall_dist + b * CELLS + c);
    const uchar2 ob = *(const uchar2 *)(obstacle + b * CELLS + c);
    const float2 rh = *(const float2 *)(rho + b * CELLS + c);
    const float *v = vel + b * 3 * CELLS + c;
    const float2 vx = *(const float2 *)v, vy = *(const float2 *)(v + CELLS), vz = *(const float2 *)(v + 2 * CELLS);
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {                                     // one copy of the double-precision pow / log for both cells
        const float d = j ? wd.y : wd.x;
        if ((j ? ob.y : ob.x) != 0 || !(d > 0.0f && d < 10.0f)) continue;
        atomicAdd(&count[N_NEAR], 1u);
        const float ux = j ? vx.y : vx.x, uy = j ? vy.y : vy.x, uz = j ? vz.y : vz.x, r = j ? rh.y : rh.x;
        const WallState s = wall_model_state(d, tau, r, sqrtf(ux * ux + uy * uy + uz * uz));
        if ((s.code & 3) < WALL_POWER) continue;
        if (!monitor_finite(s.y_plus) || !monitor_finite(r * s.u_tau * s.u_tau)) {
            atomicAdd(&count[N_BAD], 1u);
            continue;
        }
        const uint32_t bits = __float_as_uint(s.y_plus);
        atomicAdd(&count[N_EVAL], 1u);
        if ((s.code & 3) == WALL_LOG) atomicAdd(&count[N_LOG], 1u);
        if (s.code & WALL_FORCED) atomicAdd(&count[N_FORCED], 1u);
        atomicAdd(&count[wall_bin_of_bits(bits)], 1u);
        atomicMin(&ext[0], bits);
        atomicMax(&ext[1], bits);
    }
    __syncthreads();
    if (t < N_COUNTS) {
        const uint32_t n = count[t];
        if (n) {
            // the record as 200 eight-byte words: five counters, the min / max pair, the histogram
            unsigned long long *words = reinterpret_cast<unsigned long long *>(rec);
            atomicAdd(words + (t < WALL_BINS ? 6 + t : t - WALL_BINS), (unsigned long long)n);
        }
    }
    if (t == 0 && count[N_EVAL]) {
        atomicMin(&rec->min_bits, ext[0]);
        atomicMax(&rec->max_bits, ext[1]);
    }
}

// One lane per triangle of a wall-surface set: out = [WALL_SURFACE_ROWS][n] floats p, tau_model_x, tau_model_y, tau_model_z, u_tau,
// y_plus, code. cell[i] = internal block * 512 + cell of the triangle's nearest fluid cell (-1: none), nrm = [3][n]. p and the
// tangential direction are wall_stress's expressions; the wall distance is the LEVEL's wall_dist at the cell (what the step used), not
// the triangle's own; the shear is (rho u_tau u_tau) stress_scale along the tangential velocity, zero where umag <= 1e-10 or the model
// did not run. A triangle without a cell gives the p of rho = 1 and zeros.
constexpr int WALL_SURFACE_ROWS = 7;
__global__ __launch_bounds__(256) void k_wall_surface(float *__restrict__ out, const int32_t *__restrict__ cell, const float *__restrict__ nrm,
                                                      int n, const float *__restrict__ rho, const float *__restrict__ vel,
                                                      const uint8_t *__restrict__ obstacle, const float *__restrict__ wall_dist, float tau,
                                                      float pressure_scale, float stress_scale)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int32_t c = cell[i];
    float r = 1.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    WallState s;
    s.u_tau = 0.0f; s.y_plus = 0.0f; s.code = WALL_FAR;
    if (c >= 0) {
        const int64_t b = c >> 9, cc = c & 511;
        const float *v = vel + b * (3 * CELLS) + cc;
        const float ux = v[0], uy = v[CELLS], uz = v[2 * CELLS], nx = nrm[i], ny = nrm[n + i], nz = nrm[2 * n + i];
        r = rho[c];
        if (obstacle[c] == 0) s = wall_model_state(wall_dist[c], tau, r, sqrtf(ux * ux + uy * uy + uz * uz));
        const float udn = ux * nx + uy * ny + uz * nz;
        const float utx = ux - udn * nx, uty = uy - udn * ny, utz = uz - udn * nz;
        const float umag = sqrtf(utx * utx + uty * uty + utz * utz);
        if (umag > 1.0e-10f && (s.code & 3) >= WALL_POWER) {
            const float tmag = (r * s.u_tau * s.u_tau) * stress_scale;
            sx = (utx / umag) * tmag; sy = (uty / umag) * tmag; sz = (utz / umag) * tmag;
        }
    }
    const int64_t N = n;
    float *o = out + i;
    o[0] = ((r - 1.0f) / 3.0f) * pressure_scale;
    o[N] = sx; o[2 * N] = sy; o[3 * N] = sz;
    o[4 * N] = s.u_tau; o[5 * N] = s.y_plus; o[6 * N] = (float)s.code;
}

// ---- warm start (ludwig_level_init_from_source; no reference counterpart; include/ludwig_hip.h states the definition and
// open_ludwig_amd/warm_start.py restates it in numpy bit for bit) ----
// A level filled from another hierarchy's rho and u, the populations at their equilibrium. One workgroup of 256 lanes per destination
// block, two phases:
//   sample: the block's 512 cells in 16 rounds of 32, one group of eight lanes per cell - stream_sample's mapping, unchanged: the lanes
//           of a group form the same P from the same words, so they run the same control flow and a shuffle meets its partners; every
//           group of every round samples (512 = 16 x 32: no lane leaves early). Lane 0 of the group classifies the cell, scales or
//           replaces the values and leaves rho', u' in LDS (8 KiB); the outcome counters are integer adds in LDS, then one integer
//           atomic per non-zero counter and block - sums of integers, so the counts depend on no scheduling.
//   store:  the pass is write-bound - 244 B per cell (27 + 27 populations, 3 + 3 velocities, rho), 368 B with the saved state - so
//           every store is the widest there is: a lane holds four x-consecutive cells and writes 16 B, 128 lanes cover one component
//           of the block (2 KiB contiguous, 1 KiB per wave instruction). The two halves of the workgroup share the components: half h
//           evaluates and stores the populations k with k % 2 == h into every population array; half 0 stores vel, rho and rho_old,
//           half 1 vel_temp and vel_old. The halves are whole waves: the choice is wave-uniform.
// Writes: this block's 512 cells of the level's own arrays (block = blockIdx.x < n_blocks, the grid's size) and counts[0 .. 4 +
// n_levels - 1]. The source is only read, through stream_sample's checked indices.
constexpr int WARM_OUTCOMES = 4;                 // found, outside, source obstacle, non-finite
constexpr int WARM_MAX_LEVELS = 30;
struct WarmArgs {
    StreamArgs s;                // lv, n_levels of the source, temp_mask 0; the rest unused
    const int32_t *meta;         // destination: [n_blocks][NBR_STRIDE]
    const uint8_t *obstacle;     // destination: [block][512]
    float *f[3];                 // f, f_temp, f_old (null without temporal storage)
    float *vel[3];               // vel, vel_temp, vel_old (null without)
    float *rho[2];               // rho, rho_old (null without)
    float map[6];                // a_x, a_y, a_z, b_x, b_y, b_z
    float scale;
    float fallback[4];
    unsigned long long *counts;  // [4 + n_levels], null: not wanted
};

__global__ __launch_bounds__(256) void k_init_from_source(const WarmArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_q[4][CELLS];
    __shared__ unsigned s_n[WARM_OUTCOMES + WARM_MAX_LEVELS];
    const int t = (int)threadIdx.x;
    const int64_t blk = blockIdx.x;
    if (t < WARM_OUTCOMES + WARM_MAX_LEVELS) s_n[t] = 0u;
    __syncthreads();
    const int32_t *row = a.meta + blk * NBR_STRIDE;
    const int ox = 8 * (row[NBR_BX] - 1), oy = 8 * (row[NBR_BY] - 1), oz = 8 * (row[NBR_BZ] - 1);
    {
        const int c = t & 7, grp = t >> 3;
        const StreamLevel mine = a.s.lv[max(a.s.n_levels - 1 - c, 0)];
        const float s2 = a.scale * a.scale;
        for (int r = 0; r < CELLS / 32; ++r) {
            const int cell = r * 32 + grp;
            const int x = cell & 7, y = (cell >> 3) & 7, z = cell >> 6;
            const float px = a.map[0] * ((float)(ox + x) + 0.5f) + a.map[3];
            const float py = a.map[1] * ((float)(oy + y) + 0.5f) + a.map[4];
            const float pz = a.map[2] * ((float)(oz + z) + 0.5f) + a.map[5];
            float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            int li = 0;
            const int code = stream_sample(a.s, mine, c, px, py, pz, q, li);
            if (c == 0) {
                float o[4] = {a.fallback[0], a.fallback[1], a.fallback[2], a.fallback[3]};
                int slot = code;                                     // 1 outside, 2 source obstacle
                if (code == 0) {
                    const bool finite = __builtin_isfinite(q[0]) && __builtin_isfinite(q[1]) && __builtin_isfinite(q[2]) &&
                                        __builtin_isfinite(q[3]);
                    slot = finite ? 0 : 3;
                    if (finite) {
                        o[0] = 1.0f + (q[0] - 1.0f) * s2;
                        o[1] = q[1] * a.scale;
                        o[2] = q[2] * a.scale;
                        o[3] = q[3] * a.scale;
                    }
                }
                if (a.obstacle[blk * CELLS + cell]) {
                    o[0] = 1.0f; o[1] = 0.0f; o[2] = 0.0f; o[3] = 0.0f;
                } else if (a.counts) {
                    atomicAdd(&s_n[slot], 1u);
                    if (slot == 0) atomicAdd(&s_n[WARM_OUTCOMES + li], 1u);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) s_q[k][cell] = o[k];
            }
        }
    }
    __syncthreads();
    if (a.counts && t < WARM_OUTCOMES + a.s.n_levels && s_n[t] != 0u) atomicAdd(a.counts + t, (unsigned long long)s_n[t]);
    const int h = t >> 7, c4 = (t & 127) * 4;
    const float4 r4 = *(const float4 *)&s_q[0][c4], x4 = *(const float4 *)&s_q[1][c4], y4 = *(const float4 *)&s_q[2][c4],
                 z4 = *(const float4 *)&s_q[3][c4];
    static_for<0, Q>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if ((k & 1) == h) {
            constexpr float w = WEIGHT(k), cx = (float)CX(k), cy = (float)CY(k), cz = (float)CZ(k);
            float4 e;
            e.x = calculate_equilibrium(r4.x, x4.x, y4.x, z4.x, w, cx, cy, cz);
            e.y = calculate_equilibrium(r4.y, x4.y, y4.y, z4.y, w, cx, cy, cz);
            e.z = calculate_equilibrium(r4.z, x4.z, y4.z, z4.z, w, cx, cy, cz);
            e.w = calculate_equilibrium(r4.w, x4.w, y4.w, z4.w, w, cx, cy, cz);
            const int64_t at = (blk * Q + k) * CELLS + c4;
#pragma unroll
            for (int m = 0; m < 3; ++m)
                if (a.f[m]) *(float4 *)(a.f[m] + at) = e;
        }
    });
    const int64_t vat = blk * 3 * CELLS + c4, sat = blk * CELLS + c4;
    auto store_vel = [&](float *v) {
        if (!v) return;
        *(float4 *)(v + vat) = x4;
        *(float4 *)(v + vat + CELLS) = y4;
        *(float4 *)(v + vat + 2 * CELLS) = z4;
    };
    if (h == 0) {
        store_vel(a.vel[0]);
        *(float4 *)(a.rho[0] + sat) = r4;
        if (a.rho[1]) *(float4 *)(a.rho[1] + sat) = r4;
    } else {
        store_vel(a.vel[1]);
        store_vel(a.vel[2]);
    }
}

}  // namespace lw
