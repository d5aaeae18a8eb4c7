# LudwigHIP.jl - the reference-side binding of libludwig_hip.so (include/ludwig_hip.h).
#
# Drop this file next to the reference's src/ and `include("LudwigHIP.jl")` after blocks.jl. It replaces, for an
# MI355X, the four device-facing calls of the hot path:
#     adapt(backend, level)                 (src/main.jl:98, src/blocks.jl:67-87)      -> LudwigHIP.adapt_level
#     perform_timestep_v2!(level, ...)      (src/physics_v2.jl:26-97)                   -> LudwigHIP.perform_timestep!
#     copy_to_old!(level, f_in, vel_in)     (src/blocks.jl:199-205)                     -> LudwigHIP.copy_to_old!
#     KernelAbstractions.synchronize        (src/solver_control.jl:164)                 -> LudwigHIP.synchronize
# NOT TESTED HERE: the build image has no Julia. It is a thin ccall layer; every struct mirrors include/ludwig_hip.h.
module LudwigHIP

const LIB = get(ENV, "LUDWIG_HIP_LIB", joinpath(@__DIR__, "..", "open_ludwig_amd", "csrc", "libludwig_hip.so"))

# enum LudwigField
const F, F_TEMP, F_POST, F_OLD, RHO, RHO_OLD, VEL, VEL_TEMP, VEL_OLD, OBSTACLE, SPONGE, WALL_DIST = Int32.(0:11)

struct LevelHost               # LudwigLevelHost
    level_id::Int32; n_blocks::Int32; n_owned::Int32; tau::Float32
    grid_dim_x::Int32; grid_dim_y::Int32; grid_dim_z::Int32
    block_pointer::Ptr{Int32}; neighbor_table::Ptr{Int32}
    map_x::Ptr{Int32}; map_y::Ptr{Int32}; map_z::Ptr{Int32}
    obstacle::Ptr{UInt8}; sponge::Ptr{Float32}; wall_dist::Ptr{Float32}
    enable_temporal_interpolation::Int32; n_boundary_cells::Int32
    bouzidi_q_map::Ptr{UInt16}; bouzidi_cell_block::Ptr{Int32}
    bouzidi_cell_x::Ptr{Int8}; bouzidi_cell_y::Ptr{Int8}; bouzidi_cell_z::Ptr{Int8}
    comm_boundary::Ptr{UInt8}
    store_post_collision_everywhere::Int32   # 0: f_post_collision only where the Bouzidi kernel reads it
end

struct StepFlags               # LudwigStepFlags
    domain_nx::Int32; domain_ny::Int32; domain_nz::Int32
    is_symmetric::Int32; wall_model_active::Int32; use_temporal_interp::Int32; sponge_blend_distributions::Int32
    c_wale::Float32; nu_sgs_background::Float32; inlet_turbulence::Float32; q_min_threshold::Float32
end

struct SurfaceParams           # LudwigSurfaceParams
    dx::Float32; tau::Float32
    offset_x::Float32; offset_y::Float32; offset_z::Float32
    pressure_scale::Float32; stress_scale::Float32
    search_radius::Int32
end

struct BatchSamplers           # LudwigBatchSamplers
    probes::Ptr{Cvoid}; probes_start_step::Int64; probes_interval::Int32
    surface::Ptr{Cvoid}; surface_start_step::Int64; surface_interval::Int32
end

const OBSERVE_PROBES, OBSERVE_SURFACE, OBSERVE_FORCES, OBSERVE_TRACERS, OBSERVE_FLUXES = Int32.(0:4)   # LUDWIG_OBSERVE_*
const OBSERVE_MODES = Int32(5)
struct BatchObserver           # LudwigBatchObserver
    kind::Int32; set::Ptr{Cvoid}; start_step::Int64; interval::Int32
end

mutable struct DeviceLevel
    handle::Ptr{Cvoid}
    level_id::Int; tau::Float32; n_blocks::Int
    has_temporal::Bool; bouzidi_enabled::Bool; n_boundary_cells::Int
end

last_error() = unsafe_string(ccall((:ludwig_last_error, LIB), Cstring, ()))
check(rc::Cint) = rc == 0 ? nothing : error("libludwig_hip error $rc: $(last_error())")

"""adapt(backend, level) for an MI355X: uploads every array of a host BlockLevel (src/blocks.jl:16-65)."""
function adapt_level(level, device::Integer = 0)
    n = length(level.active_block_coords)
    obstacle_u8 = Array{UInt8}(level.obstacle)
    GC.@preserve level obstacle_u8 begin
        h = LevelHost(Int32(level.level_id), Int32(n), Int32(0), level.tau,
                      Int32(size(level.block_pointer, 1)), Int32(size(level.block_pointer, 2)), Int32(size(level.block_pointer, 3)),
                      pointer(level.block_pointer), pointer(level.neighbor_table),
                      pointer(level.map_x), pointer(level.map_y), pointer(level.map_z),
                      pointer(obstacle_u8), pointer(level.sponge), pointer(level.wall_dist),
                      Int32(length(level.f_old) > 27), Int32(level.n_boundary_cells),
                      level.bouzidi_enabled ? Ptr{UInt16}(pointer(level.bouzidi_q_map)) : Ptr{UInt16}(C_NULL),
                      level.bouzidi_enabled ? pointer(level.bouzidi_cell_block) : Ptr{Int32}(C_NULL),
                      level.bouzidi_enabled ? pointer(level.bouzidi_cell_x) : Ptr{Int8}(C_NULL),
                      level.bouzidi_enabled ? pointer(level.bouzidi_cell_y) : Ptr{Int8}(C_NULL),
                      level.bouzidi_enabled ? pointer(level.bouzidi_cell_z) : Ptr{Int8}(C_NULL),
                      Ptr{UInt8}(C_NULL), Int32(0))
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:ludwig_level_create, LIB), Cint, (Ref{LevelHost}, Cint, Ref{Ptr{Cvoid}}), h, device, out))
        d = DeviceLevel(out[], level.level_id, level.tau, n, length(level.f_old) > 27, level.bouzidi_enabled, level.n_boundary_cells)
        for (fld, arr) in ((F, level.f), (F_TEMP, level.f_temp), (RHO, level.rho), (VEL, level.vel), (VEL_TEMP, level.vel_temp))
            upload!(d, fld, arr)
        end
        finalizer(x -> ccall((:ludwig_level_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.handle), d)
        return d
    end
end

upload!(d::DeviceLevel, field::Int32, a::Array) =
    GC.@preserve a check(ccall((:ludwig_level_upload, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Csize_t), d.handle, field, pointer(a), sizeof(a)))

"""Array(level.field): download into a preallocated host array of the reference's shape."""
download!(a::Array, d::DeviceLevel, field::Int32) =
    GC.@preserve a check(ccall((:ludwig_level_download, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Csize_t), d.handle, field, pointer(a), sizeof(a)))

"""init_eq! (src/main.jl:109-134)"""
init_equilibrium!(d::DeviceLevel) = check(ccall((:ludwig_init_equilibrium, LIB), Cint, (Ptr{Cvoid},), d.handle))

"""
perform_timestep_v2! (src/physics_v2.jl:26-97). The reference passes f_out/f_in/vel_out/vel_in explicitly; its only callers
(src/solver_control.jl:35-41) derive them from the parity of `timestep`, which is what the library does. `parent === nothing`
is level 1, exactly like `parent_f === nothing`.
"""
function perform_timestep!(d::DeviceLevel, parent::Union{DeviceLevel,Nothing}, parent_tau::Float32, u_curr::Float32,
                           flags::StepFlags, timestep::Integer, temporal_weight::Float32)
    p = parent === nothing ? C_NULL : parent.handle
    check(ccall((:ludwig_step, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cfloat, Cfloat, Cfloat, Ref{StepFlags}),
                d.handle, p, Int64(timestep), u_curr, parent_tau, temporal_weight, flags))
end

"""copy_to_old!(level, f_in, vel_in) for the step `timestep` about to run (src/blocks.jl:199-205)."""
copy_to_old!(d::DeviceLevel, timestep::Integer) = check(ccall((:ludwig_save_old, LIB), Cint, (Ptr{Cvoid}, Int64), d.handle, Int64(timestep)))

synchronize(d::DeviceLevel) = check(ccall((:ludwig_sync, LIB), Cint, (Ptr{Cvoid},), d.handle))

"""compute_flow_stats(level).rho_min (src/diagnostics.jl:56-94), reduced on the device."""
function rho_min(d::DeviceLevel)
    v = Ref{Cfloat}(0)
    check(ccall((:ludwig_level_rho_min, LIB), Cint, (Ptr{Cvoid}, Ref{Cfloat}), d.handle, v))
    return v[]
end

# record step (no reference counterpart): plain levels keep 11 collision values per cell between steps instead of f, vel and rho;
# LUDWIG_RECORD_STEP=0 in the environment turns it off, results never depend on it
"""how many of the level's steps so far went by records (0 on a level the rule excludes)"""
function record_steps(d::DeviceLevel)
    n = Ref{Int64}(0)
    check(ccall((:ludwig_level_record_steps, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), d.handle, n))
    return n[]
end
"""the rule as a function of what a level is: `flags` = the per-block flags words (1 = all neighbours present and nothing else)"""
function record_step_rule(flags::Vector{Int32}, n_owned::Integer; has_parent=false, has_temporal=false, has_post=false, wall_model=false)
    return ccall((:ludwig_record_step_rule, LIB), Cint, (Ptr{Int32}, Int32, Int32, Int32, Int32, Int32, Int32), flags, length(flags), n_owned,
                 has_parent, has_temporal, has_post, wall_model) == 1
end

# time-averaged statistics (no reference counterpart): double-precision sums of rho, u_i and u_i u_j over the owned cells
const STAT_RHO, STAT_VEL, STAT_VEL2 = Int32(0), Int32(1), Int32(2)      # K = 1, 3, 6 (xx, yy, zz, xy, yz, xz)
"""zero the sums (allocates them on the first call)"""
stats_reset!(d::DeviceLevel) = check(ccall((:ludwig_level_stats_reset, LIB), Cint, (Ptr{Cvoid},), d.handle))
"""add the newest state of the level after sub-step `timestep` (vel_temp if even, vel if odd; rho as stored)"""
stats_accumulate!(d::DeviceLevel, timestep::Integer) =
    check(ccall((:ludwig_level_stats_accumulate, LIB), Cint, (Ptr{Cvoid}, Int64), d.handle, Int64(timestep)))
"""the sums of one statistic into a preallocated Array{Float64}(8,8,8,n_blocks,K); returns the number of samples"""
function stats_download!(a::Array{Float64}, d::DeviceLevel, stat::Int32)
    n = Ref{Int64}(0)
    GC.@preserve a check(ccall((:ludwig_level_stats_download, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Csize_t, Ref{Int64}),
                               d.handle, stat, pointer(a), sizeof(a), n))
    return n[]
end

# flow monitor: compute_flow_stats (src/diagnostics.jl:56-94) of the owned cells plus the non-finite count and where each extreme sits
"""the health record of the level's newest state after sub-step `timestep` (vel_temp if even, vel if odd; rho as stored):
(counts = [non-obstacle cells, non-finite cells], cells = 4 x 4 Int64 with one column (bx, by, bz, x + 8y + 64z) each for min rho,
max rho, max v2 and the first non-finite cell (-1 where absent), extremes = Float32[min rho, max rho, max v2],
sums = Float64[sum rho, sum rho v2] in the fixed balanced tree of include/ludwig_hip.h)"""
function monitor(d::DeviceLevel, timestep::Integer)
    counts, cells = zeros(Int64, 2), fill(Int64(-1), 4, 4)
    extremes, sums = zeros(Float32, 3), zeros(Float64, 2)
    GC.@preserve counts cells extremes sums check(ccall((:ludwig_level_monitor, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float32}, Ptr{Float64}),
        d.handle, Int64(timestep), pointer(counts), pointer(cells), pointer(extremes), pointer(sums)))
    return (counts = counts, cells = cells, extremes = extremes, sums = sums)
end

# velocity-gradient fields (no reference counterpart for the output; the gradient is compute_velocity_gradients, the one WALE uses)
const GRAD_VORTICITY, GRAD_Q = Int32(0), Int32(1)                       # K = 3, 1
"""vorticity and Q-criterion of the owned cells from `vel_field` (VEL or VEL_TEMP), derivatives times `scale` (1/dx)"""
gradient_fields_compute!(d::DeviceLevel, vel_field::Integer, scale::Real) =
    check(ccall((:ludwig_level_gradient_fields_compute, LIB), Cint, (Ptr{Cvoid}, Cint, Cfloat), d.handle, Cint(vel_field), Float32(scale)))
"""the last computed field into a preallocated Array{Float32}(8,8,8,n_blocks,K) (K = 3 for GRAD_VORTICITY, 1 for GRAD_Q)"""
gradient_fields_download!(a::Array{Float32}, d::DeviceLevel, which::Int32) =
    GC.@preserve a check(ccall((:ludwig_level_gradient_fields_download, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Csize_t),
                               d.handle, which, pointer(a), sizeof(a)))

# iso-surfaces (no reference counterpart): the triangles of s = value on one level, extracted on the device
const ISO_DENSITY = Int32(0)
const ISO_VELOCITY_MAGNITUDE = Int32(1)
const ISO_Q_CRITERION = Int32(2)
const ISO_VORTICITY_MAGNITUDE = Int32(3)
const ISO_REFUSED = Cint(1)
"""count the triangles of `which` = value on the level and, unless there are more than `max_triangles`, emit them into the level's
buffers: (n_triangles, emitted). vel_field: VEL or VEL_TEMP; scale: the gradient's (1/dx); skip: per block (reference order) non-zero
where no cube is anchored, or `nothing`; cell_lo / cell_hi: the box of anchor cells, 3 Int32 each."""
function isosurface_extract!(d::DeviceLevel, which::Integer, vel_field::Integer, scale::Real, value::Real,
                             skip::Union{Nothing,Vector{UInt8}}, cell_lo::Vector{Int32}, cell_hi::Vector{Int32}, max_triangles::Integer)
    n = Ref{Int64}(0)
    sk = skip === nothing ? UInt8[] : skip
    rc = GC.@preserve sk cell_lo cell_hi ccall((:ludwig_level_isosurface_extract, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cfloat, Cfloat, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Int64, Ref{Int64}),
        d.handle, Cint(which), Cint(vel_field), Float32(scale), Float32(value), skip === nothing ? Ptr{UInt8}(C_NULL) : pointer(sk),
        cell_lo, cell_hi, Int64(max_triangles), n)
    rc == ISO_REFUSED || check(rc)
    return Int(n[]), rc != ISO_REFUSED
end
"""the last extraction into positions (3 x 3 x n Float32), attributes (4 x 3 x n Float32: rho, ux, uy, uz) and keys (2 x 3 x n Int32)"""
isosurface_download!(positions::Array{Float32,3}, attributes::Array{Float32,3}, keys::Array{Int32,3}, d::DeviceLevel) =
    GC.@preserve positions attributes keys check(ccall((:ludwig_level_isosurface_download, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Csize_t, Ptr{Float32}, Csize_t, Ptr{Int32}, Csize_t),
        d.handle, positions, sizeof(positions), attributes, sizeof(attributes), keys, sizeof(keys)))

# probes (no reference counterpart): rho, u at points, trilinear in float32 (x, then y, then z), sampled into a device ring
"""a probe set over `grids`: per probe its 0-based level, 8 stencil corners (reference block index, cell x + 8y + 64z; corners that
are no fluid cell of that level already replaced by the base cell) as 8 x n Int32 matrices, weights 3 x n Float32, ring capacity in
samples. Free it with `probes_destroy`."""
function probes_create(grids::Vector{DeviceLevel}, level::Vector{Int32}, blocks::Matrix{Int32}, cells::Matrix{Int32},
                       weights::Matrix{Float32}, capacity::Integer)
    handles = Ptr{Cvoid}[g.handle for g in grids]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve handles level blocks cells weights check(ccall((:ludwig_probes_create, LIB), Cint,
        (Ptr{Ptr{Cvoid}}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Int32, Ref{Ptr{Cvoid}}),
        handles, Int32(length(grids)), Int32(length(level)), level, blocks, cells, weights, Int32(capacity), out))
    return out[]
end
probes_destroy(p::Ptr{Cvoid}) = ccall((:ludwig_probes_destroy, LIB), Cvoid, (Ptr{Cvoid},), p)
"""sample the probes of 0-based level `level` after its sub-step `timestep` (queued on the level's stream)"""
probes_sample!(p::Ptr{Cvoid}, level::Integer, timestep::Integer) =
    check(ccall((:ludwig_probes_sample, LIB), Cint, (Ptr{Cvoid}, Int32, Int64), p, Int32(level), Int64(timestep)))
"""the samples since the last download into values (4 x n_probes x max) and steps (max); returns how many, oldest first"""
function probes_download!(values::Array{Float32,3}, steps::Vector{Int64}, p::Ptr{Cvoid})
    n = Ref{Int32}(0)
    GC.@preserve values steps check(ccall((:ludwig_probes_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int64}, Int32, Ref{Int32}),
                                          p, values, steps, Int32(length(steps)), n))
    return Int(n[])
end

# slices (no reference counterpart): planar grids of points, the probes' stencil and trilinear, plus |u|, vorticity and Q
const SLICE_GRADIENT = Int32(1)
"""a slice set over `grids`: per point its 0-based level, 8 stencil corners as probes_create takes them, weights 3 x n Float32, valid
(UInt8, 0: not read, sampled as 0), per level the gradient scale (1/dx), flags (SLICE_GRADIENT adds vorticity and Q). Free it with
`slices_destroy`."""
function slices_create(grids::Vector{DeviceLevel}, level::Vector{Int32}, blocks::Matrix{Int32}, cells::Matrix{Int32},
                       weights::Matrix{Float32}, valid::Vector{UInt8}, scales::Vector{Float32}, flags::Integer)
    handles = Ptr{Cvoid}[g.handle for g in grids]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve handles level blocks cells weights valid scales check(ccall((:ludwig_slices_create, LIB), Cint,
        (Ptr{Ptr{Cvoid}}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{UInt8}, Ptr{Float32}, Int32, Ref{Ptr{Cvoid}}),
        handles, Int32(length(grids)), Int32(length(level)), level, blocks, cells, weights, valid, scales, Int32(flags), out))
    return out[]
end
slices_destroy(s::Ptr{Cvoid}) = ccall((:ludwig_slices_destroy, LIB), Cvoid, (Ptr{Cvoid},), s)
"""sample every point on its level's newest state after coarse step `t_coarse` (queued on the levels' streams)"""
slices_sample!(s::Ptr{Cvoid}, t_coarse::Integer) = check(ccall((:ludwig_slices_sample, LIB), Cint, (Ptr{Cvoid}, Int64), s, Int64(t_coarse)))
"""the last sample into values (n_points x rows: 5, or 9 with SLICE_GRADIENT)"""
slices_download!(values::Matrix{Float32}, s::Ptr{Cvoid}) =
    GC.@preserve values check(ccall((:ludwig_slices_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), s, values, sizeof(values)))

# streamlines (no reference counterpart): lines traced through ALL levels on the device; the kernel locates every point itself
const STREAM_END_STEPS = Int32(0)
const STREAM_END_OUTSIDE = Int32(1)
const STREAM_END_OBSTACLE = Int32(2)
const STREAM_END_SLOW = Int32(3)
"""a streamline set over every level of `grids` (each created with block_pointer, without ghost blocks): seeds 3 x n Float32 in cell
units of the first level (domain frame), sign n Float32 (1 or -1), step in cells of the level a step starts on, min_speed, max_steps.
Free it with `streamlines_destroy`."""
function streamlines_create(grids::Vector{DeviceLevel}, seeds::Matrix{Float32}, sign::Vector{Float32}, step::Real, min_speed::Real,
                            max_steps::Integer)
    handles = Ptr{Cvoid}[g.handle for g in grids]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve handles seeds sign check(ccall((:ludwig_streamlines_create, LIB), Cint,
        (Ptr{Ptr{Cvoid}}, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Int32, Ref{Ptr{Cvoid}}),
        handles, Int32(length(grids)), Int32(length(sign)), seeds, sign, Float32(step), Float32(min_speed), Int32(max_steps), out))
    return out[]
end
streamlines_destroy(s::Ptr{Cvoid}) = ccall((:ludwig_streamlines_destroy, LIB), Cvoid, (Ptr{Cvoid},), s)
"""trace every line through the newest state of all levels after coarse step `t_coarse` (one launch, queued)"""
streamlines_trace!(s::Ptr{Cvoid}, t_coarse::Integer) =
    check(ccall((:ludwig_streamlines_trace, LIB), Cint, (Ptr{Cvoid}, Int64), s, Int64(t_coarse)))
"""the last trace into counts and codes (n Int32) and vertices (8 x (max_steps + 1) x n Float32: x, y, z, rho, ux, uy, uz, level
index; only the first maximum(counts) records of each line are written)"""
streamlines_download!(counts::Vector{Int32}, codes::Vector{Int32}, vertices::Array{Float32,3}, s::Ptr{Cvoid}) =
    GC.@preserve counts codes vertices check(ccall((:ludwig_streamlines_download, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Csize_t), s, counts, codes, vertices, sizeof(vertices)))

# volume images (no reference counterpart): rays marched through ALL levels on the device and composited, one lane per ray
const RENDER_EXIT = Int32(0)
const RENDER_MISS = Int32(1)
const RENDER_BODY = Int32(2)
const RENDER_OPAQUE = Int32(3)
const RENDER_SAMPLES = Int32(4)
"""a render set over every level of `grids` (each created with block_pointer, without ghost blocks) with room for `max_pixels` pixels.
Free it with `render_destroy`."""
function render_create(grids::Vector{DeviceLevel}, max_pixels::Integer)
    handles = Ptr{Cvoid}[g.handle for g in grids]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve handles check(ccall((:ludwig_render_create, LIB), Cint, (Ptr{Ptr{Cvoid}}, Int32, Int64, Ref{Ptr{Cvoid}}),
        handles, Int32(length(grids)), Int64(max_pixels), out))
    return out[]
end
render_destroy(s::Ptr{Cvoid}) = ccall((:ludwig_render_destroy, LIB), Cvoid, (Ptr{Cvoid},), s)
"""queue one image of scalar `which` (0 density, 1 |u|, 2 Q, 3 |omega|) of the newest state after coarse step `t_coarse`: scales one
Float32 per level, camera 16 Float32 (eye, corner, du, dv, dir, 0), params 10 Float32 (step, lo, hi, t_min, background, body colour),
table 4 x 256 Float32 (r, g, b, kappa)"""
render_image!(s::Ptr{Cvoid}, t_coarse::Integer, which::Integer, scales::Vector{Float32}, camera::Vector{Float32}, perspective::Bool,
              width::Integer, height::Integer, params::Vector{Float32}, max_samples::Integer, table::Matrix{Float32}) =
    GC.@preserve scales camera params table check(ccall((:ludwig_render_image, LIB), Cint,
        (Ptr{Cvoid}, Int64, Cint, Ptr{Float32}, Ptr{Float32}, Cint, Int32, Int32, Ptr{Float32}, Int32, Ptr{Float32}),
        s, Int64(t_coarse), Cint(which), scales, camera, Cint(perspective), Int32(width), Int32(height), params, Int32(max_samples), table))
"""the last image into rgba (4 x width x height Float32), codes and samples (width x height Int32)"""
render_download!(rgba::Array{Float32,3}, codes::Matrix{Int32}, samples::Matrix{Int32}, s::Ptr{Cvoid}) =
    GC.@preserve rgba codes samples check(ccall((:ludwig_render_download, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int32}, Ptr{Int32}, Csize_t), s, rgba, codes, samples, sizeof(rgba)))

# tracers (no reference counterpart): particles advected through ALL levels on the device, inside a batch
const TRACER_EMPTY = Int32(-1)
const TRACER_ALIVE = Int32(0)
const TRACER_OUTSIDE = Int32(1)
const TRACER_OBSTACLE = Int32(2)
const TRACER_NONFINITE = Int32(3)
"""a tracer set over every level of `grids` (the streamline sets' conditions): seeds 3 x n Float32 in cell units of the first level,
`generations` slots per seed, one release every `release_every` advances, dt = coarse steps per advance. Free it with
`tracers_destroy`."""
function tracers_create(grids::Vector{DeviceLevel}, seeds::Matrix{Float32}, generations::Integer, release_every::Integer, dt::Real)
    handles = Ptr{Cvoid}[g.handle for g in grids]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve handles seeds check(ccall((:ludwig_tracers_create, LIB), Cint,
        (Ptr{Ptr{Cvoid}}, Int32, Int32, Ptr{Float32}, Int32, Int32, Cfloat, Ref{Ptr{Cvoid}}),
        handles, Int32(length(grids)), Int32(size(seeds, 2)), seeds, Int32(generations), Int32(release_every), Float32(dt), out))
    return out[]
end
tracers_destroy(s::Ptr{Cvoid}) = ccall((:ludwig_tracers_destroy, LIB), Cvoid, (Ptr{Cvoid},), s)
"""one advance behind coarse step `t_coarse`, outside a batch (one launch, queued)"""
tracers_advance!(s::Ptr{Cvoid}, t_coarse::Integer) = check(ccall((:ludwig_tracers_advance, LIB), Cint, (Ptr{Cvoid}, Int64), s, Int64(t_coarse)))
"""snapshot every slot on the newest velocity after coarse step `t_coarse` (one launch, queued; changes no state)"""
tracers_snapshot!(s::Ptr{Cvoid}, t_coarse::Integer) = check(ccall((:ludwig_tracers_snapshot, LIB), Cint, (Ptr{Cvoid}, Int64), s, Int64(t_coarse)))
"""the last snapshot into records (8 x n_slots Float32: x, y, z, ux, uy, uz, level index, code); returns the advances so far"""
function tracers_download!(records::Matrix{Float32}, s::Ptr{Cvoid})
    n = Ref{Int64}(0)
    GC.@preserve records check(ccall((:ludwig_tracers_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t, Ref{Int64}),
                                     s, records, sizeof(records), n))
    return Int(n[])
end

# warm start (no reference counterpart): a level filled from another hierarchy's rho and u, the populations at their equilibrium
"""a flow source from host arrays, one entry per level (first level first): block_pointer (Array{Int32,3}, 1-based, 0 = absent), obstacle
(8 x 8 x 8 x nb UInt8), rho (8 x 8 x 8 x nb Float32), vel (8 x 8 x 8 x nb x 3 Float32). Free it with `flow_source_destroy`."""
function flow_source_create(device::Integer, block_pointer::Vector{Array{Int32,3}}, obstacle::Vector{Array{UInt8,4}},
                            rho::Vector{Array{Float32,4}}, vel::Vector{Array{Float32,5}})
    n = length(block_pointer)
    dims = Int32[size(block_pointer[li], a) for a in 1:3, li in 1:n]
    nb = Int32[size(rho[li], 4) for li in 1:n]
    pb = Ptr{Int32}[pointer(a) for a in block_pointer]
    po = Ptr{UInt8}[pointer(a) for a in obstacle]
    pr = Ptr{Float32}[pointer(a) for a in rho]
    pv = Ptr{Float32}[pointer(a) for a in vel]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve block_pointer obstacle rho vel dims nb pb po pr pv check(ccall((:ludwig_flow_source_create, LIB), Cint,
        (Cint, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Ptr{Int32}}, Ptr{Ptr{UInt8}}, Ptr{Ptr{Float32}}, Ptr{Ptr{Float32}}, Ref{Ptr{Cvoid}}),
        Cint(device), Int32(n), dims, nb, pb, po, pr, pv, out))
    return out[]
end
"""a flow source copied on the device from the newest state of `grids` after coarse step `t_coarse` (the streamline sets' conditions)"""
function flow_source_from_levels(grids::Vector{DeviceLevel}, t_coarse::Integer)
    handles = Ptr{Cvoid}[g.handle for g in grids]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve handles check(ccall((:ludwig_flow_source_from_levels, LIB), Cint, (Ptr{Ptr{Cvoid}}, Int32, Int64, Ref{Ptr{Cvoid}}),
        handles, Int32(length(grids)), Int64(t_coarse), out))
    return out[]
end
flow_source_destroy(s::Ptr{Cvoid}) = ccall((:ludwig_flow_source_destroy, LIB), Cvoid, (Ptr{Cvoid},), s)
"""fill `grid` from the source: map = (a_x, a_y, a_z, b_x, b_y, b_z), P = a (cell centre) + b in cells of the source's first level;
rho' = 1 + (rho - 1) vel_scale^2, u' = u vel_scale, fallback (rho, ux, uy, uz) where the source has no finite value; f = f_temp =
equilibrium. Returns the counts: found, outside, source obstacle, non-finite, then found per source level (`n_src_levels` of them)."""
function init_from_source!(grid::DeviceLevel, src::Ptr{Cvoid}, map::Vector{Float32}, vel_scale::Real, fallback::Vector{Float32},
                           n_src_levels::Integer)
    counts = zeros(Int64, 4 + n_src_levels)
    GC.@preserve map fallback counts check(ccall((:ludwig_level_init_from_source, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Cfloat, Ptr{Float32}, Ptr{Int64}), grid.handle, src, map, Float32(vel_scale), fallback, counts))
    return counts
end

# surface statistics (no reference counterpart): 7 float64 sums per triangle of p, p^2, tau, |tau|, |tau|^2 at its nearest fluid cell
"""a surface set on `grid`: per triangle its nearest fluid cell (0-based reference block index, -1 = none; cell x + 8y + 64z), wall
distance in lattice units and normal (3 x n); tau and the two scales from `sp`. Free it with `surface_stats_destroy`."""
function surface_stats_create(grid::DeviceLevel, blocks::Vector{Int32}, cells::Vector{Int32}, wall_dist::Vector{Float32},
                              normals::Matrix{Float32}, sp::SurfaceParams)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve blocks cells wall_dist normals check(ccall((:ludwig_surface_stats_create, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Ref{SurfaceParams}, Ref{Ptr{Cvoid}}),
        grid.handle, Int32(length(blocks)), blocks, cells, wall_dist, normals, sp, out))
    return out[]
end
surface_stats_destroy(s::Ptr{Cvoid}) = ccall((:ludwig_surface_stats_destroy, LIB), Cvoid, (Ptr{Cvoid},), s)
surface_stats_reset!(s::Ptr{Cvoid}) = check(ccall((:ludwig_surface_stats_reset, LIB), Cint, (Ptr{Cvoid},), s))
"""one sample of the state the level's sub-step `timestep` wrote (queued on the level's stream)"""
surface_stats_accumulate!(s::Ptr{Cvoid}, timestep::Integer) =
    check(ccall((:ludwig_surface_stats_accumulate, LIB), Cint, (Ptr{Cvoid}, Int64), s, Int64(timestep)))
"""the sums into `sums` (n_tri x 7: S_p, S_pp, S_tau_x, S_tau_y, S_tau_z, S_|tau|, S_|tau|^2); returns the number of samples"""
function surface_stats_download!(sums::Matrix{Float64}, s::Ptr{Cvoid})
    n = Ref{Int64}(0)
    GC.@preserve sums check(ccall((:ludwig_surface_stats_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Csize_t, Ref{Int64}),
                                  s, sums, sizeof(sums), n))
    return Int(n[])
end

# force series (no reference counterpart): the nine integrated load sums Fp(3), Fv(3), M(3) and the coverage count per sampled coarse step
"""a force-series set on `grid`: per triangle its nearest fluid cell (0-based reference block index, -1 = none; cell x + 8y + 64z), wall
distance in lattice units, normal (3 x n), area and moment arm (n x 3: centre + offset - moment centre in Float32); tau and the two
scales from `sp`; a ring of `capacity` records. Free it with `force_series_destroy`."""
function force_series_create(grid::DeviceLevel, blocks::Vector{Int32}, cells::Vector{Int32}, wall_dist::Vector{Float32},
                             normals::Matrix{Float32}, area::Vector{Float32}, arm::Matrix{Float32}, sp::SurfaceParams, capacity::Integer)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve blocks cells wall_dist normals area arm check(ccall((:ludwig_force_series_create, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ref{SurfaceParams}, Int32,
         Ref{Ptr{Cvoid}}),
        grid.handle, Int32(length(blocks)), blocks, cells, wall_dist, normals, area, arm, sp, Int32(capacity), out))
    return out[]
end
force_series_destroy(s::Ptr{Cvoid}) = ccall((:ludwig_force_series_destroy, LIB), Cvoid, (Ptr{Cvoid},), s)
"""one record of the state the level's sub-step `timestep` wrote, filed under coarse step `t_coarse` (queued on the level's stream)"""
force_series_sample!(s::Ptr{Cvoid}, timestep::Integer, t_coarse::Integer) =
    check(ccall((:ludwig_force_series_sample, LIB), Cint, (Ptr{Cvoid}, Int64, Int64), s, Int64(timestep), Int64(t_coarse)))
"""the records taken since the last download into sums (9 x capacity), covered and steps (capacity); returns how many; empties the ring"""
function force_series_download!(sums::Matrix{Float64}, covered::Vector{Int64}, steps::Vector{Int64}, s::Ptr{Cvoid})
    n = Ref{Int32}(0)
    GC.@preserve sums covered steps check(ccall((:ludwig_force_series_download, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int32, Ref{Int32}), s, sums, covered, steps, Int32(length(steps)), n))
    return Int(n[])
end

# flux planes (no reference counterpart): per plane and sampled coarse step the eight sums of rho, un, m, m ux, m uy, m uz, rho q, m q
# (m = rho un, q = |u|^2) over its valid points and their count; pass the set to a batch as entry(OBSERVE_FLUXES, set, start_step, interval)
"""a flux-plane set over `grids`: plane k has the normal axis `normal[k]` (0, 1, 2) and the points `plane_start[k]` .. `plane_start[k+1]`-1
(0-based, `plane_start[1]` = 0); per point its 0-based level, the probes' stencil (8 x n blocks and cells, 3 x n weights) and `valid`;
a ring of `capacity` samples. Free it with `flux_planes_destroy`."""
function flux_planes_create(grids::Vector{DeviceLevel}, plane_start::Vector{Int32}, normal::Vector{Int32}, level::Vector{Int32},
                            blocks::Matrix{Int32}, cells::Matrix{Int32}, weights::Matrix{Float32}, valid::Vector{UInt8}, capacity::Integer)
    handles = Ptr{Cvoid}[g.handle for g in grids]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve handles plane_start normal level blocks cells weights valid check(ccall((:ludwig_flux_planes_create, LIB), Cint,
        (Ptr{Ptr{Cvoid}}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{UInt8}, Int32,
         Ref{Ptr{Cvoid}}),
        handles, Int32(length(grids)), Int32(length(normal)), plane_start, normal, level, blocks, cells, weights, valid, Int32(capacity), out))
    return out[]
end
flux_planes_destroy(s::Ptr{Cvoid}) = ccall((:ludwig_flux_planes_destroy, LIB), Cvoid, (Ptr{Cvoid},), s)
"""between batches: one sample of the state after coarse step `t_coarse` (every level that holds points, queued on its stream)"""
flux_planes_sample!(s::Ptr{Cvoid}, t_coarse::Integer) =
    check(ccall((:ludwig_flux_planes_sample, LIB), Cint, (Ptr{Cvoid}, Int64), s, Int64(t_coarse)))
"""the samples taken since the last download into sums (8 x n_planes x capacity), counts (n_planes x capacity) and steps (capacity);
returns how many; empties the ring"""
function flux_planes_download!(sums::Array{Float64,3}, counts::Matrix{Int64}, steps::Vector{Int64}, s::Ptr{Cvoid})
    n = Ref{Int32}(0)
    GC.@preserve sums counts steps check(ccall((:ludwig_flux_planes_download, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int32, Ref{Int32}), s, sums, counts, steps, Int32(length(steps)), n))
    return Int(n[])
end

# Fourier modes (no reference counterpart): per cell and table column the running sums of rho, ux, uy, uz times one row of a weight table
# per sample; pass the set to a batch as entry(OBSERVE_MODES, set, start_step, interval) - the row of an observed step t is then
# ((t - start_step) / interval) % n_rows, and a batch must not run past the end of a window
"""a mode set over `grids` with the weight table `W` (n_columns x n_rows: one table row per Julia column, as the C table is row-major;
1 <= n_columns <= 33, 1 <= n_rows <= 65536). Free it with `modes_destroy`."""
function modes_create(grids::Vector{DeviceLevel}, W::Matrix{Float64})
    handles = Ptr{Cvoid}[g.handle for g in grids]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve handles W check(ccall((:ludwig_modes_create, LIB), Cint,
        (Ptr{Ptr{Cvoid}}, Int32, Int32, Int32, Ptr{Float64}, Ref{Ptr{Cvoid}}),
        handles, Int32(length(grids)), Int32(size(W, 1)), Int32(size(W, 2)), W, out))
    return out[]
end
modes_destroy(s::Ptr{Cvoid}) = ccall((:ludwig_modes_destroy, LIB), Cvoid, (Ptr{Cvoid},), s)
"""zero the sums and every level's sample count (queued on the levels' streams)"""
modes_reset!(s::Ptr{Cvoid}) = check(ccall((:ludwig_modes_reset, LIB), Cint, (Ptr{Cvoid},), s))
"""between batches: one sample of level `level_index` (0-based) after its sub-step `t_sub` with table row `row` (0-based, in order)"""
modes_accumulate!(s::Ptr{Cvoid}, level_index::Integer, t_sub::Integer, row::Integer) =
    check(ccall((:ludwig_modes_accumulate, LIB), Cint, (Ptr{Cvoid}, Int32, Int64, Int32), s, Int32(level_index), Int64(t_sub), Int32(row)))
"""the sums of one column (0-based) of a level into `sums` (8 x 8 x 8 x n_blocks x 4: rho, ux, uy, uz); returns the level's samples"""
function modes_download!(sums::Array{Float64,5}, s::Ptr{Cvoid}, level_index::Integer, column::Integer)
    n = Ref{Int32}(0)
    GC.@preserve sums check(ccall((:ludwig_modes_download, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Csize_t, Ref{Int32}),
                                  s, Int32(level_index), Int32(column), sums, Csize_t(sizeof(sums)), n))
    return Int(n[])
end

# wall diagnostics (no reference counterpart: Y_PLUS_TARGET is read and never used): the wall model's y+, u_tau and modelled shear
"""LudwigWallCensus of include/ludwig_hip.h: counts, the Float32 bits of the least / greatest y+, 194 bins (eight per octave)"""
struct WallCensus
    near_cells::UInt64
    evaluated::UInt64
    log_law::UInt64
    forced::UInt64
    non_finite::UInt64
    min_bits::UInt32
    max_bits::UInt32
    hist::NTuple{194,UInt64}
end
"""the census of the level's owned blocks from the state sub-step `timestep` wrote (vel_temp if even, vel if odd; rho as stored)"""
function wall_census(d::DeviceLevel, timestep::Integer)
    out = Ref{WallCensus}()
    check(ccall((:ludwig_level_wall_census, LIB), Cint, (Ptr{Cvoid}, Int64, Ref{WallCensus}), d.handle, Int64(timestep), out))
    return out[]
end
"""a wall-surface set on `grid`: per triangle its nearest fluid cell (0-based reference block index, -1 = none; cell x + 8y + 64z)
and normal (3 x n); the two scales from `sp`. Free it with `wall_surface_destroy`."""
function wall_surface_create(grid::DeviceLevel, blocks::Vector{Int32}, cells::Vector{Int32}, normals::Matrix{Float32}, sp::SurfaceParams)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve blocks cells normals check(ccall((:ludwig_wall_surface_create, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ref{SurfaceParams}, Ref{Ptr{Cvoid}}),
        grid.handle, Int32(length(blocks)), blocks, cells, normals, sp, out))
    return out[]
end
wall_surface_destroy(s::Ptr{Cvoid}) = ccall((:ludwig_wall_surface_destroy, LIB), Cvoid, (Ptr{Cvoid},), s)
"""evaluate the state the level's sub-step `timestep` wrote (queued on the level's stream)"""
wall_surface_compute!(s::Ptr{Cvoid}, timestep::Integer) =
    check(ccall((:ludwig_wall_surface_compute, LIB), Cint, (Ptr{Cvoid}, Int64), s, Int64(timestep)))
"""the last values into `values` (n_tri x 7: p, tau_model_x, y, z, u_tau, y_plus, code)"""
wall_surface_download!(values::Matrix{Float32}, s::Ptr{Cvoid}) =
    GC.@preserve values check(ccall((:ludwig_wall_surface_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), s, values, sizeof(values)))

# subgrid model: the WALE eddy viscosity the step collides with, its branch code, and the time-averaged sums (no reference counterpart
# for the output; the model is perform_timestep_v2!'s). c_wale and nu_sgs_background are those of the level's last step.
const SUBGRID_NU, SUBGRID_CODE = Int32(0), Int32(1)
const SUBGRID_SUM_NU, SUBGRID_SUM_NUNU, SUBGRID_SUM_EPS = Int32(0), Int32(1), Int32(2)
"""nu_t (after the background floor) and the branch code of the owned cells from `vel_field` (VEL or VEL_TEMP)"""
subgrid_fields_compute!(d::DeviceLevel, vel_field::Integer) =
    check(ccall((:ludwig_level_subgrid_fields_compute, LIB), Cint, (Ptr{Cvoid}, Cint), d.handle, Cint(vel_field)))
"""the last computed field (SUBGRID_NU or SUBGRID_CODE) into a preallocated Array{Float32}(8,8,8,n_blocks)"""
subgrid_fields_download!(a::Array{Float32}, d::DeviceLevel, which::Int32) =
    GC.@preserve a check(ccall((:ludwig_level_subgrid_fields_download, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Csize_t),
                               d.handle, which, pointer(a), sizeof(a)))
subgrid_stats_reset!(d::DeviceLevel) = check(ccall((:ludwig_level_subgrid_stats_reset, LIB), Cint, (Ptr{Cvoid},), d.handle))
"""add one sample from the velocity buffer sub-step `timestep` wrote"""
subgrid_stats_accumulate!(d::DeviceLevel, timestep::Integer) =
    check(ccall((:ludwig_level_subgrid_stats_accumulate, LIB), Cint, (Ptr{Cvoid}, Int64), d.handle, Int64(timestep)))
"""one sum (SUBGRID_SUM_NU, _NUNU, _EPS) into a preallocated Array{Float64}(8,8,8,n_blocks); returns the number of samples"""
function subgrid_stats_download!(a::Array{Float64}, d::DeviceLevel, which::Int32)
    n = Ref{Int64}(0)
    GC.@preserve a check(ccall((:ludwig_level_subgrid_stats_download, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Csize_t, Ref{Int64}),
                               d.handle, which, pointer(a), sizeof(a), n))
    return n[]
end

"""
Multi-GPU hosts only: a HIP stream for the stepping kernels that leaves `reserved_cus` compute units to the halo exchange
(`ludwig_stream_create`, include/ludwig_hip.h); hand it to `ludwig_level_set_stream`. No counterpart in the reference.
"""
function stream_create(device::Integer, reserved_cus::Integer)
    s = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:ludwig_stream_create, LIB), Cint, (Cint, Cint, Ref{Ptr{Cvoid}}), Cint(device), Cint(reserved_cus), s))
    return s[]
end
stream_destroy(device::Integer, s::Ptr{Cvoid}) = check(ccall((:ludwig_stream_destroy, LIB), Cint, (Cint, Ptr{Cvoid}), Cint(device), s))

# ---- multi-GPU (no counterpart in the reference: single device, src/main.jl:75). One Julia process per GPU; the host carries the
# 128-byte RCCL id from rank 0 to the others by whatever it already has (MPI.jl: MPI.Bcast!, a shared file, Sockets). ----
struct Comm
    handle::Ptr{Cvoid}
end
"""ncclGetUniqueId through the library: call on ONE rank, broadcast the 128 bytes."""
function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    GC.@preserve id check(ccall((:ludwig_comm_unique_id, LIB), Cint, (Ptr{Cvoid},), pointer(id)))
    return id
end
function Comm(id::Vector{UInt8}, rank::Integer, world::Integer, device::Integer)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve id check(ccall((:ludwig_comm_create, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Ref{Ptr{Cvoid}}), pointer(id), Cint(rank), Cint(world), Cint(device), out))
    return Comm(out[])
end
destroy!(c::Comm) = ccall((:ludwig_comm_destroy, LIB), Cvoid, (Ptr{Cvoid},), c.handle)
"""small levels: queue the exchange on the level's own stream (no overlap, no cross-stream hand-over; `wait!` becomes a no-op)"""
in_stream!(p, on::Bool) = check(ccall((:ludwig_halo_plan_in_stream, LIB), Cint, (Ptr{Cvoid}, Cint), p.handle, Cint(on)))
"""
Bouzidi level cut over ranks: the f_post_collision elements a PEER's links read across the cut (= this rank's group-2 send list,
0-based element offsets in the [8,8,8,n_blocks,27] layout). The step then stores the rows with a reader instead of every block.
"""
function add_post_collision_readers!(d::DeviceLevel, offsets::Vector{Int64})
    GC.@preserve offsets check(ccall((:ludwig_level_add_post_collision_readers, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64),
                                     d.handle, isempty(offsets) ? Ptr{Int64}(C_NULL) : pointer(offsets), Int64(length(offsets))))
end
"""in-place all-reduce of a few Float32 diagnostics (op 0 sum, 2 max, 3 min): rho_min, the nine force sums"""
allreduce!(c::Comm, v::Vector{Float32}, op::Integer) =
    GC.@preserve v check(ccall((:ludwig_comm_allreduce_f32, LIB), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Int32, Int32), c.handle, pointer(v), Int32(length(v)), Int32(op)))

"""LudwigHaloPlanDesc (include/ludwig_hip.h): per group g = 1..4 (populations, velocity, f_post_collision, rho) the element offsets
this rank sends / receives, all peers concatenated; offsets are 0-based positions in the level's arrays as the reference lays them out."""
struct HaloPlanDesc
    n_peers::Int32
    peer_ranks::Ptr{Int32}
    send_count::NTuple{4,Ptr{Int64}}
    recv_count::NTuple{4,Ptr{Int64}}
    send_index::NTuple{4,Ptr{Int64}}
    recv_index::NTuple{4,Ptr{Int64}}
end
struct HaloPlan
    handle::Ptr{Cvoid}
end
function HaloPlan(d::DeviceLevel, c::Union{Comm,Nothing}, peers::Vector{Int32}, send_count::NTuple{4,Vector{Int64}}, recv_count::NTuple{4,Vector{Int64}},
                  send_index::NTuple{4,Vector{Int64}}, recv_index::NTuple{4,Vector{Int64}})
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve peers send_count recv_count send_index recv_index begin
        desc = HaloPlanDesc(Int32(length(peers)), pointer(peers), map(pointer, send_count), map(pointer, recv_count), map(pointer, send_index), map(pointer, recv_index))
        check(ccall((:ludwig_halo_plan_create, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{HaloPlanDesc}, Ref{Ptr{Cvoid}}),
                    d.handle, c === nothing ? C_NULL : c.handle, desc, out))
    end
    return HaloPlan(out[])
end
destroy!(p::HaloPlan) = ccall((:ludwig_halo_plan_destroy, LIB), Cvoid, (Ptr{Cvoid},), p.handle)
"""one exchange, queued behind what the level's stream holds: group groups[i] (0-based) moves field fields[i]"""
exchange!(p::HaloPlan, groups::Vector{Int32}, fields::Vector{Int32}) =
    GC.@preserve groups fields check(ccall((:ludwig_halo_exchange, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}), p.handle, Int32(length(groups)), pointer(groups), pointer(fields)))
wait!(p::HaloPlan) = check(ccall((:ludwig_halo_wait, LIB), Cint, (Ptr{Cvoid},), p.handle))

"""
perform_timestep_v2! of a level spread over ranks: interior blocks, wait for the previous exchange, boundary blocks, [f_post halo,
Bouzidi], this step's exchange left in flight (ludwig_step_distributed). Drop-in for `perform_timestep!` in `recursive_step!` below
when the level has a plan.
"""
function perform_timestep_distributed!(d::DeviceLevel, plan::HaloPlan, parent::Union{DeviceLevel,Nothing}, parent_tau::Float32, u_curr::Float32,
                                       flags::StepFlags, timestep::Integer, temporal_weight::Float32)
    p = parent === nothing ? C_NULL : parent.handle
    check(ccall((:ludwig_step_distributed, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cfloat, Cfloat, Cfloat, Ref{StepFlags}),
                d.handle, plan.handle, p, Int64(timestep), u_curr, parent_tau, temporal_weight, flags))
end

"""
recursive_step! with the device calls swapped (src/solver_control.jl:21-143): same order, same parity, same weights.
"""
function recursive_step!(grids::Vector{DeviceLevel}, lvl::Int, t_sub::Int, parent, parent_tau::Float32, tw::Float32,
                         u_vel::Float32, flags::StepFlags)
    lvl > length(grids) && return
    level = grids[lvl]
    has_children = lvl < length(grids)
    if has_children && flags.use_temporal_interp == 1 && level.has_temporal
        copy_to_old!(level, t_sub)
    end
    perform_timestep!(level, parent, parent_tau, u_vel, flags, t_sub, tw)
    if has_children
        recursive_step!(grids, lvl + 1, 2 * t_sub, level, level.tau, 0.0f0, u_vel, flags)
        recursive_step!(grids, lvl + 1, 2 * t_sub + 1, level, level.tau, 0.5f0, u_vel, flags)
    end
end

"""execute_timestep_batch! (src/solver_control.jl:145-165): the whole batch in one ccall (the library runs the same
recursion); `recursive_step!` above is the call-by-call equivalent."""
function execute_timestep_batch!(grids::Vector{DeviceLevel}, t_start::Int, batch_size::Int, u_curr::Float32, flags::StepFlags)
    handles = Ptr{Cvoid}[g.handle for g in grids]
    GC.@preserve handles check(ccall((:ludwig_execute_timestep_batch, LIB), Cint,
                                     (Ptr{Ptr{Cvoid}}, Int32, Int64, Int32, Cfloat, Ref{StepFlags}),
                                     handles, Int32(length(grids)), Int64(t_start), Int32(batch_size), u_curr, flags))
end

"""execute_timestep_batch! with the sets of `observers` observed inside the batch, each at the coarse steps start_step + k interval of
its own entry; an entry whose set is C_NULL is ignored, an empty vector is the call above"""
function execute_timestep_batch!(grids::Vector{DeviceLevel}, t_start::Int, batch_size::Int, u_curr::Float32, flags::StepFlags,
                                 observers::Vector{BatchObserver})
    handles = Ptr{Cvoid}[g.handle for g in grids]
    GC.@preserve handles observers check(ccall((:ludwig_execute_timestep_batch_observed, LIB), Cint,
                                               (Ptr{Ptr{Cvoid}}, Int32, Int64, Int32, Cfloat, Ref{StepFlags}, Ptr{BatchObserver}, Int32),
                                               handles, Int32(length(grids)), Int64(t_start), Int32(batch_size), u_curr, flags, observers,
                                               Int32(length(observers))))
end

# The methods from before the observer list keep their signatures: each builds its entries (a set may be C_NULL) and calls the one above.
entry(kind::Int32, set::Ptr{Cvoid}, start_step::Integer, interval::Integer) = BatchObserver(kind, set, Int64(start_step), Int32(interval))
entries(s::BatchSamplers) = [entry(OBSERVE_PROBES, s.probes, s.probes_start_step, s.probes_interval),
                             entry(OBSERVE_SURFACE, s.surface, s.surface_start_step, s.surface_interval)]
entries(::Nothing) = BatchObserver[]

"""the probes of `probes` sampled inside the batch: one OBSERVE_PROBES entry"""
execute_timestep_batch!(grids::Vector{DeviceLevel}, t_start::Int, batch_size::Int, u_curr::Float32, flags::StepFlags,
                        probes::Ptr{Cvoid}, start_step::Integer, interval::Integer) =
    execute_timestep_batch!(grids, t_start, batch_size, u_curr, flags, [entry(OBSERVE_PROBES, probes, start_step, interval)])

"""the probe set and the surface set of `s`: an OBSERVE_PROBES and an OBSERVE_SURFACE entry"""
execute_timestep_batch!(grids::Vector{DeviceLevel}, t_start::Int, batch_size::Int, u_curr::Float32, flags::StepFlags, s::BatchSamplers) =
    execute_timestep_batch!(grids, t_start, batch_size, u_curr, flags, entries(s))

"""the entries of `s` (`nothing`: none) and an OBSERVE_FORCES entry for the force series `forces`"""
execute_timestep_batch!(grids::Vector{DeviceLevel}, t_start::Int, batch_size::Int, u_curr::Float32, flags::StepFlags,
                        s::Union{BatchSamplers,Nothing}, forces::Ptr{Cvoid}, start_step::Integer, interval::Integer) =
    execute_timestep_batch!(grids, t_start, batch_size, u_curr, flags, [entries(s); entry(OBSERVE_FORCES, forces, start_step, interval)])

"""the entries of `s` (`nothing`: none), an OBSERVE_FORCES entry and an OBSERVE_TRACERS entry for the tracer set `tracers`"""
execute_timestep_batch!(grids::Vector{DeviceLevel}, t_start::Int, batch_size::Int, u_curr::Float32, flags::StepFlags,
                        s::Union{BatchSamplers,Nothing}, forces::Ptr{Cvoid}, force_start_step::Integer, force_interval::Integer,
                        tracers::Ptr{Cvoid}, start_step::Integer, interval::Integer) =
    execute_timestep_batch!(grids, t_start, batch_size, u_curr, flags,
                            [entries(s); entry(OBSERVE_FORCES, forces, force_start_step, force_interval);
                             entry(OBSERVE_TRACERS, tracers, start_step, interval)])

"""the Fourier modes of `modes` accumulated inside the batch: one OBSERVE_MODES entry"""
execute_timestep_batch_modes!(grids::Vector{DeviceLevel}, t_start::Int, batch_size::Int, u_curr::Float32, flags::StepFlags,
                              modes::Ptr{Cvoid}, start_step::Integer, interval::Integer) =
    execute_timestep_batch!(grids, t_start, batch_size, u_curr, flags, [entry(OBSERVE_MODES, modes, start_step, interval)])

end # module
