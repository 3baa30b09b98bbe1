# ccall wrappers of include/celeste_blend.h (libceleste_blend.so): maximize! with several active sources on the MI355X.
# Kept apart from CelesteMI355X.jl, whose surface is fixed.  Not executed in this repository's tests (no Julia here):
# tests/test_blend_host.py holds every ccall to the header's prototypes.
module CelesteMI355XBlend

const LIB = get(ENV, "CELESTE_MI355X_BLEND_LIB", joinpath(@__DIR__, "..", "celeste.jl_amd", "csrc", "blend", "libceleste_blend.so"))
const SA_MAX = 4              # CELESTE_BLEND_SA_MAX

struct OptimConfig            # celeste_optim_config_t (include/celeste_mi355x.h)
    loc_width::Float64
    loc_scale::Float64
    max_iters::Int32
    include_kl::Int32
    xtol_abs::Float64
    ftol_rel::Float64
    gtol::Float64
    initial_delta::Float64
    delta_hat::Float64
    tr_secular_iters::Int32
    reserved::Int32
end

version() = ccall((:celeste_blend_version, LIB), Cint, ())
strerror(status) = unsafe_string(ccall((:celeste_blend_strerror, LIB), Cstring, (Cint,), status))

# problem: a celeste_problem_t built as for CelesteMI355X.ctx_create
function ctx_create(problem, device::Integer=0)
    out = Ref{Ptr{Void}}(C_NULL)
    st = ccall((:celeste_blend_ctx_create, LIB), Cint, (Ptr{Void}, Cint, Ptr{Ptr{Void}}), problem, device, out)
    st == 0 || error("celeste_blend_ctx_create: " * strerror(st))
    return out[]
end
ctx_destroy(ctx) = ccall((:celeste_blend_ctx_destroy, LIB), Void, (Ptr{Void},), ctx)

# blends: a vector of vectors of 0-based source ids
function blend_arrays(blends)
    off = zeros(Int64, length(blends) + 1)
    for (b, bl) in enumerate(blends)
        off[b + 1] = off[b] + length(bl)
    end
    return off, Int32[s for bl in blends for s in bl]
end

# elbo() with active_sources = each blend: per blend v, d (44 x Sa) and h ((44 Sa) x (44 Sa)) one after another
function eval_blends(ctx, vp::Matrix{Float64}, blends; flags::UInt32=UInt32(7))
    off, src = blend_arrays(blends)
    B = length(blends)
    sa = diff(off)
    v = zeros(B); d = zeros(44 * sum(sa)); h = zeros(sum((44 .* sa) .^ 2))
    cnt = zeros(Int64, 2 * B); status = zeros(Int32, B)
    st = ccall((:celeste_blend_eval, LIB), Cint,
               (Ptr{Void}, Ptr{Float64}, Int32, Ptr{Int64}, Ptr{Int32}, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                Ptr{Int64}, Ptr{Int32}),
               ctx, vp, B, off, src, flags, v, d, h, cnt, status)
    return st, v, d, h, cnt, status
end

# maximize! for every blend; vp (44 x S) is updated in place for the members
function maximize_blends!(ctx, vp::Matrix{Float64}, blends, cfg::OptimConfig; vp_neighbors=C_NULL, pos_centers=C_NULL)
    off, src = blend_arrays(blends)
    B = length(blends)
    its = zeros(Int32, B); evals = zeros(Int32, B); elbo = zeros(B); status = zeros(Int32, B)
    st = ccall((:celeste_blend_maximize, LIB), Cint,
               (Ptr{Void}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Int64}, Ptr{Int32}, Ref{OptimConfig},
                Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}),
               ctx, vp, vp_neighbors, pos_centers, B, off, src, cfg, its, evals, elbo, status)
    return st, its, evals, elbo, status
end

# device time of the last maximize_blends!: (evaluation ms, step ms, iterations)
function last_ms(ctx)
    ms = zeros(Float32, 3)
    st = ccall((:celeste_blend_last_ms, LIB), Cint, (Ptr{Void}, Ptr{Float32}), ctx, ms)
    return st, ms
end

# the sub-problem in any dimension up to 164 (test entry)
function tr_solve_batch(dims::Vector{Int32}, H::Vector{Float64}, g::Vector{Float64}, delta::Vector{Float64};
                        device::Integer=0, secular_iters::Integer=0)
    n = length(dims)
    p = zeros(length(g)); m = zeros(n); interior = zeros(Int32, n)
    st = ccall((:celeste_blend_tr_solve_batch, LIB), Cint,
               (Cint, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64},
                Ptr{Int32}),
               device, n, dims, H, g, delta, 0, secular_iters, p, m, interior)
    return st, p, m, interior
end

end # module
