# HipGLRMSample.jl -- sample_at / sample_missing_at: draws from the fitted model at listed entries, whole rows or whole columns (include
# after HipGLRM.jl and HipGLRMExtras.jl, next to HipGLRMImputeAt.jl).  One call of the sampling extension (include/glrm_hip_sample.h, which
# states the generator, the rules and the deviations from src/sample.jl) on the model's cached list handle: nothing m x n anywhere, and
# every draw is a function of (seed, row, column, X, Y, lists) -- Julia's global generator is not used, and the model's loss scales are
# not written.  Rows and columns are 1-based on this side.  Not executed here (no julia).
module HipGLRMSample

using LowRankModels
using ..HipGLRM
import ..HipGLRM: LIB, check, with_handle
import ..HipGLRMExtras: CDomain, cdomain
import LowRankModels: GLRM

export hip_sample_at, hip_sample_missing_at, hip_sample_at_info

const NOISE = Dict(:residual => 0, :reference => 1, :given => 2)

# rows === nothing: every row (a column slab); cols === nothing: every column (a row slab); both given: pairs
function sample_at_call(glrm::GLRM, rows, cols, seed::UInt64, noise::Symbol, noise_sd, keep_observed::Bool, domains, device_id::Int)
    m, n = size(glrm.A)
    rows === nothing && cols === nothing && error("give rows, cols or both; every entry of the model is sample(glrm)")
    rows0 = rows === nothing ? Int64[] : Int64[i - 1 for i in rows]
    cols0 = cols === nothing ? Int32[] : Int32[j - 1 for j in cols]
    mode = rows === nothing ? 2 : cols === nothing ? 1 : 0
    mode == 0 && length(rows0) != length(cols0) && error("pairs need as many rows as cols")
    noise_sd === nothing || (noise = :given)
    noise == :given && noise_sd === nothing && error("noise = :given needs noise_sd, one value per column")
    noise_sd === nothing || length(noise_sd) == n || error("noise_sd has $(length(noise_sd)) values for $n columns")
    shape = mode == 0 ? (length(rows0),) : mode == 1 ? (length(rows0), n) : (m, length(cols0))
    doms = CDomain[cdomain(d) for d in domains]
    out = Array{Float64}(undef, shape)
    kept = keep_observed ? zeros(UInt8, shape) : nothing
    sd = Vector{Float64}(undef, n)
    r = with_handle(glrm, device_id) do h
        check(ccall((:glrm_hip_sample_at, LIB), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{CDomain}, Ptr{Int64}, Int64, Ptr{Int32}, Int64, Int32, UInt64, Int32,
                     Ptr{Float64}, Int32, Int64, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}),
                    h, Matrix{Float64}(glrm.X), Matrix{Float64}(glrm.Y), doms, mode == 2 ? C_NULL : rows0, length(rows0),
                    mode == 1 ? C_NULL : cols0, length(cols0), mode, seed, NOISE[noise],
                    noise_sd === nothing ? C_NULL : Vector{Float64}(noise_sd), keep_observed ? 1 : 0, 0,
                    out, kept === nothing ? C_NULL : kept, sd))
    end
    r === nothing && error("this model is outside the engine (see HipGLRMDescriptors.jl)")
    out, kept === nothing ? nothing : kept .!= 0, sd
end

"A draw at the pairs (rows[t], cols[t]); with `cols = nothing` at the whole rows, with `rows = nothing` at the whole columns.  `seed` is required."
hip_sample_at(glrm::GLRM, rows, cols; seed::Integer, noise::Symbol=:residual, noise_sd=nothing, keep_observed::Bool=false,
              domains=[l.domain for l in glrm.losses], device_id::Int=-1) =
    sample_at_call(glrm, rows, cols, UInt64(seed), noise, noise_sd, keep_observed, domains, device_id)[1]

"hip_sample_at with the observed entries (the resident row view's) keeping their stored values: (out, kept)."
function hip_sample_missing_at(glrm::GLRM, rows, cols; seed::Integer, noise::Symbol=:residual, noise_sd=nothing,
                               domains=[l.domain for l in glrm.losses], device_id::Int=-1)
    out, kept, _ = sample_at_call(glrm, rows, cols, UInt64(seed), noise, noise_sd, true, domains, device_id)
    out, kept
end

"(blocks, entries_fast, entries_general, entries_kept, variance_columns) of this thread's last call."
function hip_sample_at_info()
    b = Ref{Int64}(0); f = Ref{Int64}(0); g = Ref{Int64}(0); k = Ref{Int64}(0); v = Ref{Int64}(0)
    check(ccall((:glrm_hip_sample_at_info, LIB), Cint, (Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), b, f, g, k, v))
    b[], f[], g[], k[], v[]
end

end # module
