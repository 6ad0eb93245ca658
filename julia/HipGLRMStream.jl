# HipGLRMStream.jl -- the reference's streaming method on the device (include after HipGLRM.jl, next to HipGLRMAls.jl):
# hip_streaming_fit!(glrm, ::StreamingParams) and hip_streaming_impute_at over the streaming extension (include/glrm_hip_stream.h, which
# is the specification of the plan and of the arithmetic).  The first T0 rows initialise Y exactly as in
# src/algorithms/quad_streaming.jl:31-35 (keep_rows, init_svd!); rows T0+1 .. m are then visited once by hip_stream_rows!: rows that share
# no column run side by side, the division of Y is applied when a column is read.  The history gets one value per streamed row.
# StreamingParams is the reference's own type; there is no fit! method for it, as in the reference.
# Not executed here (no julia).
module HipGLRMStream

using LowRankModels
using ..HipGLRM
import ..HipGLRM: LIB, check, with_handle
import LowRankModels: GLRM, ConvergenceHistory, StreamingParams, keep_rows, init_svd!

export hip_stream_plan, hip_stream_rows!, hip_stream_info, hip_streaming_fit!, hip_streaming_impute_at

const STREAM_MAX_K = 64         # GLRM_STREAM_MAX_K

"The plan of rows first+1 .. m of a 0-based CSR row view (pure host code): (level, nlevels, nlaunches, max_width, dup_rows)."
function hip_stream_plan(m::Integer, n::Integer, first::Integer, rowptr::Vector{Int64}, colidx::Vector{Int32}; sequential::Bool=false)
    level = zeros(Int64, max(m - first, 1))
    nl = Ref{Int64}(0); nk = Ref{Int64}(0); mw = Ref{Int64}(0); dr = Ref{Int64}(0)
    check(ccall((:glrm_hip_stream_plan, LIB), Cint,
                (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Int32, Ptr{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                m, n, first, rowptr, colidx, C_NULL, C_NULL, sequential ? 1 : 0, level, nl, nk, mw, dr))
    level[1:(m - first)], nl[], nk[], mw[], dr[]
end

"Streams rows first+1 .. m over the resident X and Y; qptr (m + 1 offsets, 0-based) / qcol (0-based columns) are the queries of every row."
function hip_stream_rows!(h::Ptr{Cvoid}, m::Integer, first::Integer, stepsize::Real, interval::Integer;
                          sequential::Bool=false, qptr::Union{Nothing,Vector{Int64}}=nothing, qcol::Union{Nothing,Vector{Int32}}=nothing)
    objective = fill(NaN, max(m - first, 1))
    if qptr === nothing
        check(ccall((:glrm_hip_stream_rows, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Float64, Int64, Int32, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                    h, first, stepsize, interval, sequential ? 1 : 0, C_NULL, C_NULL, C_NULL, objective))
        return objective[1:(m - first)], Float64[]
    end
    qout = fill(NaN, max(qptr[end], 1))
    check(ccall((:glrm_hip_stream_rows, LIB), Cint,
                (Ptr{Cvoid}, Int64, Float64, Int64, Int32, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                h, first, stepsize, interval, sequential ? 1 : 0, qptr, qcol, qout, objective))
    objective[1:(m - first)], qout[1:qptr[end]]
end

"(solved, kept_short, kept_pivot, nlevels, nlaunches, max_width, plan_ms, status) of the last hip_stream_rows!; rows = the rows streamed."
function hip_stream_info(h::Ptr{Cvoid}, rows::Integer)
    v = [Ref{Int64}(0) for _ in 1:6]
    ms = Ref{Float64}(0.0)
    status = fill(Int8(-1), max(rows, 1))
    check(ccall((:glrm_hip_stream_info, LIB), Cint,
                (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Float64}, Ptr{Int8}),
                h, v[1], v[2], v[3], v[4], v[5], v[6], ms, status))
    v[1][], v[2][], v[3][], v[4][], v[5][], v[6][], ms[], status[1:rows]
end

function stream_pass!(glrm::GLRM, p::StreamingParams, qptr, qcol)
    m = size(glrm.A, 1)
    init_glrm = keep_rows(glrm, p.T0)                                 # quad_streaming.jl:31-35
    init_svd!(init_glrm)
    copy!(glrm.Y, init_glrm.Y)
    glrm.X[:, 1:p.T0] = init_glrm.X
    X = Matrix{Float64}(glrm.X); Y = Matrix{Float64}(glrm.Y)
    r = with_handle(glrm, -1) do h
        check(ccall((:glrm_hip_set_factors, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h, X, Y))
        out = hip_stream_rows!(h, m, p.T0, p.stepsize, p.Y_update_interval; qptr=qptr, qcol=qcol)
        check(ccall((:glrm_hip_get_factors, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h, X, Y))
        out
    end
    r === nothing && error("this model is outside the engine (see HipGLRMDescriptors.jl)")
    copyto!(glrm.X, X); copyto!(glrm.Y, Y)
    r
end

function hip_streaming_fit!(glrm::GLRM, p::StreamingParams=StreamingParams(); ch::ConvergenceHistory=ConvergenceHistory("StreamingGLRM"), verbose=true)
    objective, _ = stream_pass!(glrm, p, nothing, nothing)
    append!(ch.objective, objective)                                  # push!(ch.objective, norm(r) ^ 2), row by row (:58)
    glrm.X, glrm.Y, ch
end

"Imputed values at the listed entries (1-based rows > T0 and columns, any order), in the caller's order: x_i . y_j with Y as row i found it."
function hip_streaming_impute_at(glrm::GLRM, rows::Vector{Int}, cols::Vector{Int}, p::StreamingParams=StreamingParams())
    m = size(glrm.A, 1)
    order = sortperm(rows)                                            # stable: per-row lists in the caller's order
    qptr = zeros(Int64, m + 1)
    for i in rows
        qptr[i + 1] += 1
    end
    cumsum!(qptr, qptr)
    qcol = Int32.(cols[order] .- 1)
    _, qout = stream_pass!(glrm, p, qptr, qcol)
    values = similar(qout)
    values[order] = qout
    values
end

end # module
