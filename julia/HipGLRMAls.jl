# HipGLRMAls.jl -- exact alternating least squares for quadratic models (include after HipGLRM.jl, next to HipGLRMTransform.jl):
# AlsParams <: AbstractParams and fit!(glrm, ::AlsParams) over the ALS extension (include/glrm_hip_als.h, which is the specification of
# the arithmetic).  An iteration is hip_als_solve!(h, 0) then hip_als_solve!(h, 1): every row of X, then every column of Y, lands on
# the exact minimiser of its part of the objective -- the row solve inside the reference's streaming_fit!
# (src/algorithms/quad_streaming.jl:53), with `scale * I` where that file has `2 * scale * I` (the header says why).  The history holds
# the FULL objective after every iteration; the stopping rule is src/algorithms/proxgrad.jl:210-213.  Y == 0 is a valid start.
# Not executed here (no julia).
module HipGLRMAls

using LowRankModels
using ..HipGLRM
import ..HipGLRM: LIB, check, with_handle
import LowRankModels: GLRM, AbstractParams, ConvergenceHistory, update_ch!, fit!

export AlsParams, hip_als_solve!, hip_als_info

const ALS_MAX_K = 64            # GLRM_ALS_MAX_K
const ALS_SOLVED = Int8(0)      # GLRM_ALS_SOLVED
const ALS_KEPT_SHORT = Int8(1)  # GLRM_ALS_KEPT_SHORT
const ALS_KEPT_PIVOT = Int8(2)  # GLRM_ALS_KEPT_PIVOT

struct AlsParams <: AbstractParams
    max_iter::Int
    abs_tol::Float64
    rel_tol::Float64
    device_id::Int
end
AlsParams(; max_iter=100, abs_tol=0.00001, rel_tol=0.0001, device_id=-1) = AlsParams(max_iter, abs_tol, rel_tol, device_id)

"side 0: every row of X against Y as it stands; side 1: every column of Y against X."
hip_als_solve!(h::Ptr{Cvoid}, side::Integer) =
    check(ccall((:glrm_hip_als_solve, LIB), Cint, (Ptr{Cvoid}, Int32), h, side))

"(solved, kept_short, kept_pivot, status) of the last hip_als_solve! of `side`; nseg = the side's segments."
function hip_als_info(h::Ptr{Cvoid}, side::Integer, nseg::Integer)
    s = Ref{Int64}(0); ks = Ref{Int64}(0); kp = Ref{Int64}(0)
    status = fill(Int8(-1), max(nseg, 1))
    check(ccall((:glrm_hip_als_info, LIB), Cint, (Ptr{Cvoid}, Int32, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ptr{Int8}), h, side, s, ks, kp, status))
    s[], ks[], kp[], status[1:nseg]
end

function fit!(glrm::GLRM, p::AlsParams; ch::ConvergenceHistory=ConvergenceHistory("AlsGLRM"), verbose=true, kwargs...)
    X = Matrix{Float64}(glrm.X); Y = Matrix{Float64}(glrm.Y)
    scaled_abs_tol = p.abs_tol * sum(map(length, glrm.observed_features))   # proxgrad.jl:72
    obj = Ref{Float64}(0.0)
    r = with_handle(glrm, p.device_id) do h
        check(ccall((:glrm_hip_objective, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Float64}), h, X, Y, 1, obj))
        update_ch!(ch, 0, obj[])                                  # :76
        t = time()
        for i in 1:p.max_iter
            hip_als_solve!(h, 0)
            hip_als_solve!(h, 1)
            check(ccall((:glrm_hip_get_factors, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h, X, Y))
            check(ccall((:glrm_hip_objective, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Float64}), h, X, Y, 1, obj))
            o = obj[]                                             # the FULL objective: losses and both penalties
            update_ch!(ch, time() - t, o)
            t = time()
            dec = ch.objective[end-1] - o                         # :210-213
            i > 10 && (dec < scaled_abs_tol || dec / o < p.rel_tol) && break
            verbose && i % 10 == 0 && println("Iteration $i: objective value = $o")
        end
        true
    end
    r === nothing && error("this model is outside the engine (see HipGLRMDescriptors.jl)")
    copyto!(glrm.X, X); copyto!(glrm.Y, Y)
    glrm.X, glrm.Y, ch
end

end # module
