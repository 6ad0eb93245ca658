# HipGLRMCd.jl -- alternating cyclic coordinate descent for QuadLoss models whose regularizers are ZeroReg, QuadReg, OneReg or
# NonNegConstraint (include after HipGLRM.jl, next to HipGLRMAls.jl): CdParams <: AbstractParams and fit!(glrm, ::CdParams) over the
# coordinate-descent extension (include/glrm_hip_cd.h, which is the specification of the arithmetic).  An iteration is
# hip_cd_solve!(h, 0, sweeps) then hip_cd_solve!(h, 1, sweeps): every coordinate of every row of X, then of every column of Y, is set to
# the exact minimiser of its part of the objective with the rest held, `sweeps` times over.  The reference has no such solver.  The history
# holds the FULL objective after every iteration; the stopping rule is src/algorithms/proxgrad.jl:210-213.
# Not executed here (no julia).
module HipGLRMCd

using LowRankModels
using ..HipGLRM
import ..HipGLRM: LIB, check, with_handle
import LowRankModels: GLRM, AbstractParams, ConvergenceHistory, update_ch!, fit!

export CdParams, hip_cd_solve!, hip_cd_info

const CD_MAX_K = 64            # GLRM_CD_MAX_K
const CD_MAX_SWEEPS = 256      # GLRM_CD_MAX_SWEEPS
const CD_CONVERGED = Int8(1)   # GLRM_CD_CONVERGED
const CD_SKIPPED = Int8(2)     # GLRM_CD_SKIPPED

struct CdParams <: AbstractParams
    max_iter::Int
    sweeps::Int
    abs_tol::Float64
    rel_tol::Float64
    device_id::Int
end
CdParams(; max_iter=100, sweeps=4, abs_tol=0.00001, rel_tol=0.0001, device_id=-1) = CdParams(max_iter, sweeps, abs_tol, rel_tol, device_id)

"side 0: every row of X against Y as it stands; side 1: every column of Y against X; at most `sweeps` sweeps per segment."
hip_cd_solve!(h::Ptr{Cvoid}, side::Integer, sweeps::Integer) =
    check(ccall((:glrm_hip_cd_solve, LIB), Cint, (Ptr{Cvoid}, Int32, Int32), h, side, sweeps))

"(converged, skipped, sweeps_total, status, sweeps_run) of the last hip_cd_solve! of `side`; nseg = the side's segments."
function hip_cd_info(h::Ptr{Cvoid}, side::Integer, nseg::Integer)
    c = Ref{Int64}(0); s = Ref{Int64}(0); t = Ref{Int64}(0)
    status = fill(Int8(-1), max(nseg, 1))
    run = fill(Int32(-1), max(nseg, 1))
    check(ccall((:glrm_hip_cd_info, LIB), Cint, (Ptr{Cvoid}, Int32, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ptr{Int8}, Ptr{Int32}), h, side, c, s, t, status, run))
    c[], s[], t[], status[1:nseg], run[1:nseg]
end

function fit!(glrm::GLRM, p::CdParams; ch::ConvergenceHistory=ConvergenceHistory("CdGLRM"), verbose=true, kwargs...)
    X = Matrix{Float64}(glrm.X); Y = Matrix{Float64}(glrm.Y)
    scaled_abs_tol = p.abs_tol * sum(map(length, glrm.observed_features))   # proxgrad.jl:72
    obj = Ref{Float64}(0.0)
    r = with_handle(glrm, p.device_id) do h
        check(ccall((:glrm_hip_objective, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Float64}), h, X, Y, 1, obj))
        update_ch!(ch, 0, obj[])                                  # :76
        t = time()
        for i in 1:p.max_iter
            hip_cd_solve!(h, 0, p.sweeps)
            hip_cd_solve!(h, 1, p.sweeps)
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
