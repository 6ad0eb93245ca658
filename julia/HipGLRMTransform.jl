# HipGLRMTransform.jl -- transform: embed new rows into a fitted model with Y held fixed (include after HipGLRM.jl, next to
# HipGLRMTopK.jl).  The reference's ScikitLearnBase.transform (src/scikitlearn.jl:94-102) builds `ry_fixed` and never passes it on, so
# it refits Y from a random start; this one is the outer loop of src/algorithms/proxgrad.jl:107-217 without STEP 2, with the
# inner_iter_X half-steps of an iteration as ONE call of the transform extension (include/glrm_hip_transform.h): rows of at most 104
# observations (208 at k <= 32) fetch their vectors of Y once for all of them.  The params are a second POSITIONAL argument, as in
# HipGLRMTopK.jl.  The recorded objective is sum(obj_by_col) of :205 -- the losses over the new rows plus the column penalties of the
# fixed Y, which the host evaluates once.  Not executed here (no julia).
module HipGLRMTransform

using LowRankModels
using ..HipGLRM
import ..HipGLRM: LIB, check, with_handle, HipProxGradParams
import LowRankModels: GLRM, ConvergenceHistory, update_ch!, evaluate

export transform, inverse_transform, hip_solve_x!, hip_solve_x_info

"inner_iter X half-steps of every row with Y as it stands (the step sizes are not reset)."
hip_solve_x!(h::Ptr{Cvoid}, inner_iter::Integer, min_stepsize::Float64) =
    check(ccall((:glrm_hip_solve_x, LIB), Cint, (Ptr{Cvoid}, Int64, Float64), h, inner_iter, min_stepsize))

"(fused, fused_rows, loop_rows) of the last hip_solve_x! on the handle."
function hip_solve_x_info(h::Ptr{Cvoid})
    fused = Ref{Int32}(0); fr = Ref{Int64}(0); lr = Ref{Int64}(0)
    check(ccall((:glrm_hip_solve_x_info, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int64}, Ref{Int64}), h, fused, fr, lr))
    fused[] != 0, fr[], lr[]
end

function transform(glrm::GLRM, A_new, p::HipProxGradParams; obs=nothing, rx=nothing, X0=nothing,
                   ch::ConvergenceHistory=ConvergenceHistory("HipProxGradGLRM-transform"))
    m = size(A_new, 1)
    if rx === nothing
        all(r -> r == glrm.rx[1], glrm.rx) || error("rx is required: the fitted model's rows do not all carry the same regularizer")
        rx = glrm.rx[1]
    end
    X = X0 === nothing ? randn(glrm.k, m) : Matrix{Float64}(X0)
    Y = Matrix{Float64}(glrm.Y)                                    # a copy: glrm.Y is not written
    new = obs === nothing ? GLRM(A_new, glrm.losses, rx, glrm.ry, glrm.k, X=X, Y=Y) :
                            GLRM(A_new, glrm.losses, rx, glrm.ry, glrm.k, X=X, Y=Y, obs=obs)
    py = sum(evaluate(new.ry[j], view(Y, :, j)) for j in 1:size(Y, 2))   # the column penalties: Y is fixed
    scaled_abs_tol = p.abs_tol * sum(map(length, new.observed_features))  # :72, the new rows' observations
    obj = Ref{Float64}(0.0)
    r = with_handle(new, p.device_id) do h
        check(ccall((:glrm_hip_objective, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Float64}), h, X, Y, 1, obj))
        check(ccall((:glrm_hip_reset_stepsizes, LIB), Cint, (Ptr{Cvoid}, Float64), h, p.stepsize))   # :69-70
        update_ch!(ch, 0, obj[])                                  # :76
        t = time()
        for i in 1:p.max_iter                                     # :107
            p.inner_iter_X > 1 && check(ccall((:glrm_hip_reset_stepsizes, LIB), Cint, (Ptr{Cvoid}, Float64), h, p.stepsize))  # :112-115
            hip_solve_x!(h, p.inner_iter_X, p.min_stepsize)       # :117-158, one call
            check(ccall((:glrm_hip_get_factors, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h, X, Y))
            check(ccall((:glrm_hip_objective, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Float64}), h, X, Y, 0, obj))
            o = obj[] + py                                        # obj = sum(obj_by_col) :205
            update_ch!(ch, time() - t, o)
            t = time()
            dec = ch.objective[end-1] - o                         # :210-213
            i > 10 && (dec < scaled_abs_tol || dec / o < p.rel_tol) && break
        end
        true
    end
    r === nothing && error("this model is outside the engine (see HipGLRMDescriptors.jl)")
    X, ch
end

"X_new' * glrm.Y (src/scikitlearn.jl:107)."
inverse_transform(glrm::GLRM, X_new) = X_new' * glrm.Y

end # module
