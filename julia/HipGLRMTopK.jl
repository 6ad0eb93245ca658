# HipGLRMTopK.jl -- precision_at_k (src/cross_validate.jl:243-304) without the dense XY (include after HipGLRM.jl, next to
# HipGLRMInit.jl).  The two calls of the top-k extension (include/glrm_hip_topk.h) on the train model's cached list handle replace
# `XY = X'*Y; q = sort(XY[:], rev=true)[ntrain]` (:273-274) and the double loop (:275-297); everything else is the reference's
# method, line for line.  Keyword arguments do not take part in dispatch, so the params are a third POSITIONAL argument here:
# `precision_at_k(train_glrm, test_observed_features, HipProxGradParams(); reg_params=..., kprec=10)`; the reference's own method
# (`params=` keyword) is left as it is and still runs its fits on the engine, with the dense XY on the host.  Not executed here (no julia).
module HipGLRMTopK

using LowRankModels
using ..HipGLRM
import ..HipGLRM: LIB, check, with_handle, HipProxGradParams
import LowRankModels: precision_at_k, GLRM, ConvergenceHistory, objective, fit!, mul!

export hip_xy_select, hip_precision_scan

"(q, n_gt, n_eq): q = sort((X'Y)[:], rev=true)[rank] under isless, the entries above it, the entries equal to it."
function hip_xy_select(glrm::GLRM, X::Matrix{Float64}, Y::Matrix{Float64}, rank::Integer; device_id::Int=-1)
    q = Ref{Float64}(NaN); gt = Ref{Int64}(0); eq = Ref{Int64}(0)
    r = with_handle(glrm, device_id) do h
        check(ccall((:glrm_hip_xy_select, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{Float64}, Ref{Int64}, Ref{Int64}),
                    h, X, Y, rank, q, gt, eq))
    end
    r === nothing && error("this model is outside the engine (see HipGLRMDescriptors.jl)")
    q[], gt[], eq[]
end

"(true_pos, false_pos) of the loop at src/cross_validate.jl:275-297 for the threshold q; test_observed_features holds 1-based columns."
function hip_precision_scan(train_glrm::GLRM, X::Matrix{Float64}, Y::Matrix{Float64}, q::Float64, test_observed_features, kprec::Integer;
                            device_id::Int=-1)
    rowptr = Int64[0; cumsum(map(length, test_observed_features))]
    colidx = Int32[j - 1 for row in test_observed_features for j in row]
    tp = Ref{Int64}(0); fp = Ref{Int64}(0)
    r = with_handle(train_glrm, device_id) do h
        check(ccall((:glrm_hip_precision_scan, LIB), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Int64}, Ptr{Int32}, Int64, Int64, Ref{Int64}, Ref{Int64},
                     Ptr{Int64}, Ptr{Int64}, Ptr{UInt8}, Ptr{Int64}),
                    h, X, Y, q, rowptr, colidx, kprec, 0, tp, fp, C_NULL, C_NULL, C_NULL, C_NULL))
    end
    r === nothing && error("this model is outside the engine (see HipGLRMDescriptors.jl)")
    tp[], fp[]
end

function precision_at_k(train_glrm::GLRM, test_observed_features, params::HipProxGradParams;
                        reg_params=exp10.(range(2, stop=-2, length=5)), holdout_proportion=.1, verbose=true,
                        ch::ConvergenceHistory=ConvergenceHistory("reg_path"), kprec=10)
    m, n = size(train_glrm.A)
    ntrain = sum(map(length, train_glrm.observed_features))
    np = length(reg_params)
    train_error = Array{Float64}(undef, np); test_error = Array{Float64}(undef, np); prec_at_k = Array{Float64}(undef, np)
    solution = Array{Tuple{Float64,Float64}}(undef, np); train_time = Array{Float64}(undef, np)
    test_glrm = GLRM(train_glrm.A, train_glrm.losses, train_glrm.rx, train_glrm.ry, train_glrm.k,
                     X=copy(train_glrm.X), Y=copy(train_glrm.Y), observed_features=test_observed_features)
    for iparam = 1:np
        reg_param = reg_params[iparam]
        mul!(train_glrm.rx, reg_param); mul!(train_glrm.ry, reg_param)
        train_glrm.X, train_glrm.Y = randn(train_glrm.k, m), randn(train_glrm.k, n)
        X, Y, ch = fit!(train_glrm, params, ch=ch, verbose=verbose)
        train_time[iparam] = ch.times[end]
        train_error[iparam] = objective(train_glrm, X, Y, include_regularization=false) / ntrain
        test_error[iparam] = objective(test_glrm, X, Y, include_regularization=false) / ntrain
        Xm, Ym = Matrix{Float64}(X), Matrix{Float64}(Y)
        q, _, _ = hip_xy_select(train_glrm, Xm, Ym, ntrain; device_id=params.device_id)                       # :273-274
        true_pos, false_pos = hip_precision_scan(train_glrm, Xm, Ym, q, test_observed_features, kprec; device_id=params.device_id)  # :275-297
        prec_at_k[iparam] = true_pos / (true_pos + false_pos)
        verbose && println("\tprec_at_k:  $(prec_at_k[iparam])")
        solution[iparam] = (sum(X) + sum(Y), sum(abs.(X)) + sum(abs.(Y)))
    end
    return train_error, test_error, prec_at_k, train_time, reg_params, solution
end

end # module
