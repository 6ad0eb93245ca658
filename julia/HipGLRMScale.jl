# HipGLRMScale.jl -- equilibrate_variance! / prob_scale! (src/modify_glrm.jl:31-82) on the device (include after HipGLRM.jl, next to
# HipGLRMExtras.jl).  One call of the scaling extension (include/glrm_hip_scale.h: glrm_hip_scale_columns) on the model's column view
# returns the NEW scales; they are applied here with the reference's own mul!, which sets the scale.  Not executed here (no julia).
module HipGLRMScale

using LowRankModels, SparseArrays
using ..HipGLRM
import ..HipGLRM: LIB, CLoss, CReg, CProblem, COptions, check, closs, creg, collapse, flatten, cols_from_csc, csc_is_omega, hip_release!

export hip_equilibrate_variance!, hip_prob_scale!

const SCALE_EQUILIBRATE = Int32(0)   # GLRM_SCALE_EQUILIBRATE
const SCALE_PROB = Int32(1)          # GLRM_SCALE_PROB

# (loss_scale, ry_scale) of every column, or nothing when some loss / regularizer is outside the header's tables or multi-dimensional
# (their M-estimators do not run in the reference either): the caller then runs the reference's function.
function scale_columns(glrm::GLRM, mode::Int32, device_id::Int)
    cl = map(closs, glrm.losses); cry = map(creg, glrm.ry)
    (any(isnothing, cl) || any(isnothing, cry) || any(c -> c.kind >= 9, cl)) && return nothing
    losses = collapse(Vector{CLoss}(cl)); ry = collapse(Vector{CReg}(cry)); rx = CReg[CReg(0, 0, 1.0)]
    A = glrm.A; m, n = size(A)
    colptr, _, colvals = (A isa SparseMatrixCSC && csc_is_omega(A, glrm.observed_examples)) ? cols_from_csc(A, glrm.losses) :
                         flatten(glrm.observed_examples, glrm.losses, (j, e) -> A[e, j], true)
    ls = Vector{Float64}(undef, n); rs = Vector{Float64}(undef, n)
    GC.@preserve losses rx ry colptr colvals begin
        prob = CProblem(m, n, glrm.k, 0, 0, m, 0, n, Ptr{Int64}(C_NULL), Ptr{Int32}(C_NULL), Ptr{Float64}(C_NULL),
                        pointer(colptr), Ptr{Int32}(C_NULL), pointer(colvals),
                        pointer(losses), length(losses), pointer(rx), length(rx), pointer(ry), length(ry), Ptr{Float64}(C_NULL), 0, 0, 0)
        opt = COptions(device_id, 0, 0, 0, C_NULL, 0, 0, 0, 0, 0, 0)
        check(ccall((:glrm_hip_scale_columns, LIB), Cint,
                    (Ref{CProblem}, Ref{COptions}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    prob, opt, mode, ls, rs, C_NULL, C_NULL, C_NULL))
    end
    ls, rs
end

"equilibrate_variance!(glrm, columns_to_scale) with the column statistics computed on the device; falls back to the reference."
function hip_equilibrate_variance!(glrm::GLRM, columns_to_scale=1:size(glrm.A, 2); device_id::Int=-1)
    r = scale_columns(glrm, SCALE_EQUILIBRATE, device_id)
    r === nothing && return LowRankModels.equilibrate_variance!(glrm, columns_to_scale)
    for i in columns_to_scale
        LowRankModels.mul!(glrm.losses[i], r[1][i]); LowRankModels.mul!(glrm.ry[i], r[2][i])
    end
    hip_release!(glrm)                          # the descriptors of a cached handle are stale
end

"prob_scale!(glrm, columns_to_scale) on the device (statistics over the observed entries of each column); falls back to the reference."
function hip_prob_scale!(glrm::GLRM, columns_to_scale=1:size(glrm.A, 2); device_id::Int=-1)
    r = scale_columns(glrm, SCALE_PROB, device_id)
    r === nothing && return LowRankModels.prob_scale!(glrm, columns_to_scale)
    for i in columns_to_scale
        LowRankModels.mul!(glrm.losses[i], r[1][i])
    end
    hip_release!(glrm)
end

end # module
