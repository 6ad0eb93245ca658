# HipGLRMRecommend.jl -- recommend: the k best columns of every queried row of X'Y, the row's observed columns left out (include after
# HipGLRM.jl, next to HipGLRMTopK.jl).  One call of the recommend extension (include/glrm_hip_recommend.h) on the model's cached list
# handle: one pass over the entries of X'Y on the device, nothing m x n anywhere.  Candidates are ranked by the key of the score
# descending, then by column ascending (the key of HipGLRMTopK.jl: isless, so a NaN score ranks first).  Rows and columns are 1-based
# on this side; a row with fewer than k candidates is padded with column 0 (the library's -1, plus one) and NaN.  Not executed here
# (no julia).
module HipGLRMRecommend

using LowRankModels
using ..HipGLRM
import ..HipGLRM: LIB, check, with_handle
import LowRankModels: GLRM

export hip_recommend

"(cols, scores): length(rows) x k, best first; cols[r, t] = 0 and scores[r, t] = NaN where row rows[r] has fewer than t candidates."
function hip_recommend(glrm::GLRM, rows::AbstractVector{<:Integer}; k::Integer=10, exclude_observed::Bool=true, device_id::Int=-1)
    X, Y = Matrix{Float64}(glrm.X), Matrix{Float64}(glrm.Y)
    rows0 = Int64[i - 1 for i in rows]
    nr = length(rows0)
    cols = Matrix{Int32}(undef, k, nr); vals = Matrix{Float64}(undef, k, nr)   # column-major k x nr = the library's row-major nr x k
    r = with_handle(glrm, device_id) do h
        check(ccall((:glrm_hip_row_topk, LIB), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Int64, Int32, Int32, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}),
                    h, X, Y, rows0, nr, k, exclude_observed ? 1 : 0, 0, cols, vals, C_NULL))
    end
    r === nothing && error("this model is outside the engine (see HipGLRMDescriptors.jl)")
    permutedims(cols .+ Int32(1)), permutedims(vals)
end

hip_recommend(glrm::GLRM; kw...) = hip_recommend(glrm, 1:size(glrm.A, 1); kw...)

end # module
