# HipGLRMImputeAt.jl -- impute_at / error_metric_at: the imputed values of listed entries, whole rows or whole columns, and their errors
# against held-out values (include after HipGLRM.jl and HipGLRMExtras.jl, next to HipGLRMRecommend.jl).  One call of the impute_at
# extension (include/glrm_hip_impute_at.h) on the model's cached list handle: the entries go through the device in blocks, nothing m x n
# anywhere, and every value has the bits the same entry has in hip_impute's matrix.  Rows and columns are 1-based on this side.  Not
# executed here (no julia).
module HipGLRMImputeAt

using LowRankModels
using ..HipGLRM
import ..HipGLRM: LIB, check, with_handle
import ..HipGLRMExtras: CDomain, cdomain
import LowRankModels: GLRM

export hip_impute_at, hip_error_metric_at, hip_impute_at_info

# rows === nothing: every row (a column slab); cols === nothing: every column (a row slab); both given: pairs
function impute_at_call(glrm::GLRM, rows, cols, truth, domains, device_id::Int)
    m, n = size(glrm.A)
    rows === nothing && cols === nothing && error("give rows, cols or both; every entry of the model is hip_impute(glrm)")
    rows0 = rows === nothing ? Int64[] : Int64[i - 1 for i in rows]
    cols0 = cols === nothing ? Int32[] : Int32[j - 1 for j in cols]
    mode = rows === nothing ? 2 : cols === nothing ? 1 : 0
    mode == 0 && length(rows0) != length(cols0) && error("pairs need as many rows as cols")
    shape = mode == 0 ? (length(rows0),) : mode == 1 ? (length(rows0), n) : (m, length(cols0))
    truth === nothing || size(truth) == shape || error("truth has size $(size(truth)), the queried entries $shape")
    doms = CDomain[cdomain(d) for d in domains]
    out = Array{Float64}(undef, shape)
    err = truth === nothing ? nothing : Array{Float64}(undef, shape)
    total = Ref{Float64}(0.0)
    r = with_handle(glrm, device_id) do h
        check(ccall((:glrm_hip_impute_at, LIB), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{CDomain}, Ptr{Int64}, Int64, Ptr{Int32}, Int64, Int32, Ptr{Float64}, Int64,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    h, Matrix{Float64}(glrm.X), Matrix{Float64}(glrm.Y), doms, mode == 2 ? C_NULL : rows0, length(rows0),
                    mode == 1 ? C_NULL : cols0, length(cols0), mode, truth === nothing ? C_NULL : Array{Float64}(truth), 0,
                    out, err === nothing ? C_NULL : err, truth === nothing ? C_NULL : total))
    end
    r === nothing && error("this model is outside the engine (see HipGLRMDescriptors.jl)")
    out, err, total[]
end

"The imputed values of the pairs (rows[t], cols[t]); with `cols = nothing` of the whole rows, with `rows = nothing` of the whole columns."
hip_impute_at(glrm::GLRM, rows, cols; domains=[l.domain for l in glrm.losses], device_id::Int=-1) =
    impute_at_call(glrm, rows, cols, nothing, domains, device_id)[1]

"(err, total): error_metric(domain, loss, u, truth) of every queried entry and their sum in index order (no standardization)."
function hip_error_metric_at(glrm::GLRM, rows, cols, truth; domains=[l.domain for l in glrm.losses], device_id::Int=-1)
    _, err, total = impute_at_call(glrm, rows, cols, truth, domains, device_id)
    err, total
end

"(blocks, entries_fast, entries_general) of this thread's last call: how many entries took the scalar-loss and the multi-dimensional path."
function hip_impute_at_info()
    b = Ref{Int64}(0); f = Ref{Int64}(0); g = Ref{Int64}(0)
    check(ccall((:glrm_hip_impute_at_info, LIB), Cint, (Ref{Int64}, Ref{Int64}, Ref{Int64}), b, f, g))
    b[], f[], g[]
end

end # module
