# HipGLRMNmf.jl -- init_nndsvd! (src/initialize_nmf.jl) on the device (include after HipGLRM.jl, next to HipGLRMInit.jl).  One call of
# the NMF initialization extension (include/glrm_hip_nmf.h: glrm_hip_init_nndsvd) on the model's cached list handle: no dense m x n
# matrix, and the soft-impute rounds (max_iters > 0) never form X'Y.  NMF.jl is not needed: the routine is the one the header states
# (NNDSVD, every component alike), so it agrees with NMF.jl's nndsvd to a tolerance, not bit for bit.  Not executed here (no julia).
module HipGLRMNmf

using LowRankModels
using ..HipGLRM
import ..HipGLRM: LIB, check, with_handle, descriptors

export hip_init_nndsvd!

const VARIANTS = Dict(:std => Int32(0), :a => Int32(1), :ar => Int32(2))

"true when some list names an index twice: the reference assigns into a matrix (the pair counts once), the device products would add it twice"
has_duplicates(lists) = any(l -> length(unique(l)) != length(l), lists)

"init_nndsvd!(glrm; scale, zeroh, variant, max_iters) with the SVD, the split and the soft-impute rounds on the device."
function hip_init_nndsvd!(glrm::GLRM; scale::Bool=true, zeroh::Bool=false, variant::Symbol=:std, max_iters::Int=0,
                          svd_max_iter::Int=0, svd_tol::Float64=1e-10, seed::Integer=1, device_id::Int=-1)
    m, n = size(glrm.A); k = glrm.k
    descriptors(glrm) === nothing && error("init_nndsvd!: this model is outside the engine (losses or regularizers without a descriptor)")
    size(glrm.Y, 2) == n || error("init_nndsvd! sets glrm.Y = H (k x n): it has no slot for a multi-dimensional loss")
    haskey(VARIANTS, variant) || error("init_nndsvd!: unknown variant $variant")
    variant == :ar && error("init_nndsvd!: variant :ar fills the zeros with NMF.jl's own random draws, which cannot be restated; use :std or :a")
    max_iters >= 0 || error("init_nndsvd!: max_iters = $max_iters is negative")
    (has_duplicates(glrm.observed_features) || has_duplicates(glrm.observed_examples)) &&
        error("init_nndsvd! assigns the observed entries into a matrix: a pair is listed twice, which the device products would count twice")
    X = Matrix{Float64}(undef, k, m)
    Y = Matrix{Float64}(undef, k, n)
    sv = Vector{Float64}(undef, k)
    split = Matrix{Float64}(undef, 2, k)
    iters = Vector{Int32}(undef, max_iters + 1)
    with_handle(glrm, device_id) do h
        check(ccall((:glrm_hip_init_nndsvd, LIB), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Int32, Int32, Int32, Float64, UInt64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                    h, X, Y, Int32(scale), Int32(zeroh), VARIANTS[variant], Int32(max_iters), Int32(svd_max_iter), svd_tol, UInt64(seed), sv, split, iters))
    end
    glrm.X = X
    glrm.Y = Y
    glrm
end

end # module
