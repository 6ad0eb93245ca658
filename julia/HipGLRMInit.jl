# HipGLRMInit.jl -- init_kmeanspp! (src/initialize.jl:8-33) on the device (include after HipGLRM.jl, next to HipGLRMExtras.jl and
# HipGLRMScale.jl).  One call of the initialization extension (include/glrm_hip_init.h: glrm_hip_init_kmeanspp) on the model's cached
# list handle; the random numbers are drawn HERE, from the caller's generator, in the order the reference consumes them: randn(k, n),
# sample(1:m), then one rand() per wsample.  Not executed here (no julia).
module HipGLRMInit

using LowRankModels, Random
using ..HipGLRM
import ..HipGLRM: LIB, check, with_handle, descriptors

export hip_init_kmeanspp!

"init_kmeanspp!(glrm) with the distances and the sampling on the device; falls back to the reference for models outside the engine."
function hip_init_kmeanspp!(glrm::GLRM; rng::AbstractRNG=Random.default_rng(), device_id::Int=-1)
    descriptors(glrm) === nothing && return LowRankModels.init_kmeanspp!(glrm)      # before a single number is drawn from rng
    m, n = size(glrm.A); k = glrm.k
    size(glrm.Y, 2) == n || error("init_kmeanspp! sets Y = randn(k, n): it has no slot for a multi-dimensional loss")
    Y = randn(rng, k, n)
    first = rand(rng, 1:m)
    u = rand(rng, k - 1)
    centers = Vector{Int64}(undef, k)
    with_handle(glrm, device_id) do h
        check(ccall((:glrm_hip_init_kmeanspp, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}),
                    h, Y, first - 1, u, centers, C_NULL))
    end
    glrm.Y = Y
    glrm
end

end # module
