# HipGLRMRegVec.jl -- included by HipGLRM.jl (before HipGLRMHandle.jl): the regularizers that carry a vector -- fixed_latent_features,
# fixed_last_latent_features (src/regularizers.jl:193-231; fix_latent_features!, src/modify_glrm.jl:25-29) and RemQuadReg (:412-423) -- on
# the engine, through the extension header include/glrm_hip_regvec.h (outside the 37 symbols of include/glrm_hip.h, hence a file of its
# own like HipGLRMScale.jl).  The handle was created from placeholder descriptors (HipGLRMDescriptors.jl: placeholder, side); this hands it
# the descriptors with the vector codes and, per side, the k x count table of the vectors with one Int32 length per descriptor.  The shim
# no longer falls back to the reference solver for these types.  Not executed here (no julia).
struct CRegVec; vec::Ptr{Float64}; len::Ptr{Int32}; end      # glrm_regvec

# desc = (losses, rx placeholders, ry placeholders, (x = nothing | (descriptors, table, lengths), y = ...)).  A side without vectors still
# passes a table of zero lengths: a handle that is given one runs the general sweeps, whichever side holds the vectors.
function install_regvec!(h::Ptr{Cvoid}, multi::Bool, desc)
    k = size(something(desc[4].x, desc[4].y)[2], 1)
    full(v, ph) = v === nothing ? (ph, zeros(k, length(ph)), zeros(Int32, length(ph))) : v
    (rx, tx, lx), (ry, ty, ly) = full(desc[4].x, desc[2]), full(desc[4].y, desc[3])
    GC.@preserve rx tx lx ry ty ly begin
        vx, vy = Ref(CRegVec(pointer(tx), pointer(lx))), Ref(CRegVec(pointer(ty), pointer(ly)))
        check(multi ?                        # (a `ccall` target is a constant expression: one literal call per entry point)
              ccall((:glrm_hip_multi_set_regularizers_vec, LIB), Cint, (Ptr{Cvoid}, Ptr{CReg}, Int64, Ref{CRegVec}, Ptr{CReg}, Int64, Ref{CRegVec}),
                    h, rx, length(rx), vx, ry, length(ry), vy) :
              ccall((:glrm_hip_set_regularizers_vec, LIB), Cint, (Ptr{Cvoid}, Ptr{CReg}, Int64, Ref{CRegVec}, Ptr{CReg}, Int64, Ref{CRegVec}),
                    h, rx, length(rx), vx, ry, length(ry), vy))
    end
    h
end
