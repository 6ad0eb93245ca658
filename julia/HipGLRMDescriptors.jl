# HipGLRMDescriptors.jl -- included by HipGLRM.jl: the reference's loss / regularizer TYPES as the descriptor tables of
# include/glrm_hip.h (glrm_loss: kind, dim, scale, p0, p1; glrm_reg: kind, wrap, scale) and of include/glrm_hip_regvec.h (the three regularizers
# that carry a vector: their descriptors, placeholders and tables), and the test "does the engine take this
# model?" (anything else falls back to the reference solver: src/algorithms/proxgrad.jl).  Pure table look-ups.
import LowRankModels: Loss, Regularizer, QuadLoss, L1Loss, HuberLoss, QuantileLoss, PeriodicLoss, PoissonLoss, OrdinalHingeLoss,
                      LogisticLoss, WeightedHingeLoss, MultinomialLoss, OvALoss, BvSLoss, OrdisticLoss, MultinomialOrdinalLoss,
                      embedding_dim, ZeroReg, QuadReg, OneReg, NonNegConstraint, UnitOneSparseConstraint,
                      QuadConstraint, NonNegOneReg, OneSparseConstraint, KSparseConstraint, SimplexConstraint,
                      lastentry1, lastentry_unpenalized, OrdinalReg, MNLOrdinalReg,
                      fixed_latent_features, fixed_last_latent_features, RemQuadReg

closs(l::QuadLoss) = CLoss(0, 0, l.scale, 0, 0)                               # src/losses.jl:138-148
closs(l::L1Loss) = CLoss(1, 0, l.scale, 0, 0)                                 # :152-162
closs(l::HuberLoss) = CLoss(2, 0, l.scale, l.crossover, 0)                    # :166-179
closs(l::QuantileLoss) = CLoss(3, 0, l.scale, l.quantile, 0)                  # :186-203
closs(l::PeriodicLoss) = CLoss(4, 0, l.scale, l.T, 0)                         # :209-224
closs(l::PoissonLoss) = CLoss(5, 0, l.scale, 0, 0)                            # :231-243
closs(l::OrdinalHingeLoss) = CLoss(6, 0, l.scale, l.min, l.max)               # :247-294
closs(l::LogisticLoss) = CLoss(7, 0, l.scale, 0, 0)                           # :298-311
closs(l::WeightedHingeLoss) = CLoss(8, 0, l.scale, l.case_weight_ratio, 0)    # :317-352
# multi-dimensional losses (src/losses.jl:360-620): dim columns of Y per column of A; bin_loss must be Logistic / Hinge
binkind(b::LogisticLoss) = 7.0
binkind(b::WeightedHingeLoss) = b.case_weight_ratio == 1 ? 8.0 : NaN
binkind(b) = NaN
closs(l::MultinomialLoss) = CLoss(9, l.max, l.scale, 0, 0)
closs(l::OvALoss) = isnan(binkind(l.bin_loss)) ? nothing : CLoss(10, l.max, l.scale, l.bin_loss.scale, binkind(l.bin_loss))
closs(l::BvSLoss) = isnan(binkind(l.bin_loss)) ? nothing : CLoss(11, l.max - 1, l.scale, l.bin_loss.scale, binkind(l.bin_loss))
closs(l::OrdisticLoss) = CLoss(12, l.max, l.scale, 0, 0)
closs(l::MultinomialOrdinalLoss) = CLoss(13, l.max - 1, l.scale, 0, 0)
closs(l::Loss) = nothing                     # anything else: reference path
creg(r::ZeroReg) = CReg(0, 0, 1.0)                                            # src/regularizers.jl:91-97
creg(r::QuadReg) = CReg(1, 0, r.scale)                                        # :52-58
creg(r::OneReg) = CReg(2, 0, r.scale)                                         # :79-88
creg(r::NonNegConstraint) = CReg(3, 0, 1.0)                                   # :101-114
creg(r::UnitOneSparseConstraint) = CReg(4, 0, 1.0)                            # :295-318
# the vector regularizers (GLRM_REG_QUAD_CONSTRAINT .. GLRM_REG_SIMPLEX): k-vectors only, see vector_ok below
creg(r::QuadConstraint) = CReg(5, 0, r.max_2norm)                             # :68-76
creg(r::NonNegOneReg) = CReg(6, 0, r.scale)                                   # :118-138
creg(r::OneSparseConstraint) = CReg(7, 0, 1.0)                                # :235-255
creg(r::KSparseConstraint) = CReg(8, 0, Float64(r.k))                         # :258-291
creg(r::SimplexConstraint) = CReg(9, 0, 1.0)                                  # :323-348
# wrappers around one of the base regularizers (src/regularizers.jl:163-189,356-411)
wrapped(r, flag) = (b = creg(r.r); (b === nothing || b.wrap != 0 || b.kind == 10) ? nothing : CReg(b.kind, flag, b.scale))
creg(r::lastentry1) = wrapped(r, 1)
creg(r::lastentry_unpenalized) = wrapped(r, 2)
creg(r::OrdinalReg) = wrapped(r, 4)
creg(r::MNLOrdinalReg) = wrapped(r, 8)
# the regularizers that carry a vector (include/glrm_hip_regvec.h: GLRM_WRAP_FIXED_FIRST = 16, GLRM_WRAP_FIXED_LAST = 32, GLRM_REG_REM_QUAD = 10).
# These codes only go to glrm_hip_set_regularizers_vec (julia/HipGLRMRegVec.jl); glrm_hip_create gets placeholder(c)
creg(r::fixed_latent_features) = wrapped(r, 16)                               # :193-210
creg(r::fixed_last_latent_features) = wrapped(r, 32)                          # :214-231
creg(r::RemQuadReg) = CReg(10, 0, r.scale)                                    # :412-423
creg(r::Regularizer) = nothing
regvec(r::Union{fixed_latent_features,fixed_last_latent_features}) = r.y
regvec(r::RemQuadReg) = r.m
regvec(r::Regularizer) = nothing
carries(c) = c.kind == 10 || c.wrap & 48 != 0
placeholder(c) = c.kind == 10 ? CReg(0, 0, 1.0) : CReg(c.kind, c.wrap & ~Int32(48), c.scale)

isclass(l) = l isa LogisticLoss || l isa WeightedHingeLoss
value(l, a) = isclass(l) ? (a isa Bool ? Float64(a) : Float64(LowRankModels.myBool(Int(a)))) : Float64(a)   # src/losses.jl:104-106
collapse(v) = all(==(v[1]), v) ? v[1:1] : v          # one descriptor when every column / row carries the same one

fallback(glrm, p; kw...) = fit!(glrm, ProxGradParams(p.stepsize; max_iter=p.max_iter, inner_iter_X=p.inner_iter_X, inner_iter_Y=p.inner_iter_Y,
                                             abs_tol=p.abs_tol, rel_tol=p.rel_tol, min_stepsize=p.min_stepsize); kw...)

# A vector regularizer the engine takes: not under OrdinalReg / MNLOrdinalReg, not on the block of a multi-dimensional column (dim > 1),
# KSparseConstraint(r) with 1 <= r <= the length its base sees, QuadConstraint with a finite max_2norm > 0.  Where this fails the
# reference throws inside fit! (sort / partialsortperm on a matrix, BoundsError) or divides by zero: it is left to do so.
function vector_ok(c, k, dim)
    (c.kind < 5 || carries(c)) && return true      # (the vector-carrying ones: carrier_ok)
    (c.wrap & 12 != 0 || dim > 1) && return false
    len = c.wrap != 0 ? k - 1 : k
    c.kind == 8 && return 1 <= c.scale <= len
    c.kind == 5 && return 0 < c.scale < Inf
    true
end

# A vector-carrying regularizer the engine takes (what glrm_hip_set_regularizers_vec checks): a k-vector (dim == 1), 1 <= nfix <= k or a mean
# of length k, finite entries, and a base that can run on the k - nfix entries it sees.  Where this fails the reference is left to throw.
function carrier_ok(c, v, k, dim)
    carries(c) || return true
    (dim > 1 || !all(isfinite, v)) && return false
    c.kind == 10 && return length(v) == k
    sub = k - length(v)
    (1 <= length(v) <= k) || return false
    c.kind == 8 && return 1 <= c.scale <= sub
    c.kind == 5 && return 0 < c.scale < Inf
    (c.kind == 4 || c.kind == 7) && return sub >= 1
    true
end

# one side: (descriptors glrm_hip_create takes, nothing | (descriptors with the new codes, k x count table, lengths)); ONE entry when every
# row / column carries the same regularizer AND the same vector
function side(cr, vs, k)
    one = all(==(cr[1]), cr) && all(==(vs[1]), vs)
    cr, vs = one ? (cr[1:1], vs[1:1]) : (cr, vs)
    any(carries, cr) || return Vector{CReg}(cr), nothing
    table = zeros(k, length(cr)); lens = zeros(Int32, length(cr))
    for (i, v) in enumerate(vs)
        v === nothing && continue
        lens[i] = length(v); table[1:length(v), i] = v
    end
    Vector{CReg}(map(placeholder, cr)), (Vector{CReg}(cr), table, lens)
end

# descriptors of a model, or nothing if some loss / regularizer type is outside include/glrm_hip.h and include/glrm_hip_regvec.h:
# (losses, rx, ry, vec) with vec = nothing or (x = side's vectors | nothing, y = ...) for glrm_hip_set_regularizers_vec
function descriptors(glrm::GLRM)
    cl = map(closs, glrm.losses); crx = map(creg, glrm.rx); cry = map(creg, glrm.ry)
    (any(isnothing, cl) || any(isnothing, crx) || any(isnothing, cry)) && return nothing
    (all(c -> vector_ok(c, glrm.k, 1), crx) && all(j -> vector_ok(cry[j], glrm.k, max(cl[j].dim, 1)), eachindex(cry))) || return nothing
    vrx = map(regvec, glrm.rx); vry = map(regvec, glrm.ry)
    (all(i -> carrier_ok(crx[i], vrx[i], glrm.k, 1), eachindex(crx)) &&
     all(j -> carrier_ok(cry[j], vry[j], glrm.k, max(cl[j].dim, 1)), eachindex(cry))) || return nothing
    n = size(glrm.A, 2)
    general = embedding_dim(glrm.losses) != n || any(c -> c.wrap != 0 || c.kind == 10, crx) || any(c -> c.wrap != 0 || c.kind == 10, cry)
    (general && glrm.k > 64) && return nothing
    (rx, vx), (ry, vy) = side(crx, vrx, glrm.k), side(cry, vry, glrm.k)
    collapse(Vector{CLoss}(cl)), rx, ry, (vx === nothing && vy === nothing) ? nothing : (x = vx, y = vy)
end

# the dense hand-over applies when every entry is observed (the constructor's default UnitRanges) under one QuadLoss
fully_observed(glrm) = (s = size(glrm.A); all(==(1:s[2]), glrm.observed_features) && all(==(1:s[1]), glrm.observed_examples))
dense_ok(glrm, desc, p) = p.dense && glrm.A isa Matrix{Float64} && length(desc[1]) == 1 && desc[1][1].kind == 0 && desc[4] === nothing &&
                          9 <= glrm.k <= 64 && fully_observed(glrm)   # (vector-carrying regularizers run on the general sweeps)
