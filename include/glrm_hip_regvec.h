/*
 * glrm_hip_regvec.h -- the regularizers of libglrm_hip.so that carry a VECTOR beside their 16-byte descriptor:
 * fixed_latent_features, fixed_last_latent_features and RemQuadReg.
 *
 * An extension header like glrm_hip_scale.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged (glrm_reg
 * stays 16 bytes), no existing entry point changes what it accepts, and the CPU oracle has no counterpart.  A host that never calls
 * it is unaffected.
 *
 * Reference interfaces replaced (paths relative to the LowRankModels.jl tree), for k-vectors:
 *   GLRM_WRAP_FIXED_FIRST <- fixed_latent_features(r, y)       src/regularizers.jl:193-210  (FixedLatentFeaturesConstraint(y): r = ZeroReg, :200)
 *   GLRM_WRAP_FIXED_LAST  <- fixed_last_latent_features(r, y)  src/regularizers.jl:214-231  (FixedLastLatentFeaturesConstraint(y), :221)
 *   GLRM_REG_REM_QUAD     <- RemQuadReg(scale, m)              src/regularizers.jl:412-423
 *   fix_latent_features!(glrm, n)                              src/modify_glrm.jl:25-29 is host code over these (ry[i] <- fixed_latent_features(ry[i], Y[1:n, i]))
 *
 * Semantics, transcribed literally (y has nfix entries, r is the base, u has k entries, 0-based).  Inside fit! the prox! call receives
 * a SubArray, so only the generic prox! -> prox is reachable (:34); the in-place methods at :203-207 / :224-228 are never selected.
 *   fixed_latent_features       prox(u, a)  = [y ; prox_r(u[nfix..k), a)]                                        (:202)
 *                               evaluate(v) = v[0..nfix) == y ? evaluate_r(v[nfix..k)) : Inf                      (:208)
 *   fixed_last_latent_features  prox(u, a)  = [prox_r(u[nfix..k), a) ; y]                                        (:223)
 *                               -- the base is fed the LAST k - nfix entries of u and its result lands in the FIRST k - nfix positions;
 *                               this is what the reference computes and it is reproduced, not repaired
 *                               evaluate(v) = v[k-nfix..k) == y ? evaluate_r(v[0..k-nfix)) : Inf                  (:229)
 *   The comparisons are exact, entry by entry (IEEE ==: -0.0 equals +0.0, a NaN in v gives Inf).
 *   RemQuadReg(s, m)            prox(u, a)_c = (u_c + ((2a) s) m_c) / (1 + (2a) s), a true division per entry     (:417-418)
 *                               evaluate(v)  = s sum_c (v_c - m_c)^2                                              (:423)
 *
 * The base of the two fixed wrappers is any kind in [0, GLRM_REG_KIND_END); it sees a vector of length k - nfix, so KSparseConstraint(r)
 * needs 1 <= r <= k - nfix, and OneSparseConstraint / UnitOneSparseConstraint need nfix < k (their argmax of an empty vector throws in
 * the reference).  1 <= nfix <= k; with nfix = k the base sees an empty vector.
 */
#ifndef GLRM_HIP_REGVEC_H
#define GLRM_HIP_REGVEC_H

#include "glrm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Codes that are valid ONLY in the two entry points below.  glrm_hip_create / glrm_hip_set_regularizers (and their multi forms) keep
 * answering GLRM_ERR_UNSUPPORTED for kind 10 and GLRM_ERR_INVALID for the two flags: a descriptor that needs a vector and arrives
 * without one is never accepted. */
#define GLRM_REG_REM_QUAD 10      /* glrm_reg.kind: RemQuadReg(scale, m), glrm_reg.scale = scale; wrap must be 0 */
#define GLRM_WRAP_FIXED_FIRST 16  /* glrm_reg.wrap: fixed_latent_features(r, y); kind / scale describe the base r */
#define GLRM_WRAP_FIXED_LAST 32   /* glrm_reg.wrap: fixed_last_latent_features(r, y) */

/* The vectors of one side's descriptors (count = n_rx or n_ry of the call). */
typedef struct glrm_regvec {
  const double* vec;   /* k x count, column-major: the vector of descriptor i starts at vec[i * k]; entries past len[i] are ignored */
  const int32_t* len;  /* count entries: nfix for the fixed wrappers (1..k), k for RemQuadReg, 0 for a descriptor that carries no vector */
} glrm_regvec;

/*
 * glrm_hip_set_regularizers with vectors.  rx / ry are as there (the counts must equal the handle's; one descriptor is broadcast to the
 * whole side, and so is its vector); vx / vy describe the vectors of rx / ry and may be NULL when no descriptor of that side needs one.
 * The handle copies everything: the caller's arrays may go after the call.  With vx == vy == NULL (and hence no vector-carrying
 * descriptor) the call is glrm_hip_set_regularizers.  A non-NULL vx or vy moves the handle to the general sweeps even when every length in
 * it is 0: a host that shards a problem itself (row / column ranges, glrm_signature) passes tables to EVERY shard as soon as ANY shard's
 * descriptors carry a vector, so that all shards add in the same order; glrm_hip_multi_set_regularizers_vec does this by construction.
 *
 * Which handles take it: those that take a wrapper -- observation lists (not the dense hand-over), k <= 64.  The handle then runs the
 * general sweeps (csrc/glrm_multi.hpp), where the segment's k-vector lives in LDS, in all three modes (line search, losses only, the
 * fixed step of glrm_hip_gradstep_x / _y) and in the penalties of glrm_hip_objective.  No speed is claimed for this path.
 *
 * Lifetime: the handle owns device copies of the tables, freed by glrm_hip_destroy and replaced by the next call.  A later plain
 * glrm_hip_set_regularizers replaces everything and drops the vectors.  glrm_hip_subset children inherit the parent's descriptors AND
 * vectors (a subset keeps m and n).  A failed call leaves the handle exactly as it was.
 *
 * Errors (message in glrm_hip_last_error()):
 *   GLRM_ERR_UNSUPPORTED  a new flag combined with another GLRM_WRAP_* flag (or both new flags); GLRM_REG_REM_QUAD with any wrap flag,
 *                         i.e. also as the base of a fixed wrapper; a vector-carrying ry on a column whose loss has dim > 1; a handle
 *                         with storage = f32 or sum_order = 1; the dense hand-over; k > 64
 *   GLRM_ERR_NONFINITE    a non-finite entry among the first len[i] entries of a vector
 *   GLRM_ERR_INVALID      NULL where a vector is needed, a length outside 1..k (fixed wrappers) / other than k (RemQuadReg) / other than
 *                         0 (no vector), KSparseConstraint(r) with r outside 1..k - nfix, an argmax base with nfix = k, wrong counts
 *   and everything glrm_hip_set_regularizers answers for the descriptors that carry no vector.
 */
int glrm_hip_set_regularizers_vec(glrm_handle* h, const glrm_reg* rx, int64_t n_rx, const glrm_regvec* vx, const glrm_reg* ry, int64_t n_ry,
                                  const glrm_regvec* vy);

/* The same on a multi handle (n_rx, n_ry as at glrm_hip_multi_create).  The descriptors AND the vectors are sliced per shard; every
 * shard's slice is checked before any shard is changed, like glrm_hip_multi_set_regularizers. */
int glrm_hip_multi_set_regularizers_vec(glrm_multi* mh, const glrm_reg* rx, int64_t n_rx, const glrm_regvec* vx, const glrm_reg* ry,
                                        int64_t n_ry, const glrm_regvec* vy);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_REGVEC_H */
