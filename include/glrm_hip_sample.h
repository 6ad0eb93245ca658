/*
 * glrm_hip_sample.h -- the sampling extension of libglrm_hip.so: DRAWS from the fitted model at a LIST of entries (pairs, whole rows or
 * whole columns), computed on the device without anything m x n.  glrm_hip_impute_at returns point predictions; multiple imputation,
 * synthetic look-alike data and posterior-predictive checks need draws.  This is sample(glrm) / sample_missing(glrm) of the reference
 * (src/sample.jl) with three differences of kind: nothing m x n is formed, every draw is a pure function of
 * (seed, row, column, X, Y, lists) -- not of the blocking, the query order or the mode -- and the model is never written.
 *
 * An extension header like glrm_hip_impute_at.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged, and
 * the CPU oracle has no counterpart.  A host that never calls it is unaffected.  Handle, Factors, mode, rows, cols, the output layout,
 * block_entries and the 1 GiB scratch bound are those of glrm_hip_impute_at.h (its GLRM_IMPUTE_AT_* modes are used as they are).
 *
 * RANDOM NUMBERS.  Philox4x32-10 (Random123: multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten
 * rounds).  key = (seed & 0xffffffff, seed >> 32); counter = (row, col, 0, 0) (m, n <= 2^31 - 1).  Known answers:
 *     counter 0 0 0 0, key 0 0                                          -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *     counter ffffffff x 4, key ffffffff x 2                            -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *     counter 243f6a88 85a308d3 13198a2e 03707344, key a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
 * The output words w0..w3 give two uniforms in [0, 1):  U0 = ((((uint64)w1 << 32) | w0) >> 11) * 2^-53, U1 likewise from w3, w2.
 * Integer arithmetic and exact conversions: device and host agree bit for bit.  A pair queried twice gets the same draw; a fresh
 * replicate needs a fresh seed.
 *
 * SCORE.  u is the engine's one definition of an entry: u = +0.0; for c in 0 .. k-1: u = fma(X[c,i], Y[c,v], u) for each of the d
 * vectors v of column j (glrm_hip_topk.h), computed by the device function glrm_hip_impute_at uses.
 *
 * RULES, by what Julia dispatch selects for sample(domains[f], losses[f], U[e, yidxs[f]]) (src/sample.jl:159):
 *   S1  Real x QuadLoss (:31)                   u + z * sd_j,  z = sqrt(-2 * log(1 - U0)) * cos(6.283185307179586 * U1); plain
 *                                               multiplies and adds, nothing contracted
 *   S2  Bool x LogisticLoss (:36-38)            U0 <= 1 / (1 + exp(-u)) ? 1.0 : 0.0
 *   S3  Categorical x MultinomialLoss (:68-70)  wsample over p_v = exp(u_v), v = 1 .. d; the level
 *   S4  (Ordinal or Categorical) x any other multi-dimensional loss (:60-63, :75-78)
 *                                               wsample over p_l = exp(-evaluate(loss, u, l)), l = D.min .. D.max; the level l
 *   --  everything else                         impute(D, l, u), the bits of glrm_hip_impute_at: the reference's fallback
 *                                               sample(D, l, u) = impute(D, l, u) (:178) is what a scalar u reaches outside S1 and S2
 *                                               (its AbstractArray methods never match a Float64; its Ordinal x DiffLoss and Count
 *                                               methods compute what roundcutoff computes)
 * wsample(p), as glrm_hip_init.h states it: t = U0 * sum(p), the sum taken left to right in level order; the answer is the first
 * level whose left-to-right running sum reaches t, else the last (the walk `while cw < t && l < last`).  A zero or NaN sum therefore
 * returns the first level.  One thread adds the levels sequentially (two walks: the sum, then the search with the weights computed
 * again), so only the exponentials can differ from a host restatement.
 * The levels of S4 must lie inside the levels the loss defines (1 .. l.max: d for OvA, Multinomial and Ordistic, d + 1 for BvS and
 * MultinomialOrdinal); otherwise the column cannot be answered, like a pair without an imputation rule (the reference would throw).
 *
 * Deviations from the reference:
 *   - S4 returns D.min + index; the reference returns the 1-based index, the same wherever D.min = 1 (every default domain).
 *   - Bool x a multi-dimensional loss is refused.
 *   - A Real column is never silently switched to Ordinal for integer-typed data (:136-140): the caller passes the domains.
 *   - The model's loss scales are never written; the generator is not a global one.
 *
 * THE NOISE OF S1.  sample(glrm) sets noisevar to the column's mean squared residual over observed_examples[j] (:143-150) and draws
 * u + randn() / sqrt(noisevar); :30 says "l.scale should be 1/var", so the literal code puts the INVERSE of the residual spread into
 * the draw.  noise_rule selects:
 *   GLRM_SAMPLE_NOISE_RESIDUAL   sd_j = sqrt(v_j): the documented intent
 *   GLRM_SAMPLE_NOISE_REFERENCE  sd_j = 1 / sqrt(v_j): the literal line
 *   GLRM_SAMPLE_NOISE_GIVEN      sd_j = noise_sd_in[j]
 * v_j = (sum over the handle's column-view list of column j of (u_ej - A_ej)^2) / (the length of that list): one device pass, for the
 * Real x QuadLoss columns only, and only when its result is used (rule 0 or 1, and a queried entry lies in such a column or
 * noise_sd_out is asked for).  Every sum is taken in a fixed order that is a function of the column's length: no floating-point
 * atomics.  An empty column gives NaN; v_j = 0 gives what the arithmetic gives.
 *
 * KEEPING OBSERVED ENTRIES (sample_missing).  With keep_observed = 1 an entry whose column occurs in row i's resident ROW-VIEW list
 * returns the stored value of its first occurrence in list order, and kept[t] = 1.  The reference tests the column view; the row view
 * is what glrm_hip_row_topk excludes by.  The two are the same set for every model built from an observation list or a matrix.
 */
#ifndef GLRM_HIP_SAMPLE_H
#define GLRM_HIP_SAMPLE_H

#include "glrm_hip_impute_at.h"

#define GLRM_SAMPLE_NOISE_RESIDUAL 0
#define GLRM_SAMPLE_NOISE_REFERENCE 1
#define GLRM_SAMPLE_NOISE_GIVEN 2

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A draw for every queried entry, in index order t = 0 .. T-1 (mode, rows, cols, domains, block_entries, out: glrm_hip_impute_at.h).
 *
 *   seed           the key of the generator
 *   noise_rule     GLRM_SAMPLE_NOISE_*
 *   noise_sd_in    host, n values, under GLRM_SAMPLE_NOISE_GIVEN (read at the Real x QuadLoss columns); NULL otherwise
 *   keep_observed  0 or 1
 *   kept           host, T bytes, or NULL; only with keep_observed = 1
 *   noise_sd_out   host, n values, or NULL: the sd_j that were used -- NaN for the columns that are not Real x QuadLoss, noise_sd_in
 *                  echoed under GLRM_SAMPLE_NOISE_GIVEN.  A caller can pay for the pass once and pass the result back as noise_sd_in.
 *
 * Refusals (nothing is written): those of glrm_hip_impute_at, and GLRM_ERR_INVALID for a noise_rule outside 0 .. 2, noise_sd_in NULL
 * under GLRM_SAMPLE_NOISE_GIVEN or non-NULL otherwise, keep_observed outside {0, 1}, kept without keep_observed, keep_observed on a
 * handle without a row view;  GLRM_ERR_UNSUPPORTED if a QUERIED entry lies in a column that cannot be answered (no imputation rule
 * where the draw is the imputation, Bool x a multi-dimensional loss, S4 levels outside the loss's; such a column that no queried entry
 * touches is not an error).  T == 0 returns GLRM_OK and writes only noise_sd_out (where asked for).
 *
 * Mechanism: the blocks, the partition and the gather of glrm_hip_impute_at; the draw is made by the lane that holds u.  With
 * keep_observed a 16-lane group per entry then walks the row's list 16 at a time.  No waiting between workgroups, no global atomics.
 */
int glrm_hip_sample_at(glrm_handle* h, const double* X, const double* Y, const glrm_domain* domains,
                       const int64_t* rows, int64_t n_rows, const int32_t* cols, int64_t n_cols, int32_t mode,
                       uint64_t seed, int32_t noise_rule, const double* noise_sd_in, int32_t keep_observed,
                       int64_t block_entries, double* out, uint8_t* kept, double* noise_sd_out);

/*
 * Diagnostics of the calling thread's last successful glrm_hip_sample_at: the blocks, the entries of the scalar-loss and the
 * multi-dimensional path, the entries that kept their observed value, and the columns the variance pass computed v_j for (0: it did not
 * run).  Any pointer may be NULL.
 */
int glrm_hip_sample_at_info(int64_t* blocks, int64_t* entries_fast, int64_t* entries_general,
                            int64_t* entries_kept, int64_t* variance_columns);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_SAMPLE_H */
