/*
 * glrm_hip_init.h -- the initialization extension of libglrm_hip.so: init_kmeanspp! on the handle's resident observation lists.
 *
 * An extension header like glrm_hip_scale.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged, and
 * the CPU oracle has no counterpart.  A host that never calls it is unaffected.  (glrm_hip_init_svd, the other initializer, is part
 * of the boundary header.)
 *
 * Reference interface replaced (paths relative to the LowRankModels.jl tree):
 *   glrm_hip_init_kmeanspp <- init_kmeanspp!(glrm)   src/initialize.jl:8-33, with StatsBase's sample / wsample
 */
#ifndef GLRM_HIP_INIT_H
#define GLRM_HIP_INIT_H

#include "glrm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * k-means++ seeding with missing data.  The reference sets glrm.Y = randn(k, n) -- k x n, indexed by DATA column, so the routine only
 * has a meaning when every loss is scalar (d == n) -- copies the observed entries of a uniformly drawn row into row 1 of Y and then,
 * for l = 1 .. k-1, draws the next centre with probability proportional to
 *     w[i] = min_{ll <= l} ( sum_{j in obs(i)} evaluate(L_j, Y[ll, j], A[i, j]) ) / |obs(i)|
 * and copies its observed entries into row l+1.  Quirks that are kept: only the FIRST centre is taken out of the candidate set
 * (w = 0 for that row alone; later centres keep their computed weight); a row without observations has w = 0/0 = NaN; entries of a
 * centre's row that the centre does not observe keep their randn value; a column listed twice in a centre's row is assigned twice
 * in list order, so the last listed value stays.  X is not touched.
 *
 * The caller owns all randomness, which makes the call deterministic and lets a host pass the draws of its own generator:
 *   Y             host, k x n, column-major (Y[l + k j]).  In: the randn(k, n) draw.  Out: the initialized factor.
 *   first_center  0-based, the sample(1:m) draw.
 *   u             k-1 uniform draws in [0, 1); u[l-1] belongs to round l.  May be NULL when k == 1.
 *   centers       out, k row indices, 0-based; centers[0] == first_center.
 *   weights       out or NULL: the w vector of every round, (k-1) x m, round l at weights + (l-1) m.  For tests and diagnostics at
 *                 small sizes (it is kept on the device until the end of the call).
 *
 * The draw of round l is wsample(1:m, w):  t = u S with S = sum(w); the first row whose running sum of w reaches t, else row m-1.
 * A draw of 0, S == 0 and a NaN S (some row without observations, a non-finite loss) all give row 0.  Here the running sum is
 * hierarchical -- S and the sums of blocks of rows are fixed trees, the walk descends block by block with the reference's loop
 * `while cw < t && i < last` at every level -- so the chosen row is the reference's whenever t is not within rounding of a boundary
 * of the cumulative weights.
 *
 * Every row's distance to centre ll has the same bits in every round (row ll of Y never changes once it is set), so the engine keeps
 * a running minimum per row and evaluates ONE new distance per row and round: |Omega| k loss evaluations instead of the reference's
 * |Omega| k^2 / 2, with the same minimum bit for bit.
 *
 * Works on a finalized, unsharded list handle, like glrm_hip_init_svd.  The handle's rowptr / colidx / rowvals and loss table are
 * read in place; nothing is uploaded but Y and u, and the handle's own factors and step sizes are left alone.  The k-1 rounds are
 * enqueued on the handle's stream without a host round trip (the sampled row stays on the device, where the next scatter reads it);
 * the call returns after centers, Y and weights have been copied out.
 *
 * Determinism: two calls with the same arguments on the same handle return the same bits -- every sum is a fixed-shape tree whose
 * shape depends on the row's own length (the distances) or on m (the sampler) only, and a duplicated column is resolved by list
 * position, never by arrival order.  Handles created with different sweep-family options may hold a row's list in a different order
 * (tile order); a row's sum may then differ in its last bits.  centers and Y still agree whenever no draw lands within rounding of
 * a boundary of the cumulative weights, and Y holds only copied data values and untouched input values, so given equal centres it
 * is bit-equal.
 *
 * Errors: GLRM_ERR_UNSUPPORTED for a model with a multi-dimensional loss (dim > 1: the reference's Y = randn(k, n) has no slot for
 * it) and for a dense (dense_A) handle; GLRM_ERR_INVALID for a NULL, deferred, unfinalized or sharded handle, NULL Y or centers,
 * NULL u with k > 1, first_center outside [0, m) and a draw outside [0, 1); the message is in glrm_hip_last_error().
 */
int glrm_hip_init_kmeanspp(glrm_handle* h, double* Y, int64_t first_center, const double* u, int64_t* centers, double* weights);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_INIT_H */
