/*
 * glrm_hip_nmf.h -- the NMF initialization extension of libglrm_hip.so: init_nndsvd! on the handle's resident observation lists.
 *
 * An extension header like glrm_hip_init.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged, and
 * the CPU oracle has no counterpart.  A host that never calls it is unaffected.
 *
 * Reference interface replaced (paths relative to the LowRankModels.jl tree):
 *   glrm_hip_init_nndsvd <- init_nndsvd!(glrm; scale, zeroh, variant, max_iters)   src/initialize_nmf.jl, with NMF.jl's nndsvd
 *
 * NMF.jl is not part of the reference tree, so the routine is specified HERE (NNDSVD: Boutsidis & Gallopoulos 2007, every component
 * treated alike) and agreement with NMF.jl's own nndsvd is to a tolerance, never bit for bit.
 */
#ifndef GLRM_HIP_NMF_H
#define GLRM_HIP_NMF_H

#include "glrm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { GLRM_NNDSVD_STD = 0, GLRM_NNDSVD_A = 1, GLRM_NNDSVD_AR = 2 }; /* variant; AR is refused (its random draws are NMF.jl's own) */

/*
 * Scalar-loss models only (Y = H is k x n, indexed by data column).  With Omega the observed pairs, s_j = losses[j].scale when `scale`
 * is non-zero and 1 otherwise:
 *
 *   round 0     B_0[i, j] = s_j A[i, j] on Omega, 0 elsewhere (no mean is subtracted, no m n / |Omega| factor: those are init_svd!'s)
 *   SVD         (U, sigma, V) = the top-k singular triplets of B_t
 *   split       for every j = 1 .. k alike:  xp = |max(u_j, 0)|, xn = |max(-u_j, 0)|, yp, yn the same from v_j, mp = xp yp, mn = xn yn.
 *               mp >= mn:  c = sqrt(sigma_j mp),  W[i, j] = u_ij > 0 ? u_ij c / xp : v0,  H[j, i] = v_ij > 0 ? v_ij c / yp : v0
 *               otherwise the negative parts:  c = sqrt(sigma_j mn),  -u_ij c / xn where u_ij < 0,  -v_ij c / yn where v_ij < 0.
 *               The result does not depend on the sign the SVD gave a pair (u_j, v_j).
 *   v0          GLRM_NNDSVD_STD: 0.  GLRM_NNDSVD_A: mean(B_t) over all m n entries.
 *   zeroh       non-zero: H = 0 after the split.
 *   result      X = W' (k x m), Y = H (k x n)
 *   rounds      t = 1 .. max_iters (soft impute):  B_t = s_j A on Omega and X_{t-1}' Y_{t-1} elsewhere, then SVD and split again.
 *
 * B_t is never formed: B_t = P_Omega(s A - X'Y) + X'Y, a sparse matrix on the resident lists plus a rank-k term, and both products of
 * the subspace iteration (the one of glrm_hip_init_svd: block l = k + 8 capped at 128 and at min(m, n), Gram orthonormalization, Ritz
 * values, the same stopping rule and `seed`; svd_max_iter <= 0 means 60, svd_tol <= 0 means 1e-12) are formed from the two parts.  A
 * round t >= 1 writes the residual s_j a - <x_i, y_j> of every observation once per view: 8 bytes per observation and view of scratch.
 *
 * Duplicated pairs: the reference assigns into a matrix, so a pair listed twice counts once; the products here would add it twice.
 * Lists without a duplicated pair are the CALLER'S contract (the Python and Julia bindings check the lists they hold on the host).
 *
 *   X, Y             host, out: k x m and k x n, column-major
 *   singular_values  host, out or NULL: the k singular values of the last round
 *   split            host, out or NULL: 2 k doubles, (larger, smaller) of (mp, mn) per component in the last round -- how close a
 *                    choice between the positive and the negative parts was
 *   iters_done       host, out or NULL: max_iters + 1 counts, the subspace iterations of every round
 *
 * Works on a finalized, unsharded list handle.  Lists and loss table are read in place; the handle's factors, step sizes and
 * regularizers are left alone.  No floating-point atomics: every sum is a fixed tree whose shape depends on k, on a segment's own
 * length or on m / n / |Omega| only, and two calls with the same arguments return the same bits.
 *
 * Errors: GLRM_ERR_UNSUPPORTED for a dense (dense_A) handle, a float (storage = f32) handle, a loss with dim > 1, k > 128 and variant
 * GLRM_NNDSVD_AR; GLRM_ERR_INVALID for a NULL, deferred, unfinalized or sharded handle, NULL X or Y, k > min(m, n), an unknown variant
 * and a negative max_iters; GLRM_ERR_OOM names the size of the residual arrays.  The message is in glrm_hip_last_error().
 */
int glrm_hip_init_nndsvd(glrm_handle* h, double* X, double* Y, int32_t scale, int32_t zeroh, int32_t variant, int32_t max_iters,
                         int32_t svd_max_iter, double svd_tol, uint64_t seed, double* singular_values, double* split, int32_t* iters_done);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_NMF_H */
