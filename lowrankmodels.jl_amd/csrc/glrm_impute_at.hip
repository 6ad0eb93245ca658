// glrm_impute_at.hip -- include/glrm_hip_impute_at.h: glrm_hip_impute_at, the imputed values (and errors) of a list of entries -- pairs, whole
// rows or whole columns -- without anything m x n.  The value is glrm_hip_impute's: the ascending fma chain over the true k from +0.0 and
// impute_value (glrm_impute.hpp), so an entry has the bits it has in that matrix.
//
// The query modes, the blocks the entries go through the device in, their partition by path and the bodies of the two kernels that compute
// u are those of glrm_entries.hpp (shared with glrm_sample.hip); this unit adds what is done with u:
//   ImputeFin              impute_value on u, and with truth the entry's error
//   impute_at_fast_kernel / impute_at_general_kernel   ia_fast_body / ia_general_body with ImputeFin
//   ia_errsum_kernel       err_total: accumulator s of 65536 adds the errors of the entries t = s (mod 65536), ascending -- what the first
//                          stage of glrm_hip_sum would do with the whole err vector resident -- and glrm_hip_sum finishes the sum.
// Whether a queried column has no imputation rule is decided per COLUMN before anything runs (impute_value's own verdict, which does not
// depend on u), so a refusal writes nothing and a bad column nobody asks for is not an error.
#include "glrm_entries.hpp"

using namespace glrm;
using namespace glrm::entries;

namespace {

constexpr int IA_ACC = 65536;                     // accumulators of the ordered sum: the threads of glrm_hip_sum's first stage

struct ImputeFin {
  const double* truth;      // block-local, or nullptr
  double* err;              // block-local, or nullptr
  __device__ __forceinline__ void operator()(const IaArgs& a, int64_t e, int64_t, int64_t col, int d, const double* us, int stride) const {
    const LossDesc l = load_loss(a.losses, a.loss_single ? 0 : col);
    const glrm_domain D = a.domains[col];
    int bad = 0; // decided per column before the launch (ImputeBad)
    const double imp = impute_value(D, l, d, us, stride, &bad);
    a.out[e] = imp;
    if (err) err[e] = entry_error(D, imp, truth[e]);
  }
};

// does the column's pair have an imputation rule?  impute_value's verdict
struct ImputeBad {
  __device__ __forceinline__ bool operator()(const glrm_domain& D, const LossDesc& l, int d, const double* us, int stride) const {
    int bad = 0;
    (void)impute_value(D, l, d, us, stride, &bad);
    return bad != 0;
  }
};

__global__ void __launch_bounds__(IA_THREADS, 2) impute_at_fast_kernel(const IaArgs a, const ImputeFin fin) { ia_fast_body(a, fin); }
__global__ void __launch_bounds__(IA_GT) impute_at_general_kernel(const IaArgs a, const ImputeFin fin) { ia_general_body(a, fin); }

// acc[s] += the errors of the block's entries t = s (mod IA_ACC), ascending
__global__ void __launch_bounds__(IA_THREADS) ia_errsum_kernel(const double* err, int64_t t0, int64_t nb, double* acc) {
  const int64_t s = (int64_t)blockIdx.x * IA_THREADS + threadIdx.x;
  int64_t t = t0 - t0 % IA_ACC + s;
  if (t < t0) t += IA_ACC;
  double v = acc[s];
  for (; t < t0 + nb; t += IA_ACC) v += err[t - t0];
  acc[s] = v;
}

thread_local int64_t g_ia_blocks = 0, g_ia_fast = 0, g_ia_general = 0;

} // namespace

extern "C" int glrm_hip_impute_at_info(int64_t* blocks, int64_t* entries_fast, int64_t* entries_general) {
  if (blocks) *blocks = g_ia_blocks;
  if (entries_fast) *entries_fast = g_ia_fast;
  if (entries_general) *entries_general = g_ia_general;
  return GLRM_OK;
}

extern "C" int glrm_hip_impute_at(glrm_handle* h, const double* X, const double* Y, const glrm_domain* domains, const int64_t* rows, int64_t n_rows,
                                  const int32_t* cols, int64_t n_cols, int32_t mode, const double* truth, int64_t block_entries, double* out,
                                  double* err, double* err_total) {
  const char* const what = "glrm_hip_impute_at";
  int rc = xy_check_handle(h, what);
  if (rc) return rc;
  if ((rc = xy_check_factors(h, X, Y, what))) return rc;
  if ((rc = ia_check_shape(domains, rows, n_rows, cols, n_cols, mode, out, what))) return rc;
  if (!truth && (err || err_total)) return fail(GLRM_ERR_INVALID, "%s: err / err_total need truth", what);
  int64_t total = 0;
  if ((rc = ia_check_indices(h, domains, rows, n_rows, cols, n_cols, mode, block_entries, what, &total))) return rc;
  if (total == 0) {
    if (err_total) *err_total = 0.0;
    g_ia_blocks = 0; g_ia_fast = 0; g_ia_general = 0;
    return GLRM_OK;
  }

  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  hipStream_t st = h->stream;

  DevArena w;
  IaArgs a{};
  // the queried columns must have a rule
  {
    std::vector<uint8_t> bad_h;
    int64_t badcol = -1;
    if ((rc = ia_columns(h, w, a, domains, cols, n_cols, mode, n_rows, ImputeBad{}, bad_h, &badcol))) return rc;
    if (badcol >= 0)
      return fail(GLRM_ERR_UNSUPPORTED, "%s: column %lld is queried and its (domain, loss) pair has no imputation rule in the reference (src/impute_and_err.jl)", what, (long long)badcol);
  }

  TkFactors f{};
  if ((rc = tk_factors(h, X, Y, f))) return rc;
  a.X = f.X; a.Y = f.Y;

  // this unit's scratch: truth and err per entry, the accumulators of the ordered sum
  IaBlocks b;
  if ((rc = ia_blocks_alloc(h, w, a, rows, n_rows, cols, n_cols, mode, total, block_entries, (size_t)IA_ACC * 8, (truth ? 8 : 0) + (err || err_total ? 8 : 0), what, b)))
    return rc;
  double *d_truth = nullptr, *d_err = nullptr, *acc = nullptr;
  if (truth && (rc = w.alloc(&d_truth, (size_t)b.block))) return rc;
  if ((err || err_total) && (rc = w.alloc(&d_err, (size_t)b.block))) return rc;
  if (err_total) {
    if ((rc = w.alloc(&acc, (size_t)IA_ACC))) return rc;
    HIPCK(hipMemsetAsync(acc, 0, (size_t)IA_ACC * 8, st));
  }
  const ImputeFin fin{d_truth, d_err};

  int64_t nblocks = 0, n_fast = 0;
  for (int64_t t0 = 0; t0 < total; t0 += b.block, ++nblocks) {
    const int64_t nb = std::min(b.block, total - t0);
    if ((rc = ia_block_begin(st, a, b, rows, cols, t0, nb))) return rc;
    if (truth) HIPCK(hipMemcpyAsync(d_truth, truth + t0, (size_t)nb * 8, hipMemcpyHostToDevice, st));
    ia_block_launch(h, a, b, fin, impute_at_fast_kernel, impute_at_general_kernel);
    if (err_total) hipLaunchKernelGGL(ia_errsum_kernel, dim3(IA_ACC / IA_THREADS), dim3(IA_THREADS), 0, st, (const double*)d_err, t0, nb, acc);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(out + t0, b.d_out, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
    if (err) HIPCK(hipMemcpyAsync(err + t0, d_err, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
    int64_t nf = nb;
    if (b.multi) HIPCK(hipMemcpyAsync(&nf, b.d_nfast, 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    n_fast += nf;
  }
  if (err_total && (rc = glrm_hip_sum(h, acc, IA_ACC, err_total))) return rc;
  g_ia_blocks = nblocks; g_ia_fast = n_fast; g_ia_general = total - n_fast;
  return GLRM_OK;
}
