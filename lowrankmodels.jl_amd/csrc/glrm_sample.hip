// glrm_sample.hip -- include/glrm_hip_sample.h: glrm_hip_sample_at, a draw from the fitted model at every entry of a list -- pairs, whole
// rows or whole columns -- without anything m x n.  The header is the specification (generator, rules S1 .. S4, wsample, the noise of
// S1, keep_observed); this file is its mechanism.
//
// The query modes, the blocks, their partition by path and the bodies of the two kernels that compute u are those of glrm_entries.hpp
// (shared with glrm_impute_at.hip; sample_at_fast_kernel / sample_at_general_kernel wrap them here); what this unit adds:
//   SampleFin              the draw, made by the lane that holds u: Philox4x32-10 on (seed, row, column) -- about 40 integer multiplies
//                          -- and then at most one exp, or one log + sqrt + cos, per scalar entry; the two level walks of wsample per
//                          entry of a multi-dimensional column (the weights are computed again in the second walk: levels are
//                          unbounded, nothing is kept in a local array)
//   SampleBad              the per-column verdict: impute_value's where the draw is the imputation, the levels of S4 against the
//                          loss's, Bool x a multi-dimensional loss
//   sa_variance_kernel     v_j and sd_j of the Real x QuadLoss columns: one workgroup per column, thread t adds the squared residuals of
//                          the list positions t, t + 256, .. ascending, then a fixed tree over the 256 partial sums -- an order that is a
//                          function of the column's length, no atomics
//   sa_keep_kernel         keep_observed: a 16-lane group per entry walks the row's row-view list 16 at a time; the first occurrence of
//                          the column in list order overwrites the draw with the stored value
#include "../../include/glrm_hip_sample.h"
#include "glrm_entries.hpp"
#include "glrm_fastmath.hpp"

using namespace glrm;
using namespace glrm::entries;

namespace {

constexpr int SA_VT = 256;  // variance pass: threads per column
constexpr int SA_KG = 16;   // keep pass: lanes per entry

// ---- Philox4x32-10 (Random123) and the two uniforms of a (row, column)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__device__ __forceinline__ void sample_uniforms(uint32_t k0, uint32_t k1, int64_t row, int64_t col, double& U0, double& U1) {
  uint32_t w[4];
  philox4x32_10((uint32_t)row, (uint32_t)col, 0u, 0u, k0, k1, w);
  U0 = (double)((((uint64_t)w[1] << 32) | w[0]) >> 11) * 0x1p-53;
  U1 = (double)((((uint64_t)w[3] << 32) | w[2]) >> 11) * 0x1p-53;
}

// ---- the rule of a (domain, loss) pair
enum { SA_IMPUTE = 0, SA_S1, SA_S2, SA_S3, SA_S4, SA_REFUSED };

__host__ __device__ __forceinline__ int sample_rule(int dkind, int lkind, int d) {
  if (d <= 1) {
    if (dkind == GLRM_DOMAIN_REAL && lkind == GLRM_LOSS_QUAD) return SA_S1;
    if (dkind == GLRM_DOMAIN_BOOL && lkind == GLRM_LOSS_LOGISTIC) return SA_S2;
    return SA_IMPUTE;
  }
  if (dkind == GLRM_DOMAIN_CATEGORICAL && lkind == GLRM_LOSS_MULTINOMIAL) return SA_S3;
  if (dkind == GLRM_DOMAIN_ORDINAL || dkind == GLRM_DOMAIN_CATEGORICAL) return SA_S4;
  if (dkind == GLRM_DOMAIN_BOOL) return SA_REFUSED;
  return SA_IMPUTE;
}

// levels the loss defines: 1 .. l.max
__device__ __forceinline__ int loss_levels(int lkind, int d) { return (lkind == GLRM_LOSS_BVS || lkind == GLRM_LOSS_MULTINOMIAL_ORDINAL) ? d + 1 : d; }

struct SampleBad {
  __device__ __forceinline__ bool operator()(const glrm_domain& D, const LossDesc& l, int d, const double* us, int stride) const {
    const int rule = sample_rule(D.kind, l.kind, d);
    if (rule == SA_REFUSED) return true;
    if (rule == SA_S4) return !(D.lo >= 1.0 && D.hi <= (double)loss_levels(l.kind, d) && D.lo <= D.hi);
    if (rule != SA_IMPUTE) return false;
    int bad = 0;
    (void)impute_value(D, l, d, us, stride, &bad);
    return bad != 0;
  }
};

// weight of level lev (1-based) under S3 / S4
__device__ __forceinline__ double level_weight(bool s3, const LossDesc& l, const double* us, int stride, int d, int lev) {
  return s3 ? fm_exp(us[(lev - 1) * stride]) : fm_exp(-vloss_eval_strided(l, us, stride, d, lev - 1));
}

struct SampleFin {
  uint32_t k0, k1;          // the key: seed & 0xffffffff, seed >> 32
  const double* sd;         // n values: sd_j of the Real x QuadLoss columns
  __device__ __forceinline__ void operator()(const IaArgs& a, int64_t e, int64_t row, int64_t col, int d, double* us, int stride) const {
    const LossDesc l = load_loss(a.losses, a.loss_single ? 0 : col);
    const glrm_domain D = a.domains[col];
    const int rule = sample_rule(D.kind, l.kind, d);
    double U0, U1;
    sample_uniforms(k0, k1, row, col, U0, U1);
    double r;
    if (rule == SA_S1) {
      const double z = sqrt(-2.0 * fm_log(1.0 - U0)) * cos(6.283185307179586 * U1);
      r = us[0] + z * sd[col];
    } else if (rule == SA_S2) {
      r = U0 <= 1.0 / (1.0 + fm_exp(-us[0])) ? 1.0 : 0.0;
    } else if (d > 1 && (rule == SA_S3 || rule == SA_S4)) {
      const bool s3 = rule == SA_S3;
      if (l.kind == GLRM_LOSS_MULTINOMIAL_ORDINAL) enforce_mnl_ord_rules_strided(us, stride, d); // evaluate() does (src/losses.jl:582)
      const int first = s3 ? 1 : (int)D.lo, last = s3 ? d : (int)D.hi;
      double sum = 0.0;
      for (int lev = first; lev <= last; ++lev) sum += level_weight(s3, l, us, stride, d, lev);
      const double t = U0 * sum;
      int lev = first;
      double cw = level_weight(s3, l, us, stride, d, lev);
      while (cw < t && lev < last) { ++lev; cw += level_weight(s3, l, us, stride, d, lev); }
      r = (double)lev;
    } else {
      int bad = 0; // decided per column before the launch (SampleBad)
      r = impute_value(D, l, d, us, stride, &bad);
    }
    a.out[e] = r;
  }
};

__global__ void __launch_bounds__(IA_THREADS, 2) sample_at_fast_kernel(const IaArgs a, const SampleFin fin) { ia_fast_body(a, fin); }
__global__ void __launch_bounds__(IA_GT) sample_at_general_kernel(const IaArgs a, const SampleFin fin) { ia_general_body(a, fin); }

// ---- v_j and sd_j: one workgroup per column
struct VarArgs {
  const double *X, *Y;
  int k, kp;
  int64_t n;
  const int64_t* ystart;
  const int64_t* cptr;      // the column view
  const int32_t* cidx;
  const double* cvals;
  const uint8_t* s1;        // n flags: the column is Real x QuadLoss
  int rule;                 // GLRM_SAMPLE_NOISE_RESIDUAL / _REFERENCE
  double* sd;               // n values out; NaN where s1 is 0
};

__global__ void __launch_bounds__(SA_VT) sa_variance_kernel(const VarArgs a) {
  __shared__ double part[SA_VT];
  const int64_t j = blockIdx.x;
  const int tid = threadIdx.x;
  if (!a.s1[j]) { // the whole workgroup
    if (tid == 0) a.sd[j] = __builtin_nan("");
    return;
  }
  const int64_t b = a.cptr[j], en = a.cptr[j + 1];
  const double* y = a.Y + a.ystart[j] * a.kp;
  double acc = 0.0;
  for (int64_t q = b + tid; q < en; q += SA_VT) {
    const double* x = a.X + (int64_t)a.cidx[q] * a.kp;
    double u = 0.0;
    for (int c = 0; c < a.k; ++c) u = fma(x[c], y[c], u);
    const double res = u - a.cvals[q];
    acc += res * res;
  }
  part[tid] = acc;
  __syncthreads();
  for (int s = SA_VT / 2; s > 0; s >>= 1) {
    if (tid < s) part[tid] += part[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    const double v = part[0] / (double)(en - b); // an empty column: 0 / 0
    a.sd[j] = a.rule == GLRM_SAMPLE_NOISE_RESIDUAL ? sqrt(v) : 1.0 / sqrt(v);
  }
}

// ---- keep_observed: the first occurrence of the entry's column in its row's row-view list
__global__ void __launch_bounds__(256) sa_keep_kernel(const IaArgs a, const int64_t* rptr, const int32_t* ridx, const double* rvals, uint8_t* kept) {
  const int tid = threadIdx.x, g = tid & (SA_KG - 1), grp = (tid & 63) / SA_KG;
  const int64_t e = (int64_t)blockIdx.x * (256 / SA_KG) + tid / SA_KG;
  if (e >= a.nb) return; // the whole group
  int64_t row, col;
  ia_decode(a, e, row, col);
  const int64_t b = rptr[row], en = rptr[row + 1];
  for (int64_t q = b; q < en; q += SA_KG) { // trip counts are uniform inside a group
    const bool hit = q + g < en && ridx[q + g] == (int32_t)col;
    const unsigned m = (unsigned)(__ballot(hit) >> (SA_KG * grp)) & 0xffffu;
    if (m) {
      const int first = __ffs(m) - 1;
      if (g == first) { a.out[e] = rvals[q + first]; kept[e] = 1; }
      return;
    }
  }
  if (g == 0) kept[e] = 0;
}

thread_local int64_t g_sa_blocks = 0, g_sa_fast = 0, g_sa_general = 0, g_sa_kept = 0, g_sa_varcols = 0;

} // namespace

extern "C" int glrm_hip_sample_at_info(int64_t* blocks, int64_t* entries_fast, int64_t* entries_general, int64_t* entries_kept, int64_t* variance_columns) {
  if (blocks) *blocks = g_sa_blocks;
  if (entries_fast) *entries_fast = g_sa_fast;
  if (entries_general) *entries_general = g_sa_general;
  if (entries_kept) *entries_kept = g_sa_kept;
  if (variance_columns) *variance_columns = g_sa_varcols;
  return GLRM_OK;
}

extern "C" int glrm_hip_sample_at(glrm_handle* h, const double* X, const double* Y, const glrm_domain* domains, const int64_t* rows, int64_t n_rows,
                                  const int32_t* cols, int64_t n_cols, int32_t mode, uint64_t seed, int32_t noise_rule, const double* noise_sd_in,
                                  int32_t keep_observed, int64_t block_entries, double* out, uint8_t* kept, double* noise_sd_out) {
  const char* const what = "glrm_hip_sample_at";
  int rc = xy_check_handle(h, what);
  if (rc) return rc;
  if ((rc = xy_check_factors(h, X, Y, what))) return rc;
  if ((rc = ia_check_shape(domains, rows, n_rows, cols, n_cols, mode, out, what))) return rc;
  if (noise_rule < GLRM_SAMPLE_NOISE_RESIDUAL || noise_rule > GLRM_SAMPLE_NOISE_GIVEN)
    return fail(GLRM_ERR_INVALID, "%s: noise_rule %d must be 0 (residual), 1 (reference) or 2 (given)", what, noise_rule);
  const bool given = noise_rule == GLRM_SAMPLE_NOISE_GIVEN;
  if (given && !noise_sd_in) return fail(GLRM_ERR_INVALID, "%s: noise_rule 2 (given) needs noise_sd_in", what);
  if (!given && noise_sd_in) return fail(GLRM_ERR_INVALID, "%s: noise_sd_in is read under noise_rule 2 (given) only, not under %d", what, noise_rule);
  if (keep_observed != 0 && keep_observed != 1) return fail(GLRM_ERR_INVALID, "%s: keep_observed %d must be 0 or 1", what, keep_observed);
  if (kept && !keep_observed) return fail(GLRM_ERR_INVALID, "%s: kept needs keep_observed = 1", what);
  const glrm_handle::Side& rv = h->side[GLRM_ROWS];
  const glrm_handle::Side& cv = h->side[GLRM_COLS];
  if (keep_observed && (!rv.ptr || !rv.idx || !rv.vals)) return fail(GLRM_ERR_INVALID, "%s: keep_observed = 1 needs the handle's row view", what);
  int64_t total = 0;
  if ((rc = ia_check_indices(h, domains, rows, n_rows, cols, n_cols, mode, block_entries, what, &total))) return rc;
  const int64_t n = h->n;

  // the Real x QuadLoss columns, and whether a queried entry lies in one
  std::vector<uint8_t> s1((size_t)n);
  int64_t n_s1 = 0;
  for (int64_t j = 0; j < n; ++j) {
    const glrm_loss& l = h->losses_h[h->n_losses == 1 ? 0 : (size_t)j];
    s1[(size_t)j] = sample_rule(domains[j].kind, l.kind, l.dim) == SA_S1 ? 1 : 0;
    n_s1 += s1[(size_t)j];
  }
  bool s1_queried = false;
  if (n_s1 > 0 && total > 0) {
    if (mode == GLRM_IMPUTE_AT_ROWS) s1_queried = true;
    else for (int64_t c = 0; c < n_cols && !s1_queried; ++c) s1_queried = s1[(size_t)cols[c]] != 0;
  }
  const bool variance = !given && n_s1 > 0 && (s1_queried || noise_sd_out);
  if (variance && (!cv.ptr || !cv.idx || !cv.vals)) return fail(GLRM_ERR_INVALID, "%s: noise_rule %d needs the handle's column view", what, noise_rule);
  if (total == 0 && !variance) {
    if (noise_sd_out) for (int64_t j = 0; j < n; ++j) noise_sd_out[j] = s1[(size_t)j] && given ? noise_sd_in[j] : __builtin_nan("");
    g_sa_blocks = g_sa_fast = g_sa_general = g_sa_kept = g_sa_varcols = 0;
    return GLRM_OK;
  }

  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  hipStream_t st = h->stream;

  DevArena w;
  IaArgs a{};
  // the queried columns must have an answer
  {
    std::vector<uint8_t> bad_h;
    int64_t badcol = -1;
    if ((rc = ia_columns(h, w, a, domains, cols, n_cols, mode, n_rows, SampleBad{}, bad_h, &badcol))) return rc;
    if (badcol >= 0)
      return fail(GLRM_ERR_UNSUPPORTED, "%s: column %lld is queried and its (domain, loss) pair cannot be sampled: no imputation rule in the reference "
                  "(src/impute_and_err.jl), Bool with a multi-dimensional loss, or levels outside those the loss defines", what, (long long)badcol);
  }

  TkFactors f{};
  if ((rc = tk_factors(h, X, Y, f))) return rc;
  a.X = f.X; a.Y = f.Y;

  // sd_j on the device: given, or from the variance pass (NaN bytes where nothing reads)
  double* d_sd = nullptr;
  if ((rc = w.alloc(&d_sd, (size_t)n))) return rc;
  std::vector<double> sd_h;
  if (given) {
    sd_h.resize((size_t)n);
    for (int64_t j = 0; j < n; ++j) sd_h[(size_t)j] = s1[(size_t)j] ? noise_sd_in[j] : __builtin_nan("");
    HIPCK(hipMemcpyAsync(d_sd, sd_h.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
  } else if (variance) {
    uint8_t* d_s1 = nullptr;
    if ((rc = w.alloc(&d_s1, (size_t)n))) return rc;
    HIPCK(hipMemcpyAsync(d_s1, s1.data(), (size_t)n, hipMemcpyHostToDevice, st));
    VarArgs v{};
    v.X = a.X; v.Y = a.Y; v.k = a.k; v.kp = a.kp; v.n = n; v.ystart = a.ystart;
    v.cptr = cv.ptr; v.cidx = cv.idx; v.cvals = cv.vals; v.s1 = d_s1; v.rule = noise_rule; v.sd = d_sd;
    hipLaunchKernelGGL(sa_variance_kernel, dim3((unsigned)n), dim3(SA_VT), 0, st, v);
    HIPCK(hipGetLastError());
    if (noise_sd_out) {
      sd_h.resize((size_t)n);
      HIPCK(hipMemcpyAsync(sd_h.data(), d_sd, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    }
  } else {
    HIPCK(hipMemsetAsync(d_sd, 0xFF, (size_t)n * 8, st));
    if (noise_sd_out) sd_h.assign((size_t)n, __builtin_nan(""));
  }
  HIPCK(hipStreamSynchronize(st)); // the uploads' host buffers, and sd_h
  if (noise_sd_out) std::copy(sd_h.begin(), sd_h.end(), noise_sd_out);
  g_sa_varcols = variance ? n_s1 : 0;
  if (total == 0) {
    g_sa_blocks = g_sa_fast = g_sa_general = g_sa_kept = 0;
    return GLRM_OK;
  }

  // this unit's scratch: a kept flag per entry
  IaBlocks b;
  if ((rc = ia_blocks_alloc(h, w, a, rows, n_rows, cols, n_cols, mode, total, block_entries, (size_t)n * 9, keep_observed ? 1 : 0, what, b))) return rc;
  uint8_t* d_kept = nullptr;
  std::vector<uint8_t> kept_h;
  if (keep_observed) {
    if ((rc = w.alloc(&d_kept, (size_t)b.block))) return rc;
    if (!kept) kept_h.resize((size_t)b.block);
  }
  const SampleFin fin{(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), d_sd};

  int64_t nblocks = 0, n_fast = 0, n_kept = 0;
  for (int64_t t0 = 0; t0 < total; t0 += b.block, ++nblocks) {
    const int64_t nb = std::min(b.block, total - t0);
    if ((rc = ia_block_begin(st, a, b, rows, cols, t0, nb))) return rc;
    ia_block_launch(h, a, b, fin, sample_at_fast_kernel, sample_at_general_kernel);
    if (keep_observed)
      hipLaunchKernelGGL(sa_keep_kernel, dim3((unsigned)((nb + 256 / SA_KG - 1) / (256 / SA_KG))), dim3(256), 0, st, a, (const int64_t*)rv.ptr,
                         (const int32_t*)rv.idx, (const double*)rv.vals, d_kept);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(out + t0, b.d_out, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
    uint8_t* kdst = keep_observed ? (kept ? kept + t0 : kept_h.data()) : nullptr;
    if (kdst) HIPCK(hipMemcpyAsync(kdst, d_kept, (size_t)nb, hipMemcpyDeviceToHost, st));
    int64_t nf = nb;
    if (b.multi) HIPCK(hipMemcpyAsync(&nf, b.d_nfast, 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    n_fast += nf;
    if (kdst) for (int64_t t = 0; t < nb; ++t) n_kept += kdst[t];
  }
  g_sa_blocks = nblocks; g_sa_fast = n_fast; g_sa_general = total - n_fast; g_sa_kept = n_kept;
  return GLRM_OK;
}
