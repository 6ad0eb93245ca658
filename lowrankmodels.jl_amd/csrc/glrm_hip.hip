// glrm_hip.hip -- libglrm_hip.so: the MI355X (gfx950 / CDNA4) engine behind
// LowRankModels.jl's fit!(glrm, ProxGradParams) (src/algorithms/proxgrad.jl:34-220).
//
// One HIP kernel per factor half-step ("sweep"):
//   X half-step = row sweep over CSR-by-row   (proxgrad.jl:118-156 + evaluate_fit.jl:24-38)
//   Y half-step = column sweep over CSC-by-col (proxgrad.jl:162-201 + evaluate_fit.jl:39-55)
// Both are the same kernel template: a *segment* (row or column) is owned by WAVES wavefronts;
// every observation of the segment is handled by a group of G lanes that reads the opposing
// factor's k-vector with one 16-byte load per lane (16*G contiguous bytes per group), reduces
// the dot product with DPP adds, evaluates loss and gradient, and accumulates the gradient in
// registers.  Gradient pass, backtracking line search (one more pass over the segment per trial)
// and the prox step are fused in the kernel; the accept/reject decision is wave/block uniform.
// Reduction order is fixed by the code => results are run-to-run deterministic and independent of
// how rows/columns are sharded over GPUs.
//
// No CPU fallback lives here; the CPU restatement (oracle/) is a separate, test-only library.

#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "glrm_device.hpp"
#include "glrm_engine.hpp"
#include "glrm_launch.hpp"
#include "glrm_sweep.hpp" // the gather sweeps and the penalty kernel: this unit instantiates them for double storage

using namespace glrm;

// =============================================================================== kernels

// Fixed-shape two-stage sum: 256 blocks x 256 threads, strided partials, LDS tree, then one block.
// The shape never depends on the shard layout, so the recorded objective is G-invariant.
constexpr int SUM_BLOCKS = 256, SUM_THREADS = 256;

__device__ __forceinline__ double block_tree_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = SUM_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

__global__ void __launch_bounds__(SUM_THREADS) sum_stage1(const double* v, int64_t n, double* partials) {
  __shared__ double sh[SUM_THREADS];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * SUM_THREADS + threadIdx.x; i < n; i += (int64_t)SUM_BLOCKS * SUM_THREADS) acc += v[i];
  const double t = block_tree_sum(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ void __launch_bounds__(SUM_THREADS) sum_stage2(const double* partials, double* out) {
  __shared__ double sh[SUM_THREADS];
  const double t = block_tree_sum(partials[threadIdx.x], sh);
  if (threadIdx.x == 0) *out = t;
}

__global__ void fill_kernel(double* p, int64_t n, double v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ void isum_kernel(const int32_t* v, int64_t n, unsigned long long* out) {
  unsigned long long acc = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) acc += (unsigned long long)v[i];
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

// Per-view statistics for glrm_signature and the class plan of the gather sweeps: out[0] = longest list, out[1..3] = segments per wave
// class (forced_cls > 0 pins the class), out[4] = segments the cached sweep takes (len <= cache_maxlen; cache_maxlen < 0: none; they are
// not counted in out[1..3]), out[5] = longest of those.
__global__ void seg_stats_kernel(const int64_t* ptr, int64_t nseg, int forced_cls, int64_t cache_maxlen, unsigned long long* out) {
  unsigned long long mx = 0, c1 = 0, c2 = 0, c3 = 0, cc = 0, mc = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t len = ptr[s + 1] - ptr[s];
    mx = (unsigned long long)len > mx ? (unsigned long long)len : mx;
    const int cls = glrm_segment_class(len, cache_maxlen, forced_cls);
    if (cls == 0) {
      ++cc;
      mc = (unsigned long long)len > mc ? (unsigned long long)len : mc;
    } else {
      c1 += cls == 1; c2 += cls == 2; c3 += cls == 3;
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o0 = __shfl_xor(mx, d, 64), o5 = __shfl_xor(mc, d, 64);
    mx = o0 > mx ? o0 : mx; mc = o5 > mc ? o5 : mc;
    c1 += __shfl_xor(c1, d, 64); c2 += __shfl_xor(c2, d, 64); c3 += __shfl_xor(c3, d, 64); cc += __shfl_xor(cc, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(out + 0, mx); atomicMax(out + 5, mc);
    if (c1) atomicAdd(out + 1, c1);
    if (c2) atomicAdd(out + 2, c2);
    if (c3) atomicAdd(out + 3, c3);
    if (cc) atomicAdd(out + 4, cc);
  }
}

// =============================================================================== host side

thread_local char g_err[768];

extern "C" int glrm_hip_version(void) { return GLRM_HIP_ABI_VERSION; }
extern "C" const char* glrm_hip_last_error(void) { return g_err; }

// kp = G*R >= k: lanes per observation G and components per lane R
static int pick_layout(int k, int& G, int& R) {
  int kp;
  if (k <= 8) { kp = 8; G = 4; }
  else if (k <= 16) { kp = 16; G = 4; }
  else if (k <= 32) { kp = 32; G = 4; }
  else if (k <= 64) { kp = 64; G = 8; }
  else if (k <= 128) { kp = 128; G = 16; }
  else return -1;
  R = kp / G;
  return 0;
}

template <typename T>
static int dev_copy_in(glrm_handle* h, T** dst, const T* src, int64_t count, bool src_on_device, hipStream_t st) {
  if (const int rc = h->mem.alloc(dst, (size_t)std::max<int64_t>(0, count))) return rc;
  if (count > 0)
    HIPCK(hipMemcpyAsync(*dst, src, (size_t)count * sizeof(T), src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  return GLRM_OK;
}

static bool is_classification(int kind) { return kind == GLRM_LOSS_LOGISTIC || kind == GLRM_LOSS_WEIGHTED_HINGE; }

// Host-array validation: the checks of the GLRM constructor (src/glrm.jl:38-43,63-71) and of the
// Bool coercion (src/losses.jl:104-106), plus structural checks of the CSR / CSC arrays.
static int check_view(const char* name, int64_t nseg, const int64_t* ptr, const int32_t* idx, const double* vals,
                      int64_t bound, const glrm_problem* p, bool by_idx, int64_t seg_offset) {
  if (!ptr) return fail(GLRM_ERR_INVALID, "%s pointer array is NULL", name);
  if (int rc = glrm_check_offsets(name, ptr, nseg)) return rc;
  if (ptr[nseg] > 0 && (!idx || !vals)) return fail(GLRM_ERR_INVALID, "%s index/value arrays are NULL", name);
  for (int64_t s = 0; s < nseg; ++s) {
    for (int64_t t = ptr[s]; t < ptr[s + 1]; ++t) {
      if (idx[t] < 0 || idx[t] >= bound)
        return fail(GLRM_ERR_INVALID, "%s: index %d out of range [0,%lld)", name, idx[t], (long long)bound);
      const int64_t e = by_idx ? seg_offset + s : idx[t], f = by_idx ? idx[t] : seg_offset + s;
      if (std::isnan(vals[t]))
        return fail(GLRM_ERR_NONFINITE, "Observed value in entry (%lld, %lld) is NaN.", (long long)e, (long long)f);
      const glrm_loss& l = p->n_losses == 1 ? p->losses[0] : p->losses[f];
      if (is_classification(l.kind) && !(vals[t] == 1.0 || vals[t] == 0.0))
        return fail(GLRM_ERR_NONFINITE, "entry in column %lld has label %g; a ClassificationLoss needs true(1)/false(0)",
                    (long long)f, vals[t]);
      if (l.kind >= GLRM_LOSS_MULTINOMIAL) { // levels 1..max index into u (BoundsError / InexactError in the reference)
        const int mx = (l.kind == GLRM_LOSS_BVS || l.kind == GLRM_LOSS_MULTINOMIAL_ORDINAL) ? l.dim + 1 : l.dim;
        if (!(vals[t] >= 1.0 && vals[t] <= (double)mx && vals[t] == std::floor(vals[t])))
          return fail(GLRM_ERR_NONFINITE, "entry (%lld, %lld) = %g is not a level in 1..%d of its categorical / ordinal loss",
                      (long long)e, (long long)f, vals[t], mx);
      }
    }
  }
  return GLRM_OK;
}

static bool wrap_ok(int w) {
  return w == 0 || w == GLRM_WRAP_LASTENTRY1 || w == GLRM_WRAP_LASTENTRY_UNPENALIZED || w == GLRM_WRAP_ORDINAL || w == GLRM_WRAP_MNL_ORDINAL;
}

static const char* reg_kind_name(int kind) {
  static const char* const names[GLRM_REG_KIND_END] = {"ZeroReg", "QuadReg", "OneReg", "NonNegConstraint", "UnitOneSparseConstraint",
                                                      "QuadConstraint", "NonNegOneReg", "OneSparseConstraint", "KSparseConstraint", "SimplexConstraint"};
  return kind >= 0 && kind < GLRM_REG_KIND_END ? names[kind] : "?";
}

// One side's regularizer descriptors (create and set_regularizers).  losses != NULL: the side is ry, descriptor i belongs to column
// col_begin + i (one descriptor: to all ncols local columns).  The kinds >= GLRM_REG_QUAD_CONSTRAINT are VECTOR regularizers: the reference's
// sort / partialsortperm / norm act on a vector, so the block of a multi-dimensional column and the base of OrdinalReg / MNLOrdinalReg are
// refused; KSparseConstraint(r) with r outside 1 .. length is the reference's BoundsError inside the fit, refused here.
static int check_regs(const char* side, const glrm_reg* r, int64_t cnt, int k, const glrm_loss* losses, int64_t n_losses, int64_t col_begin,
                      int64_t ncols) {
  for (int64_t i = 0; i < cnt; ++i) {
    const int kind = r[i].kind, wrap = r[i].wrap;
    if (kind < 0 || kind >= GLRM_REG_KIND_END) return fail(GLRM_ERR_UNSUPPORTED, "%s regularizer kind %d is not supported", side, kind);
    if (!wrap_ok(wrap)) return fail(GLRM_ERR_INVALID, "glrm_reg.wrap must be 0 or one GLRM_WRAP_* flag");
    if (kind < GLRM_REG_QUAD_CONSTRAINT) continue;
    if (wrap & (GLRM_WRAP_ORDINAL | GLRM_WRAP_MNL_ORDINAL))
      return fail(GLRM_ERR_UNSUPPORTED, "%s[%lld]: %s is a vector regularizer and cannot be the base of OrdinalReg / MNLOrdinalReg", side,
                  (long long)i, reg_kind_name(kind));
    if (losses) {
      const int64_t f0 = cnt == 1 ? col_begin : col_begin + i, f1 = cnt == 1 ? col_begin + ncols : f0 + 1;
      for (int64_t f = f0; f < f1; ++f) {
        const glrm_loss& l = n_losses == 1 ? losses[0] : losses[f];
        if (l.dim > 1)
          return fail(GLRM_ERR_UNSUPPORTED, "%s: %s is a vector regularizer and cannot regularize the %d-column block of column %lld", side,
                      reg_kind_name(kind), l.dim, (long long)f);
        if (n_losses == 1) break;
      }
    }
    const int len = wrap ? k - 1 : k; // what the base regularizer sees
    if (kind == GLRM_REG_K_SPARSE && !(r[i].scale >= 1.0 && r[i].scale <= (double)len && r[i].scale == std::floor(r[i].scale)))
      return fail(GLRM_ERR_INVALID, "%s[%lld]: KSparseConstraint keeps r = %g entries; r must be an integer in 1..%d", side, (long long)i,
                  r[i].scale, len);
    if (kind == GLRM_REG_QUAD_CONSTRAINT && !(r[i].scale > 0.0 && std::isfinite(r[i].scale)))
      return fail(GLRM_ERR_INVALID, "%s[%lld]: QuadConstraint needs a finite max_2norm > 0 (got %g)", side, (long long)i, r[i].scale);
  }
  return GLRM_OK;
}

static bool any_vector_reg(const std::vector<glrm_reg>& r) {
  for (const glrm_reg& x : r)
    if (x.kind >= GLRM_REG_QUAD_CONSTRAINT) return true;
  return false;
}

static int check_desc(const glrm_problem* p) {
  const int64_t ml = p->row_end - p->row_begin, nl = p->col_end - p->col_begin;
  if (!p->losses || !(p->n_losses == 1 || p->n_losses == p->n))
    return fail(GLRM_ERR_INVALID, "There must be as many losses as there are columns in the data matrix (n_losses=%lld, n=%lld)",
                (long long)p->n_losses, (long long)p->n);
  if (!p->rx || !(p->n_rx == 1 || p->n_rx == ml))
    return fail(GLRM_ERR_INVALID, "There must be either one X regularizer or as many X regularizers as there are rows in the data matrix");
  if (!p->ry || !(p->n_ry == 1 || p->n_ry == nl))
    return fail(GLRM_ERR_INVALID, "There must be either one Y regularizer or as many Y regularizers as there are columns in the data matrix");
  for (int64_t i = 0; i < p->n_losses; ++i) {
    if (p->losses[i].kind < 0 || p->losses[i].kind >= GLRM_LOSS_KIND_COUNT)
      return fail(GLRM_ERR_UNSUPPORTED, "loss kind %d (column %lld) is not a supported loss", p->losses[i].kind, (long long)i);
    if (p->losses[i].kind < GLRM_LOSS_MULTINOMIAL ? !(p->losses[i].dim == 0 || p->losses[i].dim == 1)
                                                  : !(p->losses[i].dim >= 2 && p->losses[i].dim <= GLRM_MAX_EMBEDDING_DIM))
      return fail(GLRM_ERR_INVALID, "glrm_loss.dim = %d is not a valid embedding dimension for loss kind %d", p->losses[i].dim, p->losses[i].kind);
    if ((p->losses[i].kind == GLRM_LOSS_OVA || p->losses[i].kind == GLRM_LOSS_BVS) &&
        !(p->losses[i].p1 == GLRM_LOSS_LOGISTIC || p->losses[i].p1 == GLRM_LOSS_WEIGHTED_HINGE))
      return fail(GLRM_ERR_UNSUPPORTED, "bin_loss of OvALoss / BvSLoss must be LogisticLoss or HingeLoss");
  }
  if (const int rc = check_regs("rx", p->rx, p->n_rx, p->k, nullptr, 0, 0, 0)) return rc;
  if (const int rc = check_regs("ry", p->ry, p->n_ry, p->k, p->losses, p->n_losses, p->col_begin, nl)) return rc;
  return GLRM_OK;
}

extern "C" void glrm_hip_destroy(glrm_handle* h) {
  if (!h) return;
  DeviceScope dg(h->device);
  (void)hipStreamSynchronize(h->stream);
  h->mem.free_all(); // every device allocation of the handle; what follows is not device memory
  if (h->iter_exec) (void)hipGraphExecDestroy(h->iter_exec);
  if (h->iter_graph) (void)hipGraphDestroy(h->iter_graph);
  if (h->pinned_obj) (void)hipHostFree(h->pinned_obj);
  for (auto& e : h->pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto& e : h->pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

// ------------------------------------------------------------------ host helpers shared by the families (glrm_engine.hpp)

// the line-search counters of both sides back to zero (create, glrm_hip_kernel_stats with reset)
static int zero_counters(glrm_handle* h) {
  for (glrm_handle::Side& v : h->side) {
    const size_t bytes = (size_t)(v.nseg > 0 ? v.nseg : 1) * 4;
    HIPCK(hipMemsetAsync(v.trials, 0, bytes, h->stream));
    HIPCK(hipMemsetAsync(v.accepts, 0, bytes, h->stream));
  }
  return GLRM_OK;
}

int glrm_alloc_pass_buffers(glrm_handle* h, int side) {
  glrm_handle::PassBuffers& b = h->side[side].pass;
  const size_t nseg1 = (size_t)std::max<int64_t>(1, h->side[side].nseg);
  int rc;
  if ((rc = h->mem.alloc(&b.part, nseg1 * b.nsup * (h->kp + 2)))) return rc;
  if ((rc = h->mem.alloc(&b.gsum, nseg1 * h->kp))) return rc;
  if ((rc = h->mem.alloc(&b.trial, nseg1 * h->kp))) return rc;
  if ((rc = h->mem.alloc(&b.jold, nseg1))) return rc;
  if ((rc = h->mem.alloc(&b.active, nseg1))) return rc;
  if ((rc = h->mem.alloc(&b.ntrial, nseg1))) return rc;
  return h->nactive ? GLRM_OK : h->mem.alloc(&h->nactive, 1);
}

int glrm_ensure_side_stream(glrm_handle* h) {
  if (h->side_stream) return GLRM_OK;
  HIPCK(hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
  HIPCK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
  HIPCK(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
  return GLRM_OK;
}

int glrm_fork_side_stream(glrm_handle* h) {
  HIPCK(hipEventRecord(h->ev_fork, h->stream));
  HIPCK(hipStreamWaitEvent(h->side_stream, h->ev_fork, 0));
  return GLRM_OK;
}

hipError_t glrm_join_side_stream(glrm_handle* h) {
  char keep[sizeof g_err];
  memcpy(keep, g_err, sizeof keep);
  const hipError_t e_rec = hipEventRecord(h->ev_join, h->side_stream);
  const hipError_t e_wait = hipStreamWaitEvent(h->stream, h->ev_join, 0);
  memcpy(g_err, keep, sizeof keep);
  return e_rec != hipSuccess ? e_rec : e_wait;
}

int glrm_host_ptr(glrm_handle* h, int side, std::vector<int64_t>& ptr) {
  const size_t nseg = (size_t)h->side[side].nseg;
  ptr.resize(nseg + 1);
  HIPCK(hipMemcpyAsync(ptr.data(), h->side[side].ptr, (nseg + 1) * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  return GLRM_OK;
}

int glrm_upload_list(glrm_handle* h, const std::vector<int32_t>& list, int32_t** out) {
  if (const int rc = h->mem.alloc(out, list.size())) return rc;
  HIPCK(hipMemcpyAsync(*out, list.data(), list.size() * 4, hipMemcpyHostToDevice, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  return GLRM_OK;
}

void glrm_split_by_length(const std::vector<int64_t>& ptr, int64_t long_from, std::vector<int32_t>& shorts, std::vector<int32_t>& longs) {
  const int64_t nseg = (int64_t)ptr.size() - 1;
  shorts.reserve((size_t)nseg);
  for (int64_t s = 0; s < nseg; ++s) (long_from > 0 && ptr[s + 1] - ptr[s] >= long_from ? longs : shorts).push_back((int32_t)s);
  std::stable_sort(shorts.begin(), shorts.end(), [&](int32_t x, int32_t y) { return ptr[x + 1] - ptr[x] > ptr[y + 1] - ptr[y]; });
}

int glrm_set_long_columns(glrm_handle* h, const std::vector<int32_t>& longs) {
  h->blk_nlong_c = (int64_t)longs.size();
  if (longs.empty()) return GLRM_OK;
  const int rc = glrm_upload_list(h, longs, &h->blk_long_c);
  return rc ? rc : glrm_ensure_side_stream(h);
}

static int view_stats(glrm_handle* h, int side, int forced_cls, int64_t cache_maxlen, unsigned long long (&st)[6]) {
  for (auto& v : st) v = 0;
  const int64_t nseg = h->side[side].nseg;
  if (nseg <= 0) return GLRM_OK;
  DevArena scratch;
  unsigned long long* d = nullptr;
  if (const int rc = scratch.alloc(&d, 6)) return rc;
  hipError_t e = hipMemsetAsync(d, 0, sizeof st, h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(seg_stats_kernel, dim3(1024), dim3(256), 0, h->stream, h->side[side].ptr, nseg, forced_cls, cache_maxlen, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(st, d, sizeof st, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(GLRM_ERR_HIP, "segment statistics failed: %s", hipGetErrorString(e));
  return GLRM_OK;
}

// The class plan of a view that runs on the gather sweeps (and, for rows, a cached kernel: cached_maxlen >= 0, `variant` names the cap
// formula): every segment is swept by the number of waves its OWN length asks for (glrm_segment_class; glrm_options.waves_* pins one
// count), rows short enough for the cached kernel by that one -- so a segment is summed in the same order whichever shard holds it.  One
// populated class: one launch over all local segments, no list.  Several (skewed lengths: a few very popular columns / very active rows
// next to many short ones): the segments class by class, one launch per class (glrm_for_each_class).  Writes the plan and, for a list,
// creates the side stream: nothing else of the handle.
static int build_class_plan(glrm_handle* h, int side, int64_t cached_maxlen, int variant, glrm_class_plan* plan) {
  const glrm_handle::Side& v = h->side[side];
  const int forced = glrm_forced_class(h, side);
  unsigned long long st[6];
  int rc = view_stats(h, side, forced, cached_maxlen, st);
  if (rc) return rc;
  int64_t* n = plan->n;
  n[0] = (int64_t)st[4]; n[1] = (int64_t)st[1]; n[2] = (int64_t)st[2]; n[3] = (int64_t)st[3];
  plan->cap = n[0] > 0 ? glrm_cached_cap(variant, h->G, h->kp, (int64_t)st[5]) : 0;
  int populated = 0;
  for (int c = 0; c < 4; ++c) populated += n[c] > 0;
  if (populated > 1) {
    std::vector<int64_t> ptr;
    if ((rc = glrm_host_ptr(h, side, ptr))) return rc;
    std::vector<int32_t> lst((size_t)v.nseg);
    int64_t pos[4] = {0, n[0], n[0] + n[1], n[0] + n[1] + n[2]};
    for (int64_t s = 0; s < v.nseg; ++s) lst[(size_t)pos[glrm_segment_class(ptr[s + 1] - ptr[s], cached_maxlen, forced)]++] = (int32_t)s;
    if ((rc = glrm_upload_list(h, lst, &plan->list))) return rc;
    if ((rc = glrm_ensure_side_stream(h))) return rc;
  }
  plan->built = true;
  return GLRM_OK;
}

// finalize: the plans of the sides the gather family runs, and what they say about the handle -- no row for the cached sweep on this shard:
// cached_row falls to 0; Side::waves: the pinned count, else that of the fullest class by length (ties: the lower)
static int plan_gather_sides(glrm_handle* h) {
  for (int s = 0; s < 2; ++s) {
    glrm_handle::Side& v = h->side[s];
    if (v.tiled || v.blocked) continue;
    const bool cached = s == GLRM_ROWS && h->cached_row != 0; // only rows have a cached sweep
    if (const int rc = build_class_plan(h, s, cached ? h->cached_maxlen : -1, h->cached_row, &v.plan)) return rc;
    if (cached && v.plan.n[0] == 0) h->cached_row = 0;
    const int forced = glrm_forced_class(h, s);
    int best = 1;
    for (int c = 2; c < 4; ++c) if (v.plan.n[c] > v.plan.n[best]) best = c;
    v.waves = glrm_class_waves(forced ? forced : best);
  }
  return GLRM_OK;
}

static int create_impl(glrm_handle* h, const glrm_problem* p, const glrm_options* o) {
  const bool on_dev = (p->flags & GLRM_PROBLEM_DEVICE_ARRAYS) != 0;
  h->m = p->m; h->n = p->n; h->k = p->k;
  glrm_handle::Side &rows = h->side[GLRM_ROWS], &cols = h->side[GLRM_COLS];
  rows.begin = p->row_begin; rows.end = p->row_end; rows.nglob = p->m;
  cols.begin = p->col_begin; cols.end = p->col_end; cols.nglob = p->n;
  for (glrm_handle::Side& v : h->side) v.nseg = v.end - v.begin;
  pick_layout(p->k, h->G, h->R);
  h->kp = h->G * h->R;
  h->profile = o ? o->profile : 0;
  h->tiled_opt = o ? o->tiled : 0;
  h->sum_order_opt = o ? o->sum_order : 0;
  if (o && o->reserved != 0) return fail(GLRM_ERR_INVALID, "glrm_options.reserved must be 0");
  h->storage = o ? o->storage : GLRM_STORAGE_F64; // range and refusals: glrm_check_storage, before the handle existed
  if (o && (o->sum_order < 0 || o->sum_order > 1)) return fail(GLRM_ERR_INVALID, "glrm_options.sum_order must be 0 (engine orders) or 1 (reference order)");
  if (o) h->opts = *o; else { h->opts = glrm_options{}; h->opts.device_id = -1; }
  h->losses_h.assign(p->losses, p->losses + p->n_losses);
  rows.regs_h.assign(p->rx, p->rx + p->n_rx);
  cols.regs_h.assign(p->ry, p->ry + p->n_ry);
  for (glrm_handle::Side& v : h->side) v.vecreg = any_vector_reg(v.regs_h);
  if (o && (o->stream || o->caller_stream)) {
    h->stream = (hipStream_t)o->stream; // may be NULL = the legacy default stream (caller_stream)
  } else {
    HIPCK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
  }
  hipStream_t st = h->stream;
  int rc;
  // (a float handle narrows the values into arrays of its own: it copies what it may borrow)
  const bool borrow = on_dev && (p->flags & GLRM_PROBLEM_BORROW_DEVICE_ARRAYS) != 0 && h->storage == GLRM_STORAGE_F64;
  const struct { const int64_t* ptr; const int32_t* idx; const double* vals; } pv[2] = {{p->rowptr, p->colidx, p->rowvals}, {p->colptr, p->rowidx, p->colvals}};
  if (!p->dense_A && borrow) { // the caller's device arrays, read in place
    for (int s = 0; s < 2; ++s) {
      glrm_handle::Side& v = h->side[s];
      v.ptr = const_cast<int64_t*>(pv[s].ptr); v.idx = const_cast<int32_t*>(pv[s].idx); v.vals = const_cast<double*>(pv[s].vals);
      HIPCK(hipMemcpyAsync(&v.nnz, v.ptr + v.nseg, 8, hipMemcpyDeviceToHost, st));
    }
    HIPCK(hipStreamSynchronize(st));
    if ((rows.nnz > 0 && (!rows.idx || !rows.vals)) || (cols.nnz > 0 && (!cols.idx || !cols.vals)))
      return fail(GLRM_ERR_INVALID, "index / value arrays are NULL");
  } else if (!p->dense_A) {
    // GLRM_PROBLEM_ROWS_FROM_COLS: the column view only; the row view is derived on the device
    const bool from_cols = (p->flags & GLRM_PROBLEM_ROWS_FROM_COLS) != 0;
    const int first = from_cols ? GLRM_COLS : GLRM_ROWS;
    for (int s = first; s < 2; ++s)
      if ((rc = dev_copy_in(h, &h->side[s].ptr, pv[s].ptr, h->side[s].nseg + 1, on_dev, st))) return rc;
    for (int s = first; s < 2; ++s) {
      if (on_dev) HIPCK(hipMemcpyAsync(&h->side[s].nnz, pv[s].ptr + h->side[s].nseg, 8, hipMemcpyDeviceToHost, st));
      else h->side[s].nnz = pv[s].ptr[h->side[s].nseg];
    }
    if (on_dev) HIPCK(hipStreamSynchronize(st));
    if (from_cols && cols.nnz > 0 && (!p->rowidx || !p->colvals)) return fail(GLRM_ERR_INVALID, "index / value arrays are NULL");
    for (int s = first; s < 2; ++s) {
      if ((rc = dev_copy_in(h, &h->side[s].idx, pv[s].idx, h->side[s].nnz, on_dev, st))) return rc;
      if ((rc = dev_copy_in(h, &h->side[s].vals, pv[s].vals, h->side[s].nnz, on_dev, st))) return rc;
    }
    if (from_cols && (rc = glrm_rows_from_cols(h))) return rc;
  }
  h->n_losses = p->n_losses; rows.n_regs = p->n_rx; cols.n_regs = p->n_ry;
  if ((rc = dev_copy_in(h, &h->losses, p->losses, p->n_losses, false, st))) return rc;
  if ((rc = dev_copy_in(h, &rows.regs, p->rx, p->n_rx, false, st))) return rc;
  if ((rc = dev_copy_in(h, &cols.regs, p->ry, p->n_ry, false, st))) return rc;
  h->loss_quad_uniform = p->n_losses == 1 && p->losses[0].kind == GLRM_LOSS_QUAD;
  h->has_trig = false;
  for (int64_t i = 0; i < p->n_losses; ++i) h->has_trig = h->has_trig || p->losses[i].kind == GLRM_LOSS_PERIODIC;
  if ((rc = h->mem.alloc(&h->partials, SUM_BLOCKS))) return rc;
  if ((rc = h->mem.alloc(&h->dscalar, 1))) return rc;
  if ((rc = h->mem.alloc(&h->dcount, 1))) return rc;
  for (glrm_handle::Side& v : h->side) {
    const int64_t nseg1 = v.nseg > 0 ? v.nseg : 1;
    if ((rc = h->mem.alloc(&v.alpha, nseg1))) return rc;
    if ((rc = h->mem.alloc(&v.trials, nseg1))) return rc;
    if ((rc = h->mem.alloc(&v.accepts, nseg1))) return rc;
  }
  if ((rc = zero_counters(h))) return rc;
  int rc2 = glrm_setup_multi(h, p);
  if (rc2) return rc2;
  // this shard's contribution to the signature of the whole problem (include/glrm_hip.h: glrm_signature)
  h->sig_local = glrm_signature{};
  if (p->dense_A) {
    h->sig_local.nnz_rows = rows.nseg * h->n; h->sig_local.nnz_cols = cols.nseg * h->m;
    h->sig_local.max_row_len = rows.nseg > 0 ? h->n : 0; h->sig_local.max_col_len = cols.nseg > 0 ? h->m : 0;
    if ((rc2 = glrm_setup_dense(h, p))) return rc2;
  } else {
    int64_t* const max_len[2] = {&h->sig_local.max_row_len, &h->sig_local.max_col_len};
    for (int s = 0; s < 2; ++s) {
      unsigned long long st6[6];
      if ((rc = view_stats(h, s, 0, -1, st6))) return rc;
      *max_len[s] = (int64_t)st6[0];
    }
    h->sig_local.nnz_rows = h->side[GLRM_ROWS].nnz; h->sig_local.nnz_cols = h->side[GLRM_COLS].nnz;
    if (!h->multi && (rc2 = glrm_prepare_tiled(h))) return rc2;
  }
  HIPCK(hipStreamSynchronize(st)); // host descriptor / index arrays may be released by the caller now
  if (h->storage == GLRM_STORAGE_F32 && (rc = glrm_narrow_views(h))) return rc; // from here on both views' vals are floats
  return GLRM_OK;
}

// Second half of create: kernel families and their buffers, chosen from the signature of the WHOLE problem.
static int finalize_impl(glrm_handle* h, const glrm_signature* whole) {
  h->sig = whole ? *whole : h->sig_local;
  if (!glrm_signature_covers(h->sig, h->sig_local))
    return fail(GLRM_ERR_INVALID, "the signature of the whole problem cannot be smaller than this shard's (sum the counts, max the rest)");
  int rc;
  const int opt_waves[2] = {h->opts.waves_row, h->opts.waves_col};
  if ((rc = glrm_setup_reforder(h))) return rc; // glrm_options.sum_order = 1: refuses models the validation sweeps do not cover
  if (h->sum_order_opt) {
    // reference-order validation sweeps: one lane per segment in list order, no family to choose and no view to re-order
    for (int s = 0; s < 2; ++s) { h->side[s].tiled = h->side[s].blocked = 0; h->side[s].waves = 1; }
    h->cached_row = h->cached_want = 0;
  } else if (h->storage == GLRM_STORAGE_F32) {
    // float storage: gather sweeps on both views; rows of at most cached_maxlen observations on the cached row sweep where
    // glrm_setup_cached says so, otherwise on the one-wave sweep; the phase-aligned passes where GLRM_HIP_BLOCKED asks for them
    // (glrm_setup_blocked; the other families have no float form)
    for (int s = 0; s < 2; ++s) h->side[s].tiled = h->side[s].blocked = 0;
    if ((rc = glrm_setup_cached(h))) return rc;
    if ((rc = glrm_setup_blocked(h))) return rc;
    if ((rc = plan_gather_sides(h))) return rc;
  } else if (h->multi || h->dense) {
    for (int s = 0; s < 2; ++s) h->side[s].waves = opt_waves[s] ? opt_waves[s] : (s == GLRM_ROWS ? 1 : 4);
    if (h->multi && (rc = glrm_setup_multi_split(h))) return rc;
  } else {
    // a failure from here on leaves re-ordered private views and partial buffers behind: the handle can then only be destroyed
    h->finalize_failed = true;
    if (glrm_test_fail_finalize())  // csrc/glrm_testhooks.hip: always 0 in the product library; the test build injects a failure on request
      return fail(GLRM_ERR_OOM, "injected set-up failure (test build hook)");
    if ((rc = glrm_setup_tiled(h))) return rc;
    if ((rc = glrm_setup_cached(h))) return rc;
    if ((rc = glrm_setup_blocked(h))) return rc;
    if ((rc = plan_gather_sides(h))) return rc;
    h->finalize_failed = false;
  }
  HIPCK(hipStreamSynchronize(h->stream));
  h->finalized = true;
  return GLRM_OK;
}

extern "C" int glrm_hip_create(glrm_handle** out, const glrm_problem* p, const glrm_options* o) {
  if (!out || !p) return fail(GLRM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (p->m <= 0 || p->n <= 0 || p->k <= 0) return fail(GLRM_ERR_INVALID, "m, n, k must be positive");
  if (p->m > INT32_MAX || p->n > INT32_MAX) return fail(GLRM_ERR_UNSUPPORTED, "m, n must fit int32 indices");
  int G, R;
  if (pick_layout(p->k, G, R)) return fail(GLRM_ERR_UNSUPPORTED, "rank k=%d is above the engine's limit of 128", p->k);
  if (p->row_begin < 0 || p->row_end > p->m || p->row_begin > p->row_end || p->col_begin < 0 || p->col_end > p->n ||
      p->col_begin > p->col_end)
    return fail(GLRM_ERR_INVALID, "shard ranges out of bounds");
  int rc = check_desc(p);
  if (rc) return rc;
  if ((rc = glrm_check_storage(p, o))) return rc;
  if ((p->flags & GLRM_PROBLEM_BORROW_DEVICE_ARRAYS) && (!(p->flags & GLRM_PROBLEM_DEVICE_ARRAYS) || p->dense_A))
    return fail(GLRM_ERR_INVALID, "GLRM_PROBLEM_BORROW_DEVICE_ARRAYS needs GLRM_PROBLEM_DEVICE_ARRAYS and observation lists (not dense_A)");
  const bool from_cols = (p->flags & GLRM_PROBLEM_ROWS_FROM_COLS) != 0;
  if (from_cols) {
    if (p->dense_A || (p->flags & GLRM_PROBLEM_BORROW_DEVICE_ARRAYS)) return fail(GLRM_ERR_INVALID, "GLRM_PROBLEM_ROWS_FROM_COLS: list problems, copied (not borrowed) arrays");
    if (p->rowptr || p->colidx || p->rowvals) return fail(GLRM_ERR_INVALID, "GLRM_PROBLEM_ROWS_FROM_COLS: rowptr / colidx / rowvals must be NULL (the engine derives the row view)");
    if (!(p->row_begin == 0 && p->row_end == p->m && p->col_begin == 0 && p->col_end == p->n))
      return fail(GLRM_ERR_INVALID, "GLRM_PROBLEM_ROWS_FROM_COLS needs the whole problem (a shard's rows meet every column)");
    if (!p->colptr) return fail(GLRM_ERR_INVALID, "colptr is NULL");
  }
  if (p->dense_A) {
    // validated in glrm_setup_dense
  } else if (!(p->flags & GLRM_PROBLEM_DEVICE_ARRAYS)) {
    rc = from_cols ? GLRM_OK : check_view("rowptr", p->row_end - p->row_begin, p->rowptr, p->colidx, p->rowvals, p->n, p, true, p->row_begin);
    if (rc) return rc;
    rc = check_view("colptr", p->col_end - p->col_begin, p->colptr, p->rowidx, p->colvals, p->m, p, false, p->col_begin);
    if (rc) return rc;
  } else if ((!from_cols && !p->rowptr) || !p->colptr) {
    return fail(GLRM_ERR_INVALID, "rowptr / colptr are NULL");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(GLRM_ERR_HIP, "no HIP device is visible (this engine has no CPU fallback)");
  int dev = o ? o->device_id : -1;
  if (dev < 0) HIPCK(hipGetDevice(&dev));
  if (dev >= ndev) return fail(GLRM_ERR_INVALID, "device_id %d out of range (%d devices)", dev, ndev);
  DeviceScope dg(dev);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", dev);
  glrm_handle* h = new (std::nothrow) glrm_handle();
  if (!h) return fail(GLRM_ERR_OOM, "out of host memory");
  h->device = dev;
  rc = create_impl(h, p, o);
  if (!rc && !(p->flags & GLRM_PROBLEM_DEFER_SETUP)) rc = finalize_impl(h, nullptr);
  if (rc) {
    char keep[sizeof g_err];
    memcpy(keep, g_err, sizeof keep);
    glrm_hip_destroy(h);
    memcpy(g_err, keep, sizeof keep);
    return rc;
  }
  *out = h;
  return GLRM_OK;
}

extern "C" int glrm_hip_signature(glrm_handle* h, glrm_signature* local) {
  if (!h || !local) return fail(GLRM_ERR_INVALID, "NULL argument");
  *local = h->sig_local;
  return GLRM_OK;
}

extern "C" int glrm_hip_finalize(glrm_handle* h, const glrm_signature* whole) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  if (h->finalized) return fail(GLRM_ERR_INVALID, "the handle is already set up (glrm_hip_finalize follows a GLRM_PROBLEM_DEFER_SETUP create, once)");
  if (h->finalize_failed)  // a set-up that failed half way (out of memory in a family's buffers) has re-ordered private views and partial buffers
    return fail(GLRM_ERR_INVALID, "an earlier glrm_hip_finalize on this handle failed: destroy it and create the shard again");
  DeviceScope dg(h->device);
  return finalize_impl(h, whole);
}

// ------------------------------------------------------------------ buffers and factors

static size_t factor_elem(const glrm_handle* h) { return h->storage == GLRM_STORAGE_F32 ? sizeof(float) : sizeof(double); }

// the handle's own buffer behind a factor / objective slot the caller has not bound: bytes, zeroed, allocated once
static int ensure_one(glrm_handle* h, double** used, double** own, size_t bytes) {
  if (*used) return GLRM_OK;
  if (!*own) {
    if (const int rc = h->mem.alloc(own, (bytes + 7) / 8)) return rc;
    HIPCK(hipMemsetAsync(*own, 0, bytes, h->stream));
  }
  *used = *own;
  return GLRM_OK;
}

static int ensure_owned(glrm_handle* h) {
  const size_t fe = factor_elem(h);
  glrm_handle::Side &rows = h->side[GLRM_ROWS], &cols = h->side[GLRM_COLS];
  int rc;
  if ((rc = ensure_one(h, &rows.factor, &rows.own_factor, (size_t)h->kp * h->m * fe))) return rc;
  if ((rc = ensure_one(h, &cols.factor, &cols.own_factor, (size_t)h->kp * h->d * fe))) return rc; // (d vectors: the embedding dimensions of the columns)
  if ((rc = ensure_one(h, &cols.obj, &cols.own_obj, (size_t)h->n * 8))) return rc;
  return ensure_one(h, &rows.obj, &rows.own_obj, (size_t)h->m * 8);
}

extern "C" int glrm_hip_factor_ld(glrm_handle* h) { return h ? h->kp : fail(GLRM_ERR_INVALID, "NULL handle"); }

extern "C" int glrm_hip_bind_buffers(glrm_handle* h, void* dX, void* dY, void* dObjCol, void* dObjRow) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  DeviceScope dg(h->device);
  h->side[GLRM_ROWS].factor = (double*)dX; h->side[GLRM_COLS].factor = (double*)dY; h->side[GLRM_COLS].obj = (double*)dObjCol; h->side[GLRM_ROWS].obj = (double*)dObjRow;
  if (h->iter_exec) { (void)hipGraphExecDestroy(h->iter_exec); h->iter_exec = nullptr; } // the captured launches hold the old pointers
  return ensure_owned(h);
}

extern "C" int glrm_hip_set_factors(glrm_handle* h, const double* X, const double* Y) {
  if (!h || !X || !Y) return fail(GLRM_ERR_INVALID, "NULL argument");
  if (h->storage == GLRM_STORAGE_F32) { // checked on the host, before the handle's factors are touched
    if (const int rcx = glrm_check_narrowable("X", X, (int64_t)h->k * h->m)) return rcx;
    if (const int rcy = glrm_check_narrowable("Y", Y, (int64_t)h->k * h->d)) return rcy;
  }
  DeviceScope dg(h->device);
  int rc = ensure_owned(h);
  if (rc) return rc;
  double *dX = h->side[GLRM_ROWS].factor, *dY = h->side[GLRM_COLS].factor;
  if (h->storage == GLRM_STORAGE_F32) {
    if ((rc = glrm_narrow_factor(h, X, dX, h->m))) return rc;
    return glrm_narrow_factor(h, Y, dY, h->d);
  }
  const size_t kb = (size_t)h->k * 8, pb = (size_t)h->kp * 8;
  if (h->kp != h->k) {
    HIPCK(hipMemsetAsync(dX, 0, pb * h->m, h->stream));
    HIPCK(hipMemsetAsync(dY, 0, pb * h->d, h->stream));
  }
  HIPCK(hipMemcpy2DAsync(dX, pb, X, kb, kb, (size_t)h->m, hipMemcpyHostToDevice, h->stream));
  HIPCK(hipMemcpy2DAsync(dY, pb, Y, kb, kb, (size_t)h->d, hipMemcpyHostToDevice, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  return GLRM_OK;
}

extern "C" int glrm_hip_get_factors(glrm_handle* h, double* X, double* Y) {
  if (!h || !X || !Y) return fail(GLRM_ERR_INVALID, "NULL argument");
  const double *dX = h->side[GLRM_ROWS].factor, *dY = h->side[GLRM_COLS].factor;
  if (!dX || !dY) return fail(GLRM_ERR_INVALID, "no factors on the device yet");
  DeviceScope dg(h->device);
  if (h->storage == GLRM_STORAGE_F32) {
    if (const int rc = glrm_widen_factor(h, dX, X, h->m)) return rc;
    return glrm_widen_factor(h, dY, Y, h->d);
  }
  const size_t kb = (size_t)h->k * 8, pb = (size_t)h->kp * 8;
  HIPCK(hipMemcpy2DAsync(X, kb, dX, pb, kb, (size_t)h->m, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipMemcpy2DAsync(Y, kb, dY, pb, kb, (size_t)h->d, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  return GLRM_OK;
}

extern "C" int glrm_hip_reset_stepsizes(glrm_handle* h, double stepsize) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  DeviceScope dg(h->device);
  for (const glrm_handle::Side& v : h->side)
    if (v.nseg > 0) hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((v.nseg + 255) / 256)), dim3(256), 0, h->stream, v.alpha, v.nseg, stepsize);
  HIPCK(hipGetLastError());
  return GLRM_OK;
}

static bool any_wrapped(const glrm_reg* rx, int64_t n_rx, const glrm_reg* ry, int64_t n_ry) {
  for (int64_t i = 0; i < n_rx; ++i) if (rx[i].wrap != 0) return true;
  for (int64_t i = 0; i < n_ry; ++i) if (ry[i].wrap != 0) return true;
  return false;
}

// Everything glrm_hip_set_regularizers refuses, without touching the handle: the multi-device entry point checks every shard's slice
// with it before it replaces any (csrc/glrm_multigpu.hip).
int glrm_check_regularizers(const glrm_handle* h, const glrm_reg* rx, int64_t n_rx, const glrm_reg* ry, int64_t n_ry) {
  if (!h || !rx || !ry) return fail(GLRM_ERR_INVALID, "NULL argument");
  if (n_rx != h->side[GLRM_ROWS].n_regs || n_ry != h->side[GLRM_COLS].n_regs)
    return fail(GLRM_ERR_INVALID, "regularizer counts must match the handle (rx %lld, ry %lld)", (long long)h->side[GLRM_ROWS].n_regs, (long long)h->side[GLRM_COLS].n_regs);
  if (h->storage == GLRM_STORAGE_F32)
    if (const int rc = glrm_check_storage_regs(rx, n_rx, ry, n_ry)) return rc;
  if (const int rc = check_regs("rx", rx, n_rx, h->k, nullptr, 0, 0, 0)) return rc;
  if (const int rc = check_regs("ry", ry, n_ry, h->k, h->losses_h.data(), (int64_t)h->losses_h.size(), h->side[GLRM_COLS].begin, h->side[GLRM_COLS].nseg)) return rc;
  // a handle created on the scalar fast paths moves to the general sweeps when a wrapper appears
  if (!h->multi && any_wrapped(rx, n_rx, ry, n_ry) && (h->dense || h->kp > 64))
    return fail(GLRM_ERR_UNSUPPORTED, "wrapped regularizers need a sparse-view handle with k <= 64");
  return GLRM_OK;
}

extern "C" int glrm_hip_set_regularizers(glrm_handle* h, const glrm_reg* rx, int64_t n_rx, const glrm_reg* ry, int64_t n_ry) {
  if (const int rc = glrm_check_regularizers(h, rx, n_rx, ry, n_ry)) return rc;
  DeviceScope dg(h->device);
  if (!h->multi && any_wrapped(rx, n_rx, ry, n_ry)) { // checked above: this handle can run the general sweeps
    if (h->finalized && !h->sum_order_opt) // (the part of set-up a handle that arrives late still needs; nothing of the handle has changed yet)
      if (const int rc = glrm_setup_multi_split(h)) return rc;
    h->multi = true;
  }
  glrm_handle::Side &rows = h->side[GLRM_ROWS], &cols = h->side[GLRM_COLS];
  rows.regs_h.assign(rx, rx + n_rx);
  cols.regs_h.assign(ry, ry + n_ry);
  const bool vx = any_vector_reg(rows.regs_h), vy = any_vector_reg(cols.regs_h);
  if ((vx != rows.vecreg || vy != cols.vecreg) && h->iter_exec) { // the captured iteration holds the other instantiation's launches
    (void)hipGraphExecDestroy(h->iter_exec);
    h->iter_exec = nullptr;
  }
  rows.vecreg = vx;
  cols.vecreg = vy;
  HIPCK(hipMemcpyAsync(rows.regs, rx, (size_t)n_rx * sizeof(glrm_reg), hipMemcpyHostToDevice, h->stream));
  HIPCK(hipMemcpyAsync(cols.regs, ry, (size_t)n_ry * sizeof(glrm_reg), hipMemcpyHostToDevice, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  if (rows.regvec || cols.regvec) { // the vectors of an earlier glrm_hip_set_regularizers_vec go with its descriptors (include/glrm_hip_regvec.h)
    glrm_regvec_drop(h);
    if (h->iter_exec) { (void)hipGraphExecDestroy(h->iter_exec); h->iter_exec = nullptr; }
  }
  return GLRM_OK;
}

extern "C" int glrm_hip_synchronize(glrm_handle* h) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  DeviceScope dg(h->device);
  HIPCK(hipStreamSynchronize(h->stream));
  return GLRM_OK;
}

// ------------------------------------------------------------------ sweep launch (glrm_sweep.hpp)

static void launch_sweep(int G, int R, int waves, int loss, int side, const SweepArgs& a, hipStream_t st) {
  if (a.storage == GLRM_STORAGE_F32) glrm_launch_sweep_f32(G, R, waves, loss, side, a, st);
  else launch_sweep_st<double>(G, R, waves, loss, side, a, st);
}


static int drain_events(glrm_handle* h) {
  for (auto& e : h->pending) {
    HIPCK(hipEventSynchronize(e.b));
    float ms = 0;
    HIPCK(hipEventElapsedTime(&ms, e.a, e.b));
    (e.slot < 2 ? h->side[e.slot].ms : h->ms_wait) += ms;
    h->pool.push_back(e);
  }
  h->pending.clear();
  return GLRM_OK;
}

// roctx ranges around every half-step (rocprofv3 --marker-trace shows "glrm step_x" / "glrm step_y" / "glrm col_losses" on the host
// timeline).  libroctx64 is looked up at run time so that the engine has no link-time dependency on the tracer; GLRM_HIP_ROCTX=0
// switches the ranges off.
struct RoctxApi {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  RoctxApi() {
    if (!knob(Knob::ROCTX)) return;
    void* lib = dlopen("libroctx64.so", RTLD_LAZY | RTLD_LOCAL);
    if (!lib) lib = dlopen("libroctx64.so.4", RTLD_LAZY | RTLD_LOCAL);
    if (!lib) return;
    push = (int (*)(const char*))dlsym(lib, "roctxRangePushA");
    pop = (int (*)())dlsym(lib, "roctxRangePop");
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
struct RoctxRange {
  static RoctxApi& api() { static RoctxApi a; return a; }
  explicit RoctxRange(const char* name) { if (api().push) api().push(name); }
  ~RoctxRange() { if (api().pop) api().pop(); }
};

// The loss variant a side's kernels are instantiated for (LOSS_*): one QuadLoss, one descriptor per segment, or -- the rows of a model
// with a loss per column -- one per observation; its columns read theirs by segment (*by_segment).  run_sweep launches it,
// glrm_hip_sum_order describes it.
static int loss_variant(const glrm_handle* h, int side, int* by_segment) {
  const bool per_column = !h->loss_quad_uniform && h->n_losses != 1;
  *by_segment = per_column && side == GLRM_COLS;
  if (h->loss_quad_uniform) return LOSS_QUAD_UNIFORM;
  const int loss = per_column && side == GLRM_ROWS ? LOSS_PER_OBS : LOSS_SEGMENT;
  return h->has_trig ? loss : loss + 2; // LOSS_*_NOTRIG: kernels compiled without the PeriodicLoss case
}

// An event pair from the pool (or a new one) with `a` recorded on the stream; end_timing records `b` behind what the caller timed and
// queues the pair for glrm_hip_kernel_stats (at 4096 waiting pairs it reads them out itself).  slot: glrm_handle::Ev
static int begin_timing(glrm_handle* h, int slot, glrm_handle::Ev* ev) {
  if (!h->pool.empty()) { *ev = h->pool.back(); h->pool.pop_back(); }
  else { HIPCK(hipEventCreate(&ev->a)); HIPCK(hipEventCreate(&ev->b)); }
  ev->slot = slot;
  HIPCK(hipEventRecord(ev->a, h->stream));
  return GLRM_OK;
}
static int end_timing(glrm_handle* h, const glrm_handle::Ev& ev) {
  HIPCK(hipEventRecord(ev.b, h->stream));
  h->pending.push_back(ev);
  return h->pending.size() >= 4096 ? drain_events(h) : GLRM_OK;
}

// launch(class, list, n, stream) for every populated class of a plan.  One class holds every local segment: one call without a list on
// h->stream.  Several: fork, main_cls on h->stream beside the other classes on the side stream (in class order), join.
template <typename Launch>
static int glrm_for_each_class(glrm_handle* h, const glrm_class_plan& p, int main_cls, const Launch& launch) {
  if (!p.list) {
    int cls = 1;
    for (int c = 0; c < 4; ++c) if (p.n[c] > 0) cls = c;
    return launch(cls, (const int32_t*)nullptr, p.n[cls], h->stream);
  }
  int rc = glrm_fork_side_stream(h);
  if (rc) return rc;
  int64_t off = 0;
  for (int c = 0; c < 4 && !rc; off += p.n[c], ++c)
    if (p.n[c] > 0) rc = launch(c, (const int32_t*)p.list + off, p.n[c], c == main_cls ? h->stream : h->side_stream);
  // join also before reporting an error: later work on h->stream (and a stream capture) must stay ordered after what the side stream already holds
  const hipError_t e_join = glrm_join_side_stream(h);
  if (rc) return rc;
  HIPCK(e_join);
  return GLRM_OK;
}

// One half-step of a side, or with eval_only its loss evaluation, as the request says (the entry points build it; the loss variant is filled
// in here).  glrm_side_family names the family; this is the dispatch on it.
static int run_sweep(glrm_handle* h, glrm_step step) {
  const int side = step.side;
  const bool eval_only = step.eval_only;
  RoctxRange range(eval_only ? "glrm col_losses" : (side == GLRM_ROWS ? "glrm step_x" : "glrm step_y"));
  GLRM_NEED_FINALIZED(h);
  int rc = ensure_owned(h);
  if (rc) return rc;
  SweepArgs a{};
  glrm_handle::Side& v = h->side[side];
  glrm_fill_side(a, h, step);
  a.storage = h->storage;
  if (a.nseg <= 0) return GLRM_OK;
  if (eval_only) a.trials = nullptr;
  a.seg_lo = 0;
  a.seg_hi = a.nseg;
  if (step.ranged()) { // glrm_hip_step_x_range
    if (step.row_end - step.row_begin <= 0) return GLRM_OK;
    if (v.plan.list) { // several classes: the class launches filter their lists by the range
      a.seg_lo = step.row_begin; a.seg_hi = step.row_end;
    } else {
      glrm_apply_row_range(a, step);
      a.seg_hi = a.nseg;
    }
  }
  step.loss = loss_variant(h, side, &step.loss_by_segment);
  const int loss = step.loss;
  a.loss_by_segment = step.loss_by_segment;
  glrm_handle::Ev ev{};
  const bool timed = h->profile && !eval_only;
  if (timed && (rc = begin_timing(h, side, &ev))) return rc;
  const glrm_family fam = glrm_side_family(h, side, eval_only);
  if (fam == GLRM_FAM_REFERENCE) {
    rc = glrm_run_reforder(h, step);
  } else if (fam == GLRM_FAM_GENERAL) {
    rc = glrm_run_multi(h, step);
  } else if (fam == GLRM_FAM_DENSE) {
    rc = glrm_run_dense(h, step);
  } else if (fam == GLRM_FAM_TILED || fam == GLRM_FAM_BLOCKED) {
    const bool divert = side == GLRM_COLS && h->blk_nlong_c > 0; // the very long columns: 8-wave gather sweep on the side stream, beside the passes
    if (divert) {
      // the gather sweep reads all of X: behind the sweeps already queued (fork) and, while X is still arriving
      // (glrm_hip_step_y_arrival), behind every block -- without holding up the passes on the main stream
      if ((rc = glrm_fork_side_stream(h))) return rc;
      for (int b = 0; step.arrivals && b < step.arrivals->n; ++b)
        if (void* e = step.arrivals->blocks[b].event) HIPCK(hipStreamWaitEvent(h->side_stream, (hipEvent_t)e, 0));
      SweepArgs b = a;
      b.seglist = h->blk_long_c;
      b.nseg = h->blk_nlong_c;
      launch_sweep(h->G, h->R, 8, loss, GLRM_COLS, b, h->side_stream);
    }
    rc = fam == GLRM_FAM_TILED ? glrm_run_tiled(h, step) : glrm_run_blocked(h, step);
    if (divert) (void)glrm_join_side_stream(h); // join before anything else (also before reporting an error: later work on the stream stays ordered)
  } else {
    // gather sweeps (and the cached row sweep), class by class -- see build_class_plan; the fullest class on the main stream (ties: the lower)
    const glrm_class_plan& p = v.plan;
    int main_cls = 0;
    for (int c = 1; c < 4; ++c) if (p.n[c] > p.n[main_cls]) main_cls = c;
    rc = glrm_for_each_class(h, p, main_cls, [&](int cls, const int32_t* list, int64_t n, hipStream_t st) {
      if (cls == 0 && !eval_only) return glrm_run_cached(h, step, list, n, p.cap, st);
      SweepArgs b = a;
      if (list) { b.seglist = list; b.nseg = n; }
      launch_sweep(h->G, h->R, glrm_class_waves(cls), loss, side, b, st);
      return (int)GLRM_OK;
    });
  }
  if (rc) return rc;
  HIPCK(hipGetLastError());
  if (timed && (rc = end_timing(h, ev))) return rc;
  if (!eval_only) v.launches += 1;
  return GLRM_OK;
}

// The requests the entry points make (what they do not name keeps glrm_step's default): a ProxGradParams half-step with its line search,
// one SparseProxGradParams step of a global step size, the loss evaluation over the column view.
static glrm_step search_step(int side, double min_stepsize) { glrm_step s{side}; s.min_stepsize = min_stepsize; return s; }
static glrm_step fixed_step(int side, double alpha) { glrm_step s{side}; s.fixed_alpha = alpha; return s; }
static glrm_step eval_step() { glrm_step s{GLRM_COLS}; s.eval_only = true; return s; }
static glrm_step search_step(bool, double) = delete; // `true` would mean columns: a side is GLRM_ROWS / GLRM_COLS (what the deleted bool
static glrm_step fixed_step(bool, double) = delete;  // overload of glrm_fill_side used to guard; every request is built by these three)

extern "C" int glrm_hip_step_x(glrm_handle* h, double min_stepsize) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  DeviceScope dg(h->device);
  return run_sweep(h, search_step(GLRM_ROWS, min_stepsize));
}

extern "C" int glrm_hip_step_x_range(glrm_handle* h, int64_t seg_begin, int64_t seg_end, double min_stepsize) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  GLRM_REFUSE_F32(h, "glrm_hip_step_x_range");
  if (seg_begin < 0 || seg_end > h->side[GLRM_ROWS].nseg || seg_begin > seg_end) return fail(GLRM_ERR_INVALID, "row range out of bounds");
  if (h->dense) return fail(GLRM_ERR_UNSUPPORTED, "step_x_range is not available on the dense path");
  DeviceScope dg(h->device);
  glrm_step step = search_step(GLRM_ROWS, min_stepsize);
  step.row_begin = seg_begin;
  step.row_end = seg_end;
  return run_sweep(h, step);
}

extern "C" int glrm_hip_step_y(glrm_handle* h, double min_stepsize) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  DeviceScope dg(h->device);
  return run_sweep(h, search_step(GLRM_COLS, min_stepsize));
}

// ---- glrm_hip_solve_x (include/glrm_hip_transform.h): inner_iter X half-steps with Y as it stands ------------------------------------
// the fused path: class 0 in one launch of the register kernel on the main stream, the longer rows `inner` launches of the gather sweep
// per class beside it (rows are independent: the classes run side by side)
static int solve_fused(glrm_handle* h, int inner, double min_stepsize) {
  RoctxRange range("glrm solve_x");
  int rc = ensure_owned(h);
  if (rc) return rc;
  glrm_handle::Side& v = h->side[GLRM_ROWS];
  // the handle's own plan where its rows are on the family (cached_row = 2: two waves, by solve_ok); else build_class_plan's with the rows the
  // two-wave register kernel takes as class 0 -- what a handle of the same problem has under GLRM_HIP_CACHED=1 -- built once, here
  glrm_class_plan& p = h->cached_row == 2 ? v.plan : h->solve_plan;
  if (!p.built && (rc = build_class_plan(h, GLRM_ROWS, glrm_cached_reg_maxlen(h->G), 2, &p))) return rc;
  glrm_step step = search_step(GLRM_ROWS, min_stepsize);
  step.loss = loss_variant(h, GLRM_ROWS, &step.loss_by_segment);
  SweepArgs a{};
  glrm_fill_side(a, h, step);
  a.storage = h->storage;
  a.seg_lo = 0;
  a.seg_hi = a.nseg;
  a.loss_by_segment = step.loss_by_segment;
  glrm_handle::Ev ev{};
  if (h->profile && (rc = begin_timing(h, GLRM_ROWS, &ev))) return rc;
  rc = glrm_for_each_class(h, p, 0, [&](int cls, const int32_t* list, int64_t n, hipStream_t st) {
    if (cls == 0) return glrm_run_solve(h, step, list, n, p.cap, inner, st);
    SweepArgs b = a;
    b.seglist = list;
    b.nseg = n;
    for (int it = 0; it < inner; ++it) launch_sweep(h->G, h->R, glrm_class_waves(cls), step.loss, GLRM_ROWS, b, st);
    return (int)GLRM_OK;
  });
  if (rc) return rc;
  HIPCK(hipGetLastError());
  if (h->profile && (rc = end_timing(h, ev))) return rc;
  v.launches += inner;
  h->solve_fused = 1;
  h->solve_fused_rows = p.n[0];
  h->solve_loop_rows = p.n[1] + p.n[2] + p.n[3];
  return GLRM_OK;
}

extern "C" int glrm_hip_solve_x(glrm_handle* h, int64_t inner_iter, double min_stepsize) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  if (inner_iter < 1 || inner_iter > INT32_MAX) return fail(GLRM_ERR_INVALID, "inner_iter must be in [1, 2^31 - 1]");
  GLRM_NEED_FINALIZED(h);
  DeviceScope dg(h->device);
  const glrm_handle::Side& v = h->side[GLRM_ROWS];
  // fused: set-up found the two-wave register kernel admissible (glrm_setup_cached) and the rows run the gather family now
  if (h->solve_ok && v.nseg > 0 && glrm_side_family(h, GLRM_ROWS, false) == GLRM_FAM_GATHER) return solve_fused(h, (int)inner_iter, min_stepsize);
  for (int64_t it = 0; it < inner_iter; ++it)
    if (const int rc = run_sweep(h, search_step(GLRM_ROWS, min_stepsize))) return rc;
  h->solve_fused = 0;
  h->solve_fused_rows = 0;
  h->solve_loop_rows = v.nseg;
  return GLRM_OK;
}

extern "C" int glrm_hip_solve_x_info(glrm_handle* h, int32_t* fused, int64_t* fused_rows, int64_t* loop_rows) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  if (h->solve_fused < 0) return fail(GLRM_ERR_INVALID, "glrm_hip_solve_x has not run on this handle");
  if (fused) *fused = h->solve_fused;
  if (fused_rows) *fused_rows = h->solve_fused_rows;
  if (loop_rows) *loop_rows = h->solve_loop_rows;
  return GLRM_OK;
}

// the Y half-step runs as passes over super-tiles (LDS-tiled, lane or phase-aligned)
static bool col_passes(const glrm_handle* h) {
  const glrm_family fam = glrm_side_family(h, GLRM_COLS, false);
  return fam == GLRM_FAM_TILED || fam == GLRM_FAM_BLOCKED;
}

// ---- the Y half-step while X is still arriving (include/glrm_hip.h: glrm_hip_step_y_arrival) ----------------------------------------
int glrm_arrival_wait(glrm_handle* h, glrm_arrivals& arr, int64_t lo, int64_t hi) {
  for (int b = 0; b < arr.n; ++b) {
    const glrm_arrival& blk = arr.blocks[b];
    if (arr.waited[b] || blk.end <= lo || blk.begin >= hi) continue;
    arr.waited[b] = 1;
    if (!blk.event) continue;
    glrm_handle::Ev ev{};
    if (h->profile) { // what the launch stream spends in front of a block that is not there yet (ms_wait_y)
      const int rc = begin_timing(h, 2, &ev);
      if (rc) return rc;
    }
    HIPCK(hipStreamWaitEvent(h->stream, (hipEvent_t)blk.event, 0));
    if (h->profile)
      if (const int rc = end_timing(h, ev)) return rc;
  }
  return GLRM_OK;
}

int glrm_for_sup_runs_in_arrival_order(glrm_handle* h, glrm_arrivals* arr, int nsup, int64_t rows_per_sup, const std::function<int(int, int)>& launch) {
  if (!arr || arr->n <= 0) return launch(0, nsup);
  if (nsup <= 1) { // one super-tile reads every row: behind ALL announced blocks (before session r6_69 it was launched without any wait --
                   // problems of at most one tile of rows on several shards raced with the exchange: tests/perf/soak_lane_shards.py, seed 5004)
    const int rc = glrm_arrival_wait(h, *arr, 0, h->m);
    return rc ? rc : launch(0, nsup);
  }
  // need[s] = the LAST announced block super-tile s touches: the run of super-tiles that become complete with block b is launched behind b
  std::vector<int> need((size_t)nsup, -1);
  for (int s = 0; s < nsup; ++s) {
    const int64_t lo = (int64_t)s * rows_per_sup, hi = std::min<int64_t>(lo + rows_per_sup, h->m);
    for (int b = 0; b < arr->n; ++b)
      if (arr->blocks[b].begin < hi && arr->blocks[b].end > lo && arr->blocks[b].begin < arr->blocks[b].end) need[s] = b;
  }
  for (int b = -1; b < arr->n; ++b) { // (-1: super-tiles no block touches -- beyond m -- first)
    for (int s = 0; s < nsup;) {
      if (need[s] != b) { ++s; continue; }
      int e = s + 1;
      while (e < nsup && need[e] == b) ++e;
      const int64_t lo = (int64_t)s * rows_per_sup, hi = std::min<int64_t>((int64_t)e * rows_per_sup, h->m);
      int rc = glrm_arrival_wait(h, *arr, lo, hi);
      if (!rc) rc = launch(s, e);
      if (rc) return rc;
      s = e;
    }
  }
  return GLRM_OK;
}

extern "C" int glrm_hip_step_y_arrival(glrm_handle* h, double min_stepsize, const glrm_arrival* blocks, int32_t n_blocks) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  GLRM_REFUSE_F32(h, "glrm_hip_step_y_arrival");
  if (n_blocks < 0 || (n_blocks > 0 && !blocks)) return fail(GLRM_ERR_INVALID, "bad block list");
  if (n_blocks == 0) return glrm_hip_step_y(h, min_stepsize);
  { // the blocks must tile [0, m): every row of X is either there or announced by exactly one event
    std::vector<std::pair<int64_t, int64_t>> r;
    for (int b = 0; b < n_blocks; ++b) {
      if (blocks[b].begin < 0 || blocks[b].end > h->m || blocks[b].begin > blocks[b].end) return fail(GLRM_ERR_INVALID, "arrival block %d: rows [%lld, %lld) out of range", b, (long long)blocks[b].begin, (long long)blocks[b].end);
      if (blocks[b].begin < blocks[b].end) r.emplace_back(blocks[b].begin, blocks[b].end);
    }
    std::sort(r.begin(), r.end());
    int64_t at = 0;
    for (auto& x : r) {
      if (x.first != at) return fail(GLRM_ERR_INVALID, "arrival blocks must tile the rows [0, m) of X without gaps or overlaps (at row %lld)", (long long)at);
      at = x.second;
    }
    if (at != h->m) return fail(GLRM_ERR_INVALID, "arrival blocks must tile the rows [0, m) of X (they end at row %lld of %lld)", (long long)at, (long long)h->m);
  }
  GLRM_NEED_FINALIZED(h);
  DeviceScope dg(h->device);
  glrm_arrivals arr{blocks, n_blocks, std::vector<char>((size_t)n_blocks, 0)};
  glrm_step step = search_step(GLRM_COLS, min_stepsize);
  step.arrivals = &arr;
  int rc = GLRM_OK;
  // the pass families of the column view can start on a part of X (the phase-aligned passes super-tile by super-tile in true arrival order,
  // the LDS-tiled / lane passes in runs of super-tiles in the announced order: round 6); everything else needs all of it
  const bool by_super_tile = col_passes(h) && knob(Knob::ARRIVAL);
  if (!by_super_tile) rc = glrm_arrival_wait(h, arr, 0, h->m);
  if (!rc) rc = run_sweep(h, step);
  if (!rc) rc = glrm_arrival_wait(h, arr, 0, h->m); // (a shard without columns launches nothing: later work on the stream still follows the arrivals)
  return rc;
}

// One prox-gradient step with a global step size and no line search (src/algorithms/sparse_proxgrad.jl:59-77, :81-99).
static int gradstep(glrm_handle* h, int side, double alpha) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  GLRM_REFUSE_F32(h, "glrm_hip_gradstep_x / glrm_hip_gradstep_y");
  if (!(alpha > 0.0)) return fail(GLRM_ERR_INVALID, "the step size must be positive");
  DeviceScope dg(h->device);
  return run_sweep(h, fixed_step(side, alpha));
}
extern "C" int glrm_hip_gradstep_x(glrm_handle* h, double alpha) { return gradstep(h, GLRM_ROWS, alpha); }
extern "C" int glrm_hip_gradstep_y(glrm_handle* h, double alpha) { return gradstep(h, GLRM_COLS, alpha); }

extern "C" int glrm_hip_col_losses(glrm_handle* h) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  DeviceScope dg(h->device);
  return run_sweep(h, eval_step());
}

static int run_penalty(glrm_handle* h, int side) {
  int rc = ensure_owned(h);
  if (rc) return rc;
  if (h->side[side].nseg <= 0) return GLRM_OK;
  if (h->multi) return glrm_run_multi_penalty(h, side);
  if (h->storage == GLRM_STORAGE_F32) glrm_launch_penalty_f32(h, side);
  else launch_penalty_st<double>(h, side);
  HIPCK(hipGetLastError());
  return GLRM_OK;
}

extern "C" int glrm_hip_row_penalties(glrm_handle* h) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  DeviceScope dg(h->device);
  return run_penalty(h, GLRM_ROWS);
}

extern "C" int glrm_hip_col_penalties(glrm_handle* h) {
  if (!h) return fail(GLRM_ERR_INVALID, "NULL handle");
  DeviceScope dg(h->device);
  return run_penalty(h, GLRM_COLS);
}

extern "C" int glrm_hip_sum(glrm_handle* h, const void* dvec, int64_t n, double* out) {
  if (!h || !out || (n > 0 && !dvec)) return fail(GLRM_ERR_INVALID, "NULL argument");
  DeviceScope dg(h->device);
  if (h->sum_order_opt) return glrm_reforder_sum(h, dvec, n, out); // sum(::Vector{Float64}) as Julia adds it (proxgrad.jl:205)
  hipLaunchKernelGGL(sum_stage1, dim3(SUM_BLOCKS), dim3(SUM_THREADS), 0, h->stream, (const double*)dvec, n, h->partials);
  hipLaunchKernelGGL(sum_stage2, dim3(1), dim3(SUM_THREADS), 0, h->stream, h->partials, h->dscalar);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(out, h->dscalar, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  return GLRM_OK;
}

static int count_sum(glrm_handle* h, const int32_t* v, int64_t n, int64_t* out) {
  *out = 0;
  if (n <= 0) return GLRM_OK;
  HIPCK(hipMemsetAsync(h->dcount, 0, 8, h->stream));
  hipLaunchKernelGGL(isum_kernel, dim3(256), dim3(256), 0, h->stream, v, n, h->dcount);
  HIPCK(hipGetLastError());
  unsigned long long r = 0;
  HIPCK(hipMemcpyAsync(&r, h->dcount, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  *out = (int64_t)r;
  return GLRM_OK;
}

extern "C" int glrm_hip_kernel_stats(glrm_handle* h, glrm_kernel_stats* out, int reset) {
  if (!h || !out) return fail(GLRM_ERR_INVALID, "NULL argument");
  DeviceScope dg(h->device);
  int rc = drain_events(h);
  if (rc) return rc;
  memset(out, 0, sizeof *out);
  out->launches_x = h->side[GLRM_ROWS].launches; out->launches_y = h->side[GLRM_COLS].launches;
  out->ms_x = h->side[GLRM_ROWS].ms; out->ms_y = h->side[GLRM_COLS].ms; out->ms_wait_y = h->ms_wait;
  int64_t* const n_trials[2] = {&out->trials_x, &out->trials_y};
  int64_t* const n_accepts[2] = {&out->accepts_x, &out->accepts_y};
  for (int s = 0; s < 2; ++s) {
    if ((rc = count_sum(h, h->side[s].trials, h->side[s].nseg, n_trials[s]))) return rc;
    if ((rc = count_sum(h, h->side[s].accepts, h->side[s].nseg, n_accepts[s]))) return rc;
  }
  out->nnz_rows = h->side[GLRM_ROWS].nnz; out->nnz_cols = h->side[GLRM_COLS].nnz;
  out->waves_row = h->side[GLRM_ROWS].waves; out->waves_col = h->side[GLRM_COLS].waves; out->ld = h->kp;
  out->tiled = h->multi ? 8 : (h->side[GLRM_ROWS].tiled ? 1 : 0) | (h->side[GLRM_COLS].tiled ? 2 : 0) | (h->dense ? 4 : 0) | (h->cached_row ? 64 : 0) | (h->side[GLRM_ROWS].blocked ? 16 : 0) |
               (h->side[GLRM_COLS].blocked ? 32 : 0) | (h->sum_order_opt ? 128 : 0) | (h->side[GLRM_ROWS].lane ? 256 : 0) | (h->side[GLRM_COLS].lane ? 512 : 0); // bit8 / bit9: lane-per-segment form of the LDS-tiled row / column passes; bit0 / bit1: LDS-tiled row / column sweep, bit4 / bit5: phase-aligned gather passes, bit7: reference order
  if (reset) {
    for (glrm_handle::Side& v : h->side) { v.launches = 0; v.ms = 0; }
    h->ms_wait = 0;
    if ((rc = zero_counters(h))) return rc;
  }
  return GLRM_OK;
}

// The order in which this handle adds a segment's terms (include/glrm_hip.h: glrm_sum_order) -- a description of what the kernels of
// the family that run_sweep dispatches do, read from the same handle fields.  The CPU oracle adopts it (glrm_cpu_set_sum_order) and then
// lands on this engine's factors bit for bit: tests/test_gpu_sum_order.py.
extern "C" int glrm_hip_sum_order(glrm_handle* handle, int32_t side, glrm_sum_order* out) {
  const glrm_handle* h = handle; // a query: nothing is written
  if (!h || !out || (side != GLRM_ROWS && side != GLRM_COLS)) return fail(GLRM_ERR_INVALID, "bad argument");
  GLRM_NEED_FINALIZED(h);
  const glrm_family fam = glrm_side_family(h, side, false);
  glrm_sum_order o{};
  o.cached_maxlen = -1;
  o.waves4_from = GLRM_WAVES4_FROM;
  o.waves8_from = GLRM_WAVES8_FROM;
  int by_segment; // the loss variant run_sweep instantiates
  const int loss = loss_variant(h, side, &by_segment);
  const bool quad = loss == LOSS_QUAD_UNIFORM, per_obs = loss_mode(loss) == LOSS_PER_OBS;
  if (side == GLRM_COLS && col_passes(h)) o.long_from = (int32_t)std::min<int64_t>(h->blk_long_from, INT32_MAX);
  if (fam == GLRM_FAM_REFERENCE) {
    o.family = GLRM_ORDER_REFERENCE; // glrm_reforder.hip: one lane per segment, list order, one accumulator per sum
    o.lanes = 1; o.comps = h->kp;
  } else if (fam == GLRM_FAM_GENERAL || fam == GLRM_FAM_DENSE) {
    o.family = GLRM_ORDER_OTHER;
  } else if (fam == GLRM_FAM_TILED) {
    const int T = glrm_tile_rows(h->kp); // vectors per staged tile
    o.family = GLRM_ORDER_WINDOWED;
    o.lanes = h->tG; o.comps = h->tR;
    o.window = T;
    o.windows_per_sup = side == GLRM_ROWS ? 0 : h->side[side].pass.tiles_per_sup; // (rows: one super-tile, nothing re-added = 0)
    o.batch = (!quad && (h->tG == 4 || h->tG == 8)) ? h->tG : 2;
    o.rotate = (side == GLRM_COLS && !quad && (h->tG == 4 || h->tG == 8) && h->tR == 8) ? 1 : 0;
    // a private copy in another order: lists the engine tile-sorted, rows regrouped by loss kind inside the tile windows
    const bool sorted_here = side == GLRM_ROWS ? h->sig_local.rows_unordered != 0 : h->sig_local.cols_unordered != 0;
    o.private_order = sorted_here ? 1 : h->side[side].grouped ? 2 : 0; // (2: stable grouping by ascending loss kind inside every window, glrm_tiled.hpp: group_rows_by_kind_kernel -- the oracle restates it)
    if (h->side[side].lane) { // lane-per-segment passes (glrm_lane.hpp): two fma chains over the even / odd chunks = the two-lane layout, rotated walk
      o.lanes = 2; o.comps = h->kp / 2;
      o.batch = 2;
      o.rotate = 2;
      o.window = T;
      o.windows_per_sup = side == GLRM_ROWS ? 0 : h->side[side].pass.tiles_per_sup;
    }
  } else if (fam == GLRM_FAM_BLOCKED) {
    o.family = GLRM_ORDER_WINDOWED;
    o.lanes = h->G; o.comps = h->R;
    o.window = (int64_t)glrm_tile_rows(h->kp) * h->side[side].pass.tiles_per_sup; // one walk per super-tile: the super-tile is the window
    o.windows_per_sup = 1;
    o.batch = (!quad && (h->G == 4 || h->G == 8)) ? h->G : 2;
  } else {
    o.family = GLRM_ORDER_STRIDED;
    o.lanes = h->G; o.comps = h->R;
    const int forced = glrm_forced_class(h, side);
    o.waves = forced ? glrm_class_waves(forced) : 0;
    if (side == GLRM_ROWS && h->cached_want) { // which rows the cached sweep takes is a function of the row's own length
      o.cached_maxlen = h->cached_maxlen; // (the whole problem's, also on a shard that holds no such row)
      o.cached_waves = h->cached_waves;
    }
    // four observations per trip with one loss evaluation per lane (sweep_pass: SCATTER): G == 4 and not the uniform QuadLoss kernel;
    // the per-segment variant only on one-wave segments (launch_sweep_loss)
    o.batch = (!quad && h->G == 4) ? 4 : 1;
    o.batch_one_wave_only = (o.batch == 4 && !per_obs) ? 1 : 0;
  }
  *out = o;
  return GLRM_OK;
}

// ------------------------------------------------------------------ whole-fit API

// loss + rx + ry at the device-resident factors (objective(...), src/evaluate_fit.jl:4-23,91-104)
static int device_objective(glrm_handle* h, int include_reg, double* out) {
  int rc;
  double loss = 0, px = 0, py = 0;
  if (h->sum_order_opt) { // reference order: one accumulator over every observation, columns outer (src/evaluate_fit.jl:12-21)
    if ((rc = ensure_owned(h))) return rc;
    return glrm_reforder_objective(h, include_reg, out);
  }
  if ((rc = run_sweep(h, eval_step()))) return rc;
  if ((rc = glrm_hip_sum(h, h->side[GLRM_COLS].obj, h->n, &loss))) return rc;
  if (include_reg) {
    if ((rc = run_penalty(h, GLRM_ROWS))) return rc;
    if ((rc = glrm_hip_sum(h, h->side[GLRM_ROWS].obj, h->m, &px))) return rc;
    if ((rc = run_penalty(h, GLRM_COLS))) return rc;
    if ((rc = glrm_hip_sum(h, h->side[GLRM_COLS].obj, h->n, &py))) return rc;
  }
  *out = loss + (px + py);
  return GLRM_OK;
}

extern "C" int glrm_hip_objective(glrm_handle* h, const double* X, const double* Y, int include_reg, double* out) {
  if (!h || !X || !Y || !out) return fail(GLRM_ERR_INVALID, "NULL argument");
  if (!glrm_single_shard(h)) return fail(GLRM_ERR_INVALID, "glrm_hip_objective needs a single-shard handle");
  DeviceScope dg(h->device);
  int rc = glrm_hip_set_factors(h, X, Y);
  if (rc) return rc;
  return device_objective(h, include_reg, out);
}

// One outer iteration as a hipGraph.  Eligible: gather sweeps (fixed launch sequence, no host round trips inside a half-step) on
// the handle's private stream (the legacy default stream cannot be captured), no per-launch event timing.
static bool graph_eligible(const glrm_handle* h) {
  return h->own_stream && !h->profile && glrm_side_family(h, GLRM_ROWS, false) == GLRM_FAM_GATHER && glrm_side_family(h, GLRM_COLS, false) == GLRM_FAM_GATHER &&
         !h->cached_row && knob(Knob::GRAPH) != 0;
}

static int build_iteration_graph(glrm_handle* h, const glrm_params* prm) {
  if (h->iter_exec && h->graph_ix == prm->inner_iter_X && h->graph_iy == prm->inner_iter_Y && h->graph_min == prm->min_stepsize &&
      h->graph_step == prm->stepsize)
    return GLRM_OK;
  if (h->iter_exec) { (void)hipGraphExecDestroy(h->iter_exec); h->iter_exec = nullptr; }
  if (h->iter_graph) { (void)hipGraphDestroy(h->iter_graph); h->iter_graph = nullptr; }
  if (!h->pinned_obj) HIPCK(hipHostMalloc((void**)&h->pinned_obj, 8, hipHostMallocDefault));
  int rc = ensure_owned(h);
  if (rc) return rc;
  HIPCK(hipStreamSynchronize(h->stream));
  if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return GLRM_OK; } // no graph: plain launches
  bool ok = true;
  const int64_t lx = h->side[GLRM_ROWS].launches, ly = h->side[GLRM_COLS].launches;
  if (prm->inner_iter_X > 1 || prm->inner_iter_Y > 1) ok = ok && glrm_hip_reset_stepsizes(h, prm->stepsize) == GLRM_OK;
  for (int64_t in = 0; ok && in < prm->inner_iter_X; ++in) ok = run_sweep(h, search_step(GLRM_ROWS, prm->min_stepsize)) == GLRM_OK;
  for (int64_t in = 0; ok && in < prm->inner_iter_Y; ++in) ok = run_sweep(h, search_step(GLRM_COLS, prm->min_stepsize)) == GLRM_OK;
  if (ok) {
    hipLaunchKernelGGL(sum_stage1, dim3(SUM_BLOCKS), dim3(SUM_THREADS), 0, h->stream, (const double*)h->side[GLRM_COLS].obj, h->n, h->partials);
    hipLaunchKernelGGL(sum_stage2, dim3(1), dim3(SUM_THREADS), 0, h->stream, h->partials, h->dscalar);
    ok = hipMemcpyAsync(h->pinned_obj, h->dscalar, 8, hipMemcpyDeviceToHost, h->stream) == hipSuccess;
  }
  h->side[GLRM_ROWS].launches = lx; h->side[GLRM_COLS].launches = ly; // capturing is not launching
  hipGraph_t g = nullptr;
  const hipError_t ec = hipStreamEndCapture(h->stream, &g);
  if (!ok || ec != hipSuccess || !g) { if (g) (void)hipGraphDestroy(g); (void)hipGetLastError(); return GLRM_OK; }
  if (hipGraphInstantiate(&h->iter_exec, g, nullptr, nullptr, 0) != hipSuccess) { (void)hipGraphDestroy(g); h->iter_exec = nullptr; (void)hipGetLastError(); return GLRM_OK; }
  h->iter_graph = g;
  h->graph_ix = prm->inner_iter_X; h->graph_iy = prm->inner_iter_Y; h->graph_min = prm->min_stepsize; h->graph_step = prm->stepsize;
  return GLRM_OK;
}

extern "C" int glrm_hip_fit(glrm_handle* h, const glrm_params* prm, double* X, double* Y, double* objective,
                            double* seconds, int64_t cap, int64_t* n_recorded) {
  if (!h || !prm || !X || !Y || !objective || !seconds || !n_recorded) return fail(GLRM_ERR_INVALID, "NULL argument");
  if (!glrm_single_shard(h)) return fail(GLRM_ERR_INVALID, "glrm_hip_fit needs a single-shard handle (use the step-level API per shard)");
  int rc;
  if ((rc = glrm_check_fit_args(prm, cap, Y, h->k, h->d))) return rc;
  DeviceScope dg(h->device);
  if ((rc = glrm_hip_set_factors(h, X, Y))) return rc;                 // X = glrm.X; Y = glrm.Y (:43)
  if ((rc = glrm_hip_reset_stepsizes(h, prm->stepsize))) return rc;   // :69-70
  glrm_trace trace(objective, seconds, prm, h->side[GLRM_ROWS].nnz);  // :72 (observed_features)
  double obj0 = 0.0;
  if ((rc = device_objective(h, 1, &obj0))) return rc;
  trace.start(obj0);
  const bool use_graph = graph_eligible(h);
  if (use_graph && (rc = build_iteration_graph(h, prm))) return rc;
  for (int64_t i = 1; i <= prm->max_iter; ++i) {                       // :107
    double obj = 0.0;
    if (use_graph && h->iter_exec) { // the same launches, replayed from one hipGraph
      HIPCK(hipGraphLaunch(h->iter_exec, h->stream));
      HIPCK(hipStreamSynchronize(h->stream));
      obj = *h->pinned_obj;
      h->side[GLRM_ROWS].launches += prm->inner_iter_X; h->side[GLRM_COLS].launches += prm->inner_iter_Y;
    } else {
      if (prm->inner_iter_X > 1 || prm->inner_iter_Y > 1)
        if ((rc = glrm_hip_reset_stepsizes(h, prm->stepsize))) return rc; // :112-115
      for (int64_t in = 0; in < prm->inner_iter_X; ++in)
        if ((rc = run_sweep(h, search_step(GLRM_ROWS, prm->min_stepsize)))) return rc; // :117-158
      for (int64_t in = 0; in < prm->inner_iter_Y; ++in)
        if ((rc = run_sweep(h, search_step(GLRM_COLS, prm->min_stepsize)))) return rc; // :160-203
      if ((rc = glrm_hip_sum(h, h->side[GLRM_COLS].obj, h->n, &obj))) return rc;     // obj = sum(obj_by_col) :205
    }
    if (trace.record(i, obj)) break;
  }
  if ((rc = glrm_hip_get_factors(h, X, Y))) return rc;
  *n_recorded = trace.nrec;
  return GLRM_OK;
}

// fit!(glrm::GLRM, params::SparseProxGradParams), src/algorithms/sparse_proxgrad.jl:22-134: global step size, one
// gradient + prox step per factor and iteration, whole-iteration accept / revert on the full objective.
extern "C" int glrm_hip_fit_sparse(glrm_handle* h, const glrm_sparse_params* prm, double* X, double* Y, double* objective,
                                   double* seconds, int64_t cap, int64_t* n_recorded) {
  if (!h || !prm || !X || !Y || !objective || !seconds || !n_recorded) return fail(GLRM_ERR_INVALID, "NULL argument");
  GLRM_REFUSE_F32(h, "glrm_hip_fit_sparse");
  if (!glrm_single_shard(h)) return fail(GLRM_ERR_INVALID, "glrm_hip_fit_sparse needs a single-shard handle");
  if (prm->max_iter < 0 || cap < prm->max_iter + 2) return fail(GLRM_ERR_INVALID, "objective/seconds capacity must be >= max_iter+2");
  if (prm->inner_iter < 1) return fail(GLRM_ERR_INVALID, "inner_iter must be >= 1");
  // norm(Y)==0 would be re-randomised by the reference (:41-43); not reproducible -> error
  if (glrm_all_zero(Y, (int64_t)h->k * h->d)) return fail(GLRM_ERR_INVALID, "Y is all zeros");
  DeviceScope dg(h->device);
  int rc;
  if ((rc = glrm_hip_set_factors(h, X, Y))) return rc; // working copies X, Y (:33); glrm.X / glrm.Y = best so far
  const size_t xb = (size_t)h->kp * h->m * 8, yb = (size_t)h->kp * h->d * 8;
  DevArena scratch;
  double *bestX = nullptr, *bestY = nullptr;
  if ((rc = scratch.alloc(&bestX, xb / 8)) || (rc = scratch.alloc(&bestY, yb / 8))) return rc;
  // X then Y between the working factors and the best model so far, on the handle's stream
  auto copy_factors = [&](bool to_best) {
    double *wx = h->side[GLRM_ROWS].factor, *wy = h->side[GLRM_COLS].factor;
    const bool ok = hipMemcpyAsync(to_best ? bestX : wx, to_best ? wx : bestX, xb, hipMemcpyDeviceToDevice, h->stream) == hipSuccess &&
                    hipMemcpyAsync(to_best ? bestY : wy, to_best ? wy : bestY, yb, hipMemcpyDeviceToDevice, h->stream) == hipSuccess;
    return ok ? (int)GLRM_OK : fail(GLRM_ERR_HIP, "device copy failed");
  };
  if ((rc = copy_factors(true))) return rc;
  double alpha = prm->stepsize;                              // :46
  const double tol = prm->abs_tol * (double)h->side[GLRM_ROWS].nnz;        // :48
  int64_t nrec = 0;
  if ((rc = device_objective(h, 1, &objective[0]))) return rc; // update_ch!(ch, 0, objective(glrm; sparse=true)) :52
  seconds[0] = 0.0;
  nrec = 1;
  double t = now_s();
  int64_t steps_in_a_row = 0;
  for (int64_t i = 1; i <= prm->max_iter; ++i) {
    for (int64_t in = 0; in < prm->inner_iter; ++in) if ((rc = run_sweep(h, fixed_step(GLRM_ROWS, alpha)))) return rc;
    for (int64_t in = 0; in < prm->inner_iter; ++in) if ((rc = run_sweep(h, fixed_step(GLRM_COLS, alpha)))) return rc;
    double obj = 0.0;
    if ((rc = device_objective(h, 1, &obj))) return rc; // :102
    if (obj < objective[nrec - 1]) {                              // :104-110
      const double dt = now_s() - t;
      objective[nrec] = obj;
      seconds[nrec] = seconds[nrec - 1] + dt;
      ++nrec;
      if ((rc = copy_factors(true))) return rc;
      alpha = alpha * 1.05;
      steps_in_a_row = steps_in_a_row + 1 > 1 ? steps_in_a_row + 1 : 1;
      t = now_s();
    } else {                                                      // :111-117
      const double div = -(double)steps_in_a_row > 1.5 ? -(double)steps_in_a_row : 1.5;
      alpha = alpha / div;
      if ((rc = copy_factors(false))) return rc;
      steps_in_a_row = steps_in_a_row - 1 < 0 ? steps_in_a_row - 1 : 0;
    }
    // :119  i>10 && (steps_in_a_row > 3 && ch.objective[end-1] - obj < tol) || alpha <= params.min_stepsize
    if ((i > 10 && (steps_in_a_row > 3 && nrec >= 2 && objective[nrec - 2] - obj < tol)) || alpha <= prm->min_stepsize) break;
  }
  // :126-127 the last objective is recorded once more with the remaining time
  objective[nrec] = objective[nrec - 1];
  seconds[nrec] = seconds[nrec - 1] + (now_s() - t);
  ++nrec;
  // glrm.X, glrm.Y are the best model found
  if ((rc = copy_factors(false))) return rc;
  rc = glrm_hip_get_factors(h, X, Y);
  *n_recorded = nrec;
  return rc;
}
