// glrm_stream.hip -- include/glrm_hip_stream.h: glrm_hip_stream_plan (pure host code), glrm_hip_stream_rows, the reference's one-pass
// streaming_fit! on the device, and glrm_hip_stream_info.  The header is the specification of the plan and of the arithmetic; the kernels
// are glrm_stream.hpp.  This unit holds the plan, the refusals (in the order of als_check, glrm_als.hip), the state of the handle
// (glrm_handle::stream_state: epoch, kept from call to call and zeroed by every call, and what the last call did) and the launch loop.
#include <chrono>
#include <cmath>

#include "glrm_stream.hpp"

using namespace glrm;

namespace {

const char* const STREAM_HEADER = "include/glrm_hip_stream.h";
constexpr int64_t STREAM_PIECE = 2048; // rows per kernel of a chain launch: no kernel runs for seconds

struct StreamPlan {
  std::vector<int64_t> level;          // row - first -> level, from 1
  std::vector<char> dup;               // row - first -> names a column twice
  int64_t nlevels = 0, nlaunches = 0, max_width = 0, dup_rows = 0;
  std::vector<int32_t> order;          // rows by (level, row)
  std::vector<int64_t> lptr;           // level l (1-based) holds order[lptr[l - 1] .. lptr[l])
};

// the plan of include/glrm_hip_stream.h; rowptr / qptr are indexed by the row, colidx / qcol by rowptr[i] - off / qptr[i]
void stream_make_plan(int64_t m, int64_t n, int64_t first, const int64_t* rowptr, const int32_t* colidx, int64_t off, const int64_t* qptr, const int32_t* qcol,
                      bool sequential, StreamPlan& p) {
  const int64_t rows = m - first;
  p.level.assign((size_t)rows, 0);
  p.dup.assign((size_t)rows, 0);
  std::vector<int64_t> lastw((size_t)n, 0), lastr((size_t)n, 0), seen((size_t)n, -1);
  for (int64_t i = first; i < m; ++i) {
    int64_t L = 0;
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int32_t j = colidx[e - off];
      L = std::max(L, std::max(lastw[j], lastr[j]));
      if (seen[j] == i) p.dup[i - first] = 1;
      seen[j] = i;
    }
    if (qptr)
      for (int64_t e = qptr[i]; e < qptr[i + 1]; ++e) L = std::max(L, lastw[qcol[e]]);
    ++L;
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) lastw[colidx[e - off]] = L;
    if (qptr)
      for (int64_t e = qptr[i]; e < qptr[i + 1]; ++e) lastr[qcol[e]] = std::max(lastr[qcol[e]], L);
    p.level[i - first] = sequential ? i - first + 1 : L;
    p.dup_rows += p.dup[i - first];
  }
  for (int64_t r = 0; r < rows; ++r) p.nlevels = std::max(p.nlevels, p.level[r]);
  p.lptr.assign((size_t)p.nlevels + 1, 0);
  for (int64_t r = 0; r < rows; ++r) ++p.lptr[p.level[r]];
  for (int64_t l = 1; l <= p.nlevels; ++l) {
    p.max_width = std::max(p.max_width, p.lptr[l]);
    p.lptr[l] += p.lptr[l - 1];
  }
  p.order.resize((size_t)rows);
  std::vector<int64_t> at(p.lptr);     // at[l - 1]: where the next row of level l goes
  for (int64_t r = 0; r < rows; ++r) p.order[at[p.level[r] - 1]++] = (int32_t)r;
  bool chain = false;                  // the level before this one was a one-row level
  for (int64_t l = 1; l <= p.nlevels; ++l) {
    const bool one = p.lptr[l] - p.lptr[l - 1] == 1;
    if (!one || !chain) ++p.nlaunches;
    chain = one;
  }
}

// the query lists of a call: offsets that ascend from 0, columns inside 0 .. n-1
int stream_check_queries(const char* what, int64_t m, int64_t n, const int64_t* qptr, const int32_t* qcol) {
  if (qptr[0] != 0) return fail(GLRM_ERR_INVALID, "%s: qptr[0] is %lld, the query offsets ascend from 0", what, (long long)qptr[0]);
  for (int64_t i = 0; i < m; ++i)
    if (qptr[i + 1] < qptr[i]) return fail(GLRM_ERR_INVALID, "%s: qptr[%lld] = %lld is below qptr[%lld] = %lld", what, (long long)(i + 1), (long long)qptr[i + 1], (long long)i, (long long)qptr[i]);
  for (int64_t e = 0; e < qptr[m]; ++e)
    if (qcol[e] < 0 || qcol[e] >= n) return fail(GLRM_ERR_INVALID, "%s: query %lld names column %d, outside 0 .. %lld", what, (long long)e, (int)qcol[e], (long long)(n - 1));
  return GLRM_OK;
}

int stream_check_reg(const char* what, const char* name, const glrm_handle::Side& v) {
  for (size_t s = 0; s < v.regs_h.size(); ++s) {
    const glrm_reg& r = v.regs_h[s];
    if ((r.kind != GLRM_REG_QUAD && r.kind != GLRM_REG_ZERO) || r.wrap != 0)
      return fail(GLRM_ERR_UNSUPPORTED, "%s: %s[%lld] has regularizer kind %d, wrap %d; the streaming pass needs a plain QuadReg (kind %d) or ZeroReg (kind %d) (%s)", what, name,
                  (long long)s, r.kind, r.wrap, (int)GLRM_REG_QUAD, (int)GLRM_REG_ZERO, STREAM_HEADER);
    if (r.kind == GLRM_REG_QUAD && !(r.scale >= 0.0))
      return fail(GLRM_ERR_UNSUPPORTED, "%s: %s[%lld] is QuadReg with scale %g; the streaming pass needs a scale >= 0 (%s)", what, name, (long long)s, r.scale, STREAM_HEADER);
  }
  if (v.regvec) return fail(GLRM_ERR_UNSUPPORTED, "%s: the %s carry a vector (glrm_hip_set_regularizers_vec); the streaming pass needs a plain QuadReg or ZeroReg (%s)", what, name, STREAM_HEADER);
  return GLRM_OK;
}

double stream_reg_scale(const glrm_reg& r) { return r.kind == GLRM_REG_QUAD ? r.scale : 0.0; }

// everything glrm_hip_stream_rows refuses, nothing touched
int stream_check(glrm_handle* h, int64_t first, double stepsize, int64_t interval, const int64_t* qptr, const int32_t* qcol, const double* qout, const char* what) {
  if (!h) return fail(GLRM_ERR_INVALID, "%s: NULL handle", what);
  GLRM_NEED_FINALIZED(h);
  if (h->storage == GLRM_STORAGE_F32)
    return fail(GLRM_ERR_UNSUPPORTED, "%s is not available with storage = f32 (glrm_options.storage = 1): the pass reads fp64 lists and factors (%s)", what, STREAM_HEADER);
  if (h->dense) return fail(GLRM_ERR_UNSUPPORTED, "%s works on the observation lists: this handle was created from dense_A (%s)", what, STREAM_HEADER);
  if (!glrm_single_shard(h))
    return fail(GLRM_ERR_UNSUPPORTED, "%s needs the whole problem on one handle: this one is a shard (rows [%lld, %lld) of %lld, columns [%lld, %lld) of %lld; %s)", what,
                (long long)h->side[GLRM_ROWS].begin, (long long)h->side[GLRM_ROWS].end, (long long)h->m, (long long)h->side[GLRM_COLS].begin,
                (long long)h->side[GLRM_COLS].end, (long long)h->n, STREAM_HEADER);
  if (h->k > GLRM_STREAM_MAX_K) return fail(GLRM_ERR_UNSUPPORTED, "%s: rank k = %d is above GLRM_STREAM_MAX_K = %d (%s)", what, h->k, GLRM_STREAM_MAX_K, STREAM_HEADER);
  for (size_t j = 0; j < h->losses_h.size(); ++j) {
    if (h->losses_h[j].kind != GLRM_LOSS_QUAD)
      return fail(GLRM_ERR_UNSUPPORTED, "%s: column %lld has loss kind %d; the streaming pass needs QuadLoss (kind %d) on every column (%s)", what, (long long)j,
                  h->losses_h[j].kind, (int)GLRM_LOSS_QUAD, STREAM_HEADER);
    if (h->losses_h[j].scale != 1.0)
      return fail(GLRM_ERR_UNSUPPORTED, "%s: column %lld is QuadLoss with scale %g; the streaming pass needs a scale of exactly 1 (the reference's loop ignores the scale) (%s)", what,
                  (long long)j, h->losses_h[j].scale, STREAM_HEADER);
  }
  int rc = stream_check_reg(what, "rx", h->side[GLRM_ROWS]);
  if (rc) return rc;
  if ((rc = stream_check_reg(what, "ry", h->side[GLRM_COLS]))) return rc;
  const std::vector<glrm_reg>& ry = h->side[GLRM_COLS].regs_h;
  for (size_t s = 1; s < ry.size(); ++s)
    if (stream_reg_scale(ry[s]) != stream_reg_scale(ry[0]))
      return fail(GLRM_ERR_UNSUPPORTED, "%s: ry[%lld] has scale %g and ry[0] has %g; the streaming pass divides all of Y by one constant and needs equal scales (%s)", what, (long long)s,
                  stream_reg_scale(ry[s]), stream_reg_scale(ry[0]), STREAM_HEADER);
  if (h->multi || h->d != h->n)
    return fail(GLRM_ERR_UNSUPPORTED, "%s: the model runs on the general sweeps (multi-dimensional losses, wrapped or vector regularizers); the streaming pass does not (%s)", what,
                STREAM_HEADER);
  if (!h->side[GLRM_ROWS].factor || !h->side[GLRM_COLS].factor)
    return fail(GLRM_ERR_INVALID, "%s: no factors on the device yet (fit, glrm_hip_set_factors or glrm_hip_bind_buffers first)", what);
  if (first < 1 || first > h->m) return fail(GLRM_ERR_INVALID, "%s: first must be in 1 .. m = %lld, got %lld", what, (long long)h->m, (long long)first);
  if (interval < 1) return fail(GLRM_ERR_INVALID, "%s: interval must be at least 1, got %lld", what, (long long)interval);
  if (!(std::isfinite(stepsize) && stepsize > 0.0)) return fail(GLRM_ERR_INVALID, "%s: stepsize must be finite and > 0, got %g", what, stepsize);
  if ((qptr != nullptr) != (qcol != nullptr) || (qptr != nullptr) != (qout != nullptr))
    return fail(GLRM_ERR_INVALID, "%s: qptr, qcol and qout go together (all three, or NULL, NULL, NULL)", what);
  if (qptr && (rc = stream_check_queries(what, h->m, h->n, qptr, qcol))) return rc;
  return GLRM_OK;
}

// device memory of one call, from the handle's arena: released when the call returns, on every path
struct StreamCallMem {
  glrm_handle* h;
  std::vector<void**> held;
  explicit StreamCallMem(glrm_handle* h_) : h(h_) {}
  template <class T>
  int alloc(T** p, size_t count) {
    const int rc = h->mem.alloc(p, count);
    if (!rc) held.push_back((void**)p);
    return rc;
  }
  ~StreamCallMem() {
    for (void** p : held) h->mem.release(p);
  }
};

template <int KP>
void stream_launch(const StreamArgs& s, int64_t blocks, int64_t pos, int64_t end, int64_t rows_per_block, hipStream_t st) {
  hipLaunchKernelGGL(stream_kernel<KP>, dim3((unsigned)blocks), dim3(als_threads(KP)), 0, st, s, pos, end, rows_per_block);
}

int stream_launch_kp(int kp, const StreamArgs& s, int64_t blocks, int64_t pos, int64_t end, int64_t rows_per_block, hipStream_t st) {
  switch (kp) {
    case 8: stream_launch<8>(s, blocks, pos, end, rows_per_block, st); break;
    case 16: stream_launch<16>(s, blocks, pos, end, rows_per_block, st); break;
    case 32: stream_launch<32>(s, blocks, pos, end, rows_per_block, st); break;
    case 64: stream_launch<64>(s, blocks, pos, end, rows_per_block, st); break;
    default: return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_stream_rows: no kernel for a factor of leading dimension %d (%s)", kp, STREAM_HEADER);
  }
  HIPCK(hipGetLastError());
  return GLRM_OK;
}

} // namespace

extern "C" int glrm_hip_stream_plan(int64_t m, int64_t n, int64_t first, const int64_t* rowptr, const int32_t* colidx, const int64_t* qptr, const int32_t* qcol,
                                    int32_t sequential, int64_t* level, int64_t* nlevels, int64_t* nlaunches, int64_t* max_width, int64_t* dup_rows) {
  const char* const what = "glrm_hip_stream_plan";
  if (m < 0 || n < 0 || first < 0 || first > m) return fail(GLRM_ERR_INVALID, "%s: first must be in 0 .. m, got m = %lld, n = %lld, first = %lld", what, (long long)m, (long long)n, (long long)first);
  if (!rowptr || (!colidx && rowptr[m] > 0)) return fail(GLRM_ERR_INVALID, "%s: NULL row view", what);
  if ((qptr != nullptr) != (qcol != nullptr)) return fail(GLRM_ERR_INVALID, "%s: qptr and qcol go together (both, or NULL, NULL)", what);
  for (int64_t i = 0; i < m; ++i)
    if (rowptr[i + 1] < rowptr[i] || rowptr[i] < 0) return fail(GLRM_ERR_INVALID, "%s: rowptr does not ascend at row %lld", what, (long long)i);
  for (int64_t e = rowptr[first]; e < rowptr[m]; ++e)
    if (colidx[e] < 0 || colidx[e] >= n) return fail(GLRM_ERR_INVALID, "%s: observation %lld names column %d, outside 0 .. %lld", what, (long long)e, (int)colidx[e], (long long)(n - 1));
  if (qptr)
    if (const int rc = stream_check_queries(what, m, n, qptr, qcol)) return rc;
  StreamPlan p;
  stream_make_plan(m, n, first, rowptr, colidx, 0, qptr, qcol, sequential != 0, p);
  if (level) std::copy(p.level.begin(), p.level.end(), level);
  if (nlevels) *nlevels = p.nlevels;
  if (nlaunches) *nlaunches = p.nlaunches;
  if (max_width) *max_width = p.max_width;
  if (dup_rows) *dup_rows = p.dup_rows;
  return GLRM_OK;
}

extern "C" int glrm_hip_stream_rows(glrm_handle* h, int64_t first, double stepsize, int64_t interval, int32_t sequential, const int64_t* qptr, const int32_t* qcol,
                                    double* qout, double* objective) {
  const char* const what = "glrm_hip_stream_rows";
  int rc = stream_check(h, first, stepsize, interval, qptr, qcol, qout, what);
  if (rc) return rc;
  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  glrm_handle::Stream& ss = h->stream_state;
  const glrm_handle::Side& v = h->side[GLRM_ROWS];
  const int64_t m = h->m, n = h->n, rows = m - first;

  // the plan, from the row view as the handle holds it
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int64_t> ptr;
  if ((rc = glrm_host_ptr(h, GLRM_ROWS, ptr))) return rc;
  const int64_t off = ptr[first], cnt = ptr[m] - off;
  std::vector<int32_t> idx((size_t)std::max<int64_t>(cnt, 1));
  if (cnt > 0) HIPCK(hipMemcpyAsync(idx.data(), v.idx + off, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  StreamPlan p;
  stream_make_plan(m, n, first, ptr.data(), idx.data(), off, qptr, qcol, sequential != 0, p);
  std::vector<int64_t> dupoff((size_t)std::max<int64_t>(rows, 1), -1);
  int64_t nscratch = 0;
  for (int64_t r = 0; r < rows; ++r)
    if (p.dup[r]) {
      dupoff[r] = nscratch;
      nscratch += ptr[first + r + 1] - ptr[first + r];
    }
  const double plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  // device memory: epoch stays with the handle, the rest is this call's
  if (!ss.epoch && (rc = h->mem.alloc(&ss.epoch, (size_t)n))) return rc;
  StreamCallMem mem(h);
  int32_t* order_d = nullptr;
  int64_t *dupoff_d = nullptr, *qptr_d = nullptr;
  int32_t* qcol_d = nullptr;
  double *scratch_d = nullptr, *qout_d = nullptr, *obj_d = nullptr;
  int8_t* status_d = nullptr;
  const int64_t nq = qptr ? qptr[m] : 0;
  if ((rc = mem.alloc(&order_d, (size_t)rows)) || (rc = mem.alloc(&dupoff_d, (size_t)rows)) || (rc = mem.alloc(&scratch_d, (size_t)nscratch)) ||
      (rc = mem.alloc(&obj_d, (size_t)rows)) || (rc = mem.alloc(&status_d, (size_t)rows)))
    return rc;
  if (qptr && ((rc = mem.alloc(&qptr_d, (size_t)m + 1)) || (rc = mem.alloc(&qcol_d, (size_t)nq)) || (rc = mem.alloc(&qout_d, (size_t)nq)))) return rc;
  HIPCK(hipMemsetAsync(ss.epoch, 0, (size_t)std::max<int64_t>(n, 1) * sizeof(int64_t), h->stream));
  if (rows > 0) {
    HIPCK(hipMemcpyAsync(order_d, p.order.data(), (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCK(hipMemcpyAsync(dupoff_d, dupoff.data(), (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  }
  if (qptr) {
    HIPCK(hipMemcpyAsync(qptr_d, qptr, (size_t)(m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    if (nq > 0) HIPCK(hipMemcpyAsync(qcol_d, qcol, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  }

  StreamArgs s{};
  AlsArgs& a = s.g;
  a.ptr = v.ptr; a.idx = v.idx; a.vals = v.vals;
  a.opp = h->side[GLRM_COLS].factor; a.own = v.factor;
  a.losses = h->losses; a.loss_single = h->n_losses == 1;
  a.regs = v.regs; a.reg_single = v.n_regs == 1;
  a.nseg = v.nseg; a.k = h->k; a.side = GLRM_ROWS;
  s.order = order_d; s.dupoff = dupoff_d; s.scratch = scratch_d; s.epoch = ss.epoch;
  s.qptr = qptr_d; s.qcol = qcol_d; s.qout = qout_d;
  s.objective = obj_d; s.status = status_d;
  s.first = first; s.interval = interval; s.base = first / interval;
  s.stepsize = stepsize;
  const double sy = stream_reg_scale(h->side[GLRM_COLS].regs_h[0]);
  s.c = 1.0 + ((2.0 * stepsize) * (double)interval) * sy;

  // the launch loop: a run of one-row levels is a chain (one workgroup, cut into pieces), every other level one workgroup per row
  for (int64_t l = 1; l <= p.nlevels;) {
    const int64_t b = p.lptr[l - 1], w = p.lptr[l] - b;
    if (w > 1) {
      if ((rc = stream_launch_kp(h->kp, s, w, b, b + w, 1, h->stream))) return rc;
      ++l;
      continue;
    }
    int64_t e = l;
    while (e < p.nlevels && p.lptr[e + 1] - p.lptr[e] == 1) ++e;
    const int64_t end = p.lptr[e];
    for (int64_t at = b; at < end; at += STREAM_PIECE)
      if ((rc = stream_launch_kp(h->kp, s, 1, at, std::min(at + STREAM_PIECE, end), STREAM_PIECE, h->stream))) return rc;
    l = e + 1;
  }
  const int64_t total = m / interval - first / interval;
  if (s.c != 1.0 && total > 0 && n > 0) {
    hipLaunchKernelGGL(stream_flush_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->side[GLRM_COLS].factor, ss.epoch, n, h->kp, h->k, s.c, total);
    HIPCK(hipGetLastError());
  }

  ss.status.assign((size_t)std::max<int64_t>(rows, 1), 0);
  if (rows > 0) {
    HIPCK(hipMemcpyAsync(ss.status.data(), status_d, (size_t)rows, hipMemcpyDeviceToHost, h->stream));
    if (objective) HIPCK(hipMemcpyAsync(objective, obj_d, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  if (nq > 0) HIPCK(hipMemcpyAsync(qout, qout_d, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  ss.rows = rows; ss.nlevels = p.nlevels; ss.nlaunches = p.nlaunches; ss.max_width = p.max_width; ss.plan_ms = plan_ms;
  ss.ran = true;
  return GLRM_OK;
}

extern "C" int glrm_hip_stream_info(glrm_handle* h, int64_t* solved, int64_t* kept_short, int64_t* kept_pivot, int64_t* nlevels, int64_t* nlaunches, int64_t* max_width,
                                    double* plan_ms, int8_t* status) {
  if (!h) return fail(GLRM_ERR_INVALID, "glrm_hip_stream_info: NULL handle");
  GLRM_NEED_FINALIZED(h);
  const glrm_handle::Stream& ss = h->stream_state;
  if (!ss.ran) return fail(GLRM_ERR_INVALID, "glrm_hip_stream_info: glrm_hip_stream_rows has not run on this handle");
  int64_t c[3] = {0, 0, 0};
  for (int64_t r = 0; r < ss.rows; ++r) {
    if (ss.status[r] < 0 || ss.status[r] > GLRM_ALS_KEPT_PIVOT) return fail(GLRM_ERR_HIP, "glrm_hip_stream_info: row %lld has status %d", (long long)r, (int)ss.status[r]);
    ++c[ss.status[r]];
  }
  if (status) std::copy(ss.status.begin(), ss.status.begin() + ss.rows, status);
  if (solved) *solved = c[GLRM_ALS_SOLVED];
  if (kept_short) *kept_short = c[GLRM_ALS_KEPT_SHORT];
  if (kept_pivot) *kept_pivot = c[GLRM_ALS_KEPT_PIVOT];
  if (nlevels) *nlevels = ss.nlevels;
  if (nlaunches) *nlaunches = ss.nlaunches;
  if (max_width) *max_width = ss.max_width;
  if (plan_ms) *plan_ms = ss.plan_ms;
  return GLRM_OK;
}
