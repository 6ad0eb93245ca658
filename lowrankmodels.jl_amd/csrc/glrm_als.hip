// glrm_als.hip -- include/glrm_hip_als.h: glrm_hip_als_solve, the exact half-step of a QuadLoss + QuadReg / ZeroReg model, and
// glrm_hip_als_info.  The header is the specification of the arithmetic; the kernel is glrm_als.hpp.  This unit holds the refusals, the
// per-side state of the handle (glrm_handle::als: the longest-first order of the segments, built at the side's first solve, and the
// status of every segment) and the launch.
#include <cmath>

#include "glrm_als.hpp"

using namespace glrm;

namespace {

const char* const ALS_HEADER = "include/glrm_hip_als.h";

// everything glrm_hip_als_solve refuses, nothing touched
int als_check(glrm_handle* h, int32_t side, const char* what) {
  if (!h) return fail(GLRM_ERR_INVALID, "%s: NULL handle", what);
  if (side != GLRM_ROWS && side != GLRM_COLS) return fail(GLRM_ERR_INVALID, "%s: side must be 0 (rows of X) or 1 (columns of Y), got %d", what, (int)side);
  GLRM_NEED_FINALIZED(h);
  if (h->storage == GLRM_STORAGE_F32)
    return fail(GLRM_ERR_UNSUPPORTED, "%s is not available with storage = f32 (glrm_options.storage = 1): the solve reads fp64 lists and factors (%s)", what, ALS_HEADER);
  if (h->dense) return fail(GLRM_ERR_UNSUPPORTED, "%s works on the observation lists: this handle was created from dense_A (%s)", what, ALS_HEADER);
  if (!glrm_single_shard(h))
    return fail(GLRM_ERR_UNSUPPORTED, "%s needs the whole problem on one handle: this one is a shard (rows [%lld, %lld) of %lld, columns [%lld, %lld) of %lld; %s)", what,
                (long long)h->side[GLRM_ROWS].begin, (long long)h->side[GLRM_ROWS].end, (long long)h->m, (long long)h->side[GLRM_COLS].begin,
                (long long)h->side[GLRM_COLS].end, (long long)h->n, ALS_HEADER);
  if (h->k > GLRM_ALS_MAX_K) return fail(GLRM_ERR_UNSUPPORTED, "%s: rank k = %d is above GLRM_ALS_MAX_K = %d (%s)", what, h->k, GLRM_ALS_MAX_K, ALS_HEADER);
  for (size_t j = 0; j < h->losses_h.size(); ++j)
    if (h->losses_h[j].kind != GLRM_LOSS_QUAD)
      return fail(GLRM_ERR_UNSUPPORTED, "%s: column %lld has loss kind %d; the closed-form solve needs QuadLoss (kind %d) on every column (%s)", what, (long long)j,
                  h->losses_h[j].kind, (int)GLRM_LOSS_QUAD, ALS_HEADER);
  const glrm_handle::Side& v = h->side[side];
  const char* const name = side == GLRM_ROWS ? "rx" : "ry";
  for (size_t s = 0; s < v.regs_h.size(); ++s) {
    const glrm_reg& r = v.regs_h[s];
    if ((r.kind != GLRM_REG_QUAD && r.kind != GLRM_REG_ZERO) || r.wrap != 0)
      return fail(GLRM_ERR_UNSUPPORTED, "%s: %s[%lld] has regularizer kind %d, wrap %d; the solved side needs a plain QuadReg (kind %d) or ZeroReg (kind %d) (%s)", what, name,
                  (long long)s, r.kind, r.wrap, (int)GLRM_REG_QUAD, (int)GLRM_REG_ZERO, ALS_HEADER);
    if (r.kind == GLRM_REG_QUAD && !(r.scale >= 0.0))
      return fail(GLRM_ERR_UNSUPPORTED, "%s: %s[%lld] is QuadReg with scale %g; the system needs a scale >= 0 (%s)", what, name, (long long)s, r.scale, ALS_HEADER);
  }
  if (v.regvec) return fail(GLRM_ERR_UNSUPPORTED, "%s: the %s carry a vector (glrm_hip_set_regularizers_vec); the solved side needs a plain QuadReg or ZeroReg (%s)", what, name, ALS_HEADER);
  if (h->multi || h->d != h->n)
    return fail(GLRM_ERR_UNSUPPORTED, "%s: the model runs on the general sweeps (multi-dimensional losses, wrapped or vector regularizers); the closed-form solve does not (%s)", what, ALS_HEADER);
  if (!h->side[GLRM_ROWS].factor || !h->side[GLRM_COLS].factor)
    return fail(GLRM_ERR_INVALID, "%s: no factors on the device yet (fit, glrm_hip_set_factors or glrm_hip_bind_buffers first)", what);
  return GLRM_OK;
}

// the side's state, made once: segments longest first (stable), one status byte per segment
int als_prepare(glrm_handle* h, int side) {
  glrm_handle::Als& s = h->als[side];
  if (s.order) return GLRM_OK;
  std::vector<int64_t> ptr;
  int rc = glrm_host_ptr(h, side, ptr);
  if (rc) return rc;
  std::vector<int32_t> order, none;
  glrm_split_by_length(ptr, 0, order, none);
  int32_t* order_d = nullptr;
  if ((rc = glrm_upload_list(h, order, &order_d))) return rc;
  if ((rc = h->mem.alloc(&s.status, (size_t)h->side[side].nseg))) {
    h->mem.release(&order_d);
    return rc;
  }
  s.order = order_d;
  return GLRM_OK;
}

template <int KP>
void als_launch(const AlsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(als_solve_kernel<KP>, dim3((unsigned)a.nseg), dim3(als_threads(KP)), 0, st, a);
}

} // namespace

extern "C" int glrm_hip_als_solve(glrm_handle* h, int32_t side) {
  int rc = als_check(h, side, "glrm_hip_als_solve");
  if (rc) return rc;
  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  const glrm_handle::Side& v = h->side[side];
  if ((rc = als_prepare(h, side))) return rc;
  if (v.nseg > 0) {
    AlsArgs a{};
    a.ptr = v.ptr; a.idx = v.idx; a.vals = v.vals;
    a.opp = h->side[side ^ 1].factor; a.own = v.factor;
    a.losses = h->losses; a.loss_single = h->n_losses == 1;
    a.regs = v.regs; a.reg_single = v.n_regs == 1;
    a.order = h->als[side].order; a.status = h->als[side].status;
    a.nseg = v.nseg; a.k = h->k; a.side = side;
    switch (h->kp) {
      case 8: als_launch<8>(a, h->stream); break;
      case 16: als_launch<16>(a, h->stream); break;
      case 32: als_launch<32>(a, h->stream); break;
      case 64: als_launch<64>(a, h->stream); break;
      default: return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_als_solve: no kernel for a factor of leading dimension %d (%s)", h->kp, ALS_HEADER);
    }
    HIPCK(hipGetLastError());
  }
  h->als[side].solved = true;
  return GLRM_OK;
}

extern "C" int glrm_hip_als_info(glrm_handle* h, int32_t side, int64_t* solved, int64_t* kept_short, int64_t* kept_pivot, int8_t* status) {
  if (!h) return fail(GLRM_ERR_INVALID, "glrm_hip_als_info: NULL handle");
  if (side != GLRM_ROWS && side != GLRM_COLS) return fail(GLRM_ERR_INVALID, "glrm_hip_als_info: side must be 0 (rows of X) or 1 (columns of Y), got %d", (int)side);
  GLRM_NEED_FINALIZED(h);
  if (!h->als[side].solved) return fail(GLRM_ERR_INVALID, "glrm_hip_als_info: glrm_hip_als_solve has not run on side %d of this handle", (int)side);
  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  const int64_t nseg = h->side[side].nseg;
  std::vector<int8_t> own;
  if (!status) { own.resize((size_t)std::max<int64_t>(nseg, 1)); status = own.data(); }
  if (nseg > 0) HIPCK(hipMemcpyAsync(status, h->als[side].status, (size_t)nseg, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  int64_t n[3] = {0, 0, 0};
  for (int64_t s = 0; s < nseg; ++s) {
    if (status[s] < 0 || status[s] > GLRM_ALS_KEPT_PIVOT) return fail(GLRM_ERR_HIP, "glrm_hip_als_info: segment %lld has status %d", (long long)s, (int)status[s]);
    ++n[status[s]];
  }
  if (solved) *solved = n[GLRM_ALS_SOLVED];
  if (kept_short) *kept_short = n[GLRM_ALS_KEPT_SHORT];
  if (kept_pivot) *kept_pivot = n[GLRM_ALS_KEPT_PIVOT];
  return GLRM_OK;
}
