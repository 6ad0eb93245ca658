// glrm_cd.hip -- include/glrm_hip_cd.h: glrm_hip_cd_solve, cyclic coordinate-descent sweeps on every row or column of a QuadLoss model
// whose solved side carries ZeroReg, QuadReg, OneReg or NonNegConstraint, and glrm_hip_cd_info.  The header is the specification of the
// arithmetic; the kernel is glrm_cd.hpp over the Gram stage of glrm_als.hpp.  This unit holds the refusals (in the order of als_check,
// glrm_als.hip), the per-side state of the handle (glrm_handle::cd: the longest-first order of the segments, built at the side's first
// solve, the status bits and the sweeps run of every segment) and the launch.
#include <cmath>

#include "glrm_cd.hpp"

using namespace glrm;

namespace {

const char* const CD_HEADER = "include/glrm_hip_cd.h";

bool cd_kind(int32_t kind) { return kind == GLRM_REG_ZERO || kind == GLRM_REG_QUAD || kind == GLRM_REG_ONE || kind == GLRM_REG_NONNEG; }

// everything glrm_hip_cd_solve refuses, nothing touched
int cd_check(glrm_handle* h, int32_t side, int32_t sweeps, const char* what) {
  if (!h) return fail(GLRM_ERR_INVALID, "%s: NULL handle", what);
  if (side != GLRM_ROWS && side != GLRM_COLS) return fail(GLRM_ERR_INVALID, "%s: side must be 0 (rows of X) or 1 (columns of Y), got %d", what, (int)side);
  GLRM_NEED_FINALIZED(h);
  if (h->storage == GLRM_STORAGE_F32)
    return fail(GLRM_ERR_UNSUPPORTED, "%s is not available with storage = f32 (glrm_options.storage = 1): the solve reads fp64 lists and factors (%s)", what, CD_HEADER);
  if (h->dense) return fail(GLRM_ERR_UNSUPPORTED, "%s works on the observation lists: this handle was created from dense_A (%s)", what, CD_HEADER);
  if (!glrm_single_shard(h))
    return fail(GLRM_ERR_UNSUPPORTED, "%s needs the whole problem on one handle: this one is a shard (rows [%lld, %lld) of %lld, columns [%lld, %lld) of %lld; %s)", what,
                (long long)h->side[GLRM_ROWS].begin, (long long)h->side[GLRM_ROWS].end, (long long)h->m, (long long)h->side[GLRM_COLS].begin,
                (long long)h->side[GLRM_COLS].end, (long long)h->n, CD_HEADER);
  if (h->k > GLRM_CD_MAX_K) return fail(GLRM_ERR_UNSUPPORTED, "%s: rank k = %d is above GLRM_CD_MAX_K = %d (%s)", what, h->k, GLRM_CD_MAX_K, CD_HEADER);
  for (size_t j = 0; j < h->losses_h.size(); ++j)
    if (h->losses_h[j].kind != GLRM_LOSS_QUAD)
      return fail(GLRM_ERR_UNSUPPORTED, "%s: column %lld has loss kind %d; the coordinate update needs QuadLoss (kind %d) on every column (%s)", what, (long long)j,
                  h->losses_h[j].kind, (int)GLRM_LOSS_QUAD, CD_HEADER);
  const glrm_handle::Side& v = h->side[side];
  const char* const name = side == GLRM_ROWS ? "rx" : "ry";
  for (size_t s = 0; s < v.regs_h.size(); ++s) {
    const glrm_reg& r = v.regs_h[s];
    if (!cd_kind(r.kind) || r.wrap != 0)
      return fail(GLRM_ERR_UNSUPPORTED, "%s: %s[%lld] has regularizer kind %d, wrap %d; the solved side needs a plain ZeroReg (kind %d), QuadReg (kind %d), OneReg (kind %d) or "
                  "NonNegConstraint (kind %d) (%s)", what, name, (long long)s, r.kind, r.wrap, (int)GLRM_REG_ZERO, (int)GLRM_REG_QUAD, (int)GLRM_REG_ONE, (int)GLRM_REG_NONNEG,
                  CD_HEADER);
    if ((r.kind == GLRM_REG_QUAD || r.kind == GLRM_REG_ONE) && !(r.scale >= 0.0))
      return fail(GLRM_ERR_UNSUPPORTED, "%s: %s[%lld] is %s with scale %g; the coordinate update needs a scale >= 0 (%s)", what, name, (long long)s,
                  r.kind == GLRM_REG_QUAD ? "QuadReg" : "OneReg", r.scale, CD_HEADER);
  }
  if (v.regvec)
    return fail(GLRM_ERR_UNSUPPORTED, "%s: the %s carry a vector (glrm_hip_set_regularizers_vec); the solved side needs a plain ZeroReg, QuadReg, OneReg or NonNegConstraint (%s)", what,
                name, CD_HEADER);
  if (h->multi || h->d != h->n)
    return fail(GLRM_ERR_UNSUPPORTED, "%s: the model runs on the general sweeps (multi-dimensional losses, wrapped or vector regularizers); coordinate descent does not (%s)", what,
                CD_HEADER);
  if (!h->side[GLRM_ROWS].factor || !h->side[GLRM_COLS].factor)
    return fail(GLRM_ERR_INVALID, "%s: no factors on the device yet (fit, glrm_hip_set_factors or glrm_hip_bind_buffers first)", what);
  if (sweeps < 1 || sweeps > GLRM_CD_MAX_SWEEPS)
    return fail(GLRM_ERR_INVALID, "%s: sweeps must be in [1, GLRM_CD_MAX_SWEEPS = %d], got %d", what, GLRM_CD_MAX_SWEEPS, (int)sweeps);
  return GLRM_OK;
}

// the side's state, made once: segments longest first (stable), one status byte and one sweep count per segment
int cd_prepare(glrm_handle* h, int side) {
  glrm_handle::Cd& s = h->cd[side];
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
  if ((rc = h->mem.alloc(&s.sweeps_run, (size_t)h->side[side].nseg))) {
    h->mem.release(&s.status);
    h->mem.release(&order_d);
    return rc;
  }
  s.order = order_d;
  return GLRM_OK;
}

template <int KP>
void cd_launch(const CdArgs& c, hipStream_t st) {
  hipLaunchKernelGGL(cd_solve_kernel<KP>, dim3((unsigned)c.g.nseg), dim3(als_threads(KP)), 0, st, c);
}

} // namespace

extern "C" int glrm_hip_cd_solve(glrm_handle* h, int32_t side, int32_t sweeps) {
  int rc = cd_check(h, side, sweeps, "glrm_hip_cd_solve");
  if (rc) return rc;
  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  const glrm_handle::Side& v = h->side[side];
  if ((rc = cd_prepare(h, side))) return rc;
  if (v.nseg > 0) {
    CdArgs c{};
    AlsArgs& a = c.g;
    a.ptr = v.ptr; a.idx = v.idx; a.vals = v.vals;
    a.opp = h->side[side ^ 1].factor; a.own = v.factor;
    a.losses = h->losses; a.loss_single = h->n_losses == 1;
    a.regs = v.regs; a.reg_single = v.n_regs == 1;
    a.order = h->cd[side].order; a.status = h->cd[side].status;
    a.nseg = v.nseg; a.k = h->k; a.side = side;
    c.sweeps_run = h->cd[side].sweeps_run; c.sweeps = sweeps;
    switch (h->kp) {
      case 8: cd_launch<8>(c, h->stream); break;
      case 16: cd_launch<16>(c, h->stream); break;
      case 32: cd_launch<32>(c, h->stream); break;
      case 64: cd_launch<64>(c, h->stream); break;
      default: return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_cd_solve: no kernel for a factor of leading dimension %d (%s)", h->kp, CD_HEADER);
    }
    HIPCK(hipGetLastError());
  }
  h->cd[side].solved = true;
  return GLRM_OK;
}

extern "C" int glrm_hip_cd_info(glrm_handle* h, int32_t side, int64_t* converged, int64_t* skipped, int64_t* sweeps_total, int8_t* status, int32_t* sweeps_run) {
  if (!h) return fail(GLRM_ERR_INVALID, "glrm_hip_cd_info: NULL handle");
  if (side != GLRM_ROWS && side != GLRM_COLS) return fail(GLRM_ERR_INVALID, "glrm_hip_cd_info: side must be 0 (rows of X) or 1 (columns of Y), got %d", (int)side);
  GLRM_NEED_FINALIZED(h);
  if (!h->cd[side].solved) return fail(GLRM_ERR_INVALID, "glrm_hip_cd_info: glrm_hip_cd_solve has not run on side %d of this handle", (int)side);
  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  const int64_t nseg = h->side[side].nseg;
  std::vector<int8_t> own;
  std::vector<int32_t> own_run;
  if (!status) { own.resize((size_t)std::max<int64_t>(nseg, 1)); status = own.data(); }
  if (!sweeps_run) { own_run.resize((size_t)std::max<int64_t>(nseg, 1)); sweeps_run = own_run.data(); }
  if (nseg > 0) {
    HIPCK(hipMemcpyAsync(status, h->cd[side].status, (size_t)nseg, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipMemcpyAsync(sweeps_run, h->cd[side].sweeps_run, (size_t)nseg * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCK(hipStreamSynchronize(h->stream));
  int64_t nc = 0, ns = 0, total = 0;
  for (int64_t s = 0; s < nseg; ++s) {
    if (status[s] < 0 || status[s] > (GLRM_CD_CONVERGED | GLRM_CD_SKIPPED) || sweeps_run[s] < 1 || sweeps_run[s] > GLRM_CD_MAX_SWEEPS)
      return fail(GLRM_ERR_HIP, "glrm_hip_cd_info: segment %lld has status %d after %d sweeps", (long long)s, (int)status[s], (int)sweeps_run[s]);
    nc += (status[s] & GLRM_CD_CONVERGED) != 0;
    ns += (status[s] & GLRM_CD_SKIPPED) != 0;
    total += sweeps_run[s];
  }
  if (converged) *converged = nc;
  if (skipped) *skipped = ns;
  if (sweeps_total) *sweeps_total = total;
  return GLRM_OK;
}
