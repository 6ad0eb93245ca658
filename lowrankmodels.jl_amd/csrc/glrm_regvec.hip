// glrm_regvec.hip -- host side of the regularizers that carry a vector beside their descriptor (include/glrm_hip_regvec.h):
// fixed_latent_features, fixed_last_latent_features (src/regularizers.jl:193-231) and RemQuadReg (:412-423).  The checks, the handle's
// device tables and glrm_hip_set_regularizers_vec; the device code is the VR = true instantiation of csrc/glrm_blockreg.hpp, reached
// through the general sweeps (csrc/glrm_multi.hpp).  The multi-device entry point sits beside its sibling in csrc/glrm_multigpu.hip.
// Part of libglrm_hip.so.
#include <cmath>
#include <new>

#include "glrm_engine.hpp"

namespace {

constexpr int FIXED = GLRM_WRAP_FIXED_FIRST | GLRM_WRAP_FIXED_LAST;

bool side_carries(const glrm_reg* r, int64_t cnt) {
  for (int64_t i = 0; i < cnt; ++i)
    if (glrm_regvec_carries(r[i])) return true;
  return false;
}

const char* carrier_name(const glrm_reg& r) {
  return r.kind == GLRM_REG_REM_QUAD ? "RemQuadReg" : ((r.wrap & GLRM_WRAP_FIXED_FIRST) ? "fixed_latent_features" : "fixed_last_latent_features");
}

// One side's vector-carrying descriptors and their vectors.  losses != nullptr: the side is ry (descriptor i belongs to column
// col_begin + i, one descriptor to all ncols local columns).
int check_side(const char* side, const glrm_reg* r, int64_t cnt, const glrm_regvec* v, int k, const glrm_loss* losses, int64_t n_losses,
               int64_t col_begin, int64_t ncols) {
  const bool any = side_carries(r, cnt);
  if (any && (!v || !v->vec || !v->len))
    return fail(GLRM_ERR_INVALID, "%s holds a descriptor that carries a vector, but its glrm_regvec (or its vec / len) is NULL", side);
  for (int64_t i = 0; i < cnt; ++i) {
    const int kind = r[i].kind, wrap = r[i].wrap;
    const int len = (v && v->len) ? v->len[i] : 0;
    if (!glrm_regvec_carries(r[i])) {
      if (len != 0) return fail(GLRM_ERR_INVALID, "%s[%lld] carries no vector: its length must be 0 (got %d)", side, (long long)i, len);
      continue;
    }
    const char* name = carrier_name(r[i]);
    if (kind == GLRM_REG_REM_QUAD && wrap != 0)
      return fail(GLRM_ERR_UNSUPPORTED, "%s[%lld]: RemQuadReg cannot be combined with a wrapper (wrap = %d), nor be the base of a fixed wrapper", side,
                  (long long)i, wrap);
    if (kind != GLRM_REG_REM_QUAD && wrap != GLRM_WRAP_FIXED_FIRST && wrap != GLRM_WRAP_FIXED_LAST)
      return fail(GLRM_ERR_UNSUPPORTED, "%s[%lld]: a fixed-features wrapper cannot be combined with another wrapper (wrap = %d)", side, (long long)i, wrap);
    if (kind != GLRM_REG_REM_QUAD && (kind < 0 || kind >= GLRM_REG_KIND_END))
      return fail(GLRM_ERR_UNSUPPORTED, "%s[%lld]: regularizer kind %d is not supported as the base of %s", side, (long long)i, kind, name);
    if (losses) {
      const int64_t f0 = cnt == 1 ? col_begin : col_begin + i, f1 = cnt == 1 ? col_begin + ncols : f0 + 1;
      for (int64_t f = f0; f < f1; ++f) {
        const glrm_loss& l = n_losses == 1 ? losses[0] : losses[f];
        if (l.dim > 1)
          return fail(GLRM_ERR_UNSUPPORTED, "%s: %s is a vector regularizer and cannot regularize the %d-column block of column %lld", side, name, l.dim,
                      (long long)f);
        if (n_losses == 1) break;
      }
    }
    if (kind == GLRM_REG_REM_QUAD) {
      if (len != k) return fail(GLRM_ERR_INVALID, "%s[%lld]: RemQuadReg needs a vector of length k = %d (got %d)", side, (long long)i, k, len);
    } else {
      if (len < 1 || len > k) return fail(GLRM_ERR_INVALID, "%s[%lld]: %s fixes nfix = %d entries; nfix must be in 1..%d", side, (long long)i, name, len, k);
      const int sub = k - len; // what the base regularizer sees
      if (kind == GLRM_REG_K_SPARSE && !(r[i].scale >= 1.0 && r[i].scale <= (double)sub && r[i].scale == std::floor(r[i].scale)))
        return fail(GLRM_ERR_INVALID, "%s[%lld]: KSparseConstraint keeps r = %g entries; r must be an integer in 1..%d", side, (long long)i, r[i].scale, sub);
      if (kind == GLRM_REG_QUAD_CONSTRAINT && !(r[i].scale > 0.0 && std::isfinite(r[i].scale)))
        return fail(GLRM_ERR_INVALID, "%s[%lld]: QuadConstraint needs a finite max_2norm > 0 (got %g)", side, (long long)i, r[i].scale);
      if ((kind == GLRM_REG_ONE_SPARSE || kind == GLRM_REG_UNIT_ONE_SPARSE) && sub == 0)
        return fail(GLRM_ERR_INVALID, "%s[%lld]: the base of %s takes the argmax of its vector, which is empty with nfix = k = %d", side, (long long)i, name, k);
    }
    for (int c = 0; c < len; ++c)
      if (!std::isfinite(v->vec[(size_t)i * k + c]))
        return fail(GLRM_ERR_NONFINITE, "%s[%lld]: entry %d of the vector of %s is not finite", side, (long long)i, c, name);
  }
  return GLRM_OK;
}

void to_placeholders(const glrm_reg* r, int64_t cnt, std::vector<glrm_reg>& out) {
  out.assign(r, r + cnt);
  for (glrm_reg& x : out) {
    if (x.kind == GLRM_REG_REM_QUAD) x = glrm_reg{GLRM_REG_ZERO, x.wrap & ~FIXED, 1.0};
    x.wrap &= ~FIXED;
  }
}

bool any_vector_kind(const glrm_reg* r, int64_t cnt) {
  for (int64_t i = 0; i < cnt; ++i)
    if (r[i].kind >= GLRM_REG_QUAD_CONSTRAINT) return true;
  return false;
}

} // namespace

bool glrm_regvec_carries(const glrm_reg& r) { return r.kind == GLRM_REG_REM_QUAD || (r.wrap & FIXED) != 0; }

void glrm_regvec_placeholders(const std::vector<glrm_reg>& in, std::vector<glrm_reg>& out) { to_placeholders(in.data(), (int64_t)in.size(), out); }

void glrm_regvec_drop(glrm_handle* h) {
  for (int s = 0; s < 2; ++s) {
    h->mem.release(&h->side[s].regvec);
    h->mem.release(&h->side[s].reglen);
    h->side[s].regvec_h.clear();
    h->side[s].reglen_h.clear();
  }
}

int glrm_check_regularizers_vec(const glrm_handle* h, const glrm_reg* rx, int64_t n_rx, const glrm_regvec* vx, const glrm_reg* ry, int64_t n_ry,
                                const glrm_regvec* vy) {
  if (!h || !rx || !ry) return fail(GLRM_ERR_INVALID, "NULL argument");
  if (n_rx != h->side[GLRM_ROWS].n_regs || n_ry != h->side[GLRM_COLS].n_regs)
    return fail(GLRM_ERR_INVALID, "regularizer counts must match the handle (rx %lld, ry %lld)", (long long)h->side[GLRM_ROWS].n_regs, (long long)h->side[GLRM_COLS].n_regs);
  if (side_carries(rx, n_rx) || side_carries(ry, n_ry) || vx || vy) { // the handle moves to (or stays on) the general sweeps
    if (h->storage == GLRM_STORAGE_F32)
      return fail(GLRM_ERR_UNSUPPORTED, "regularizers that carry a vector are not available with storage = f32 (glrm_options.storage = 1): they run on the general sweeps, which read fp64 factors");
    if (h->sum_order_opt)
      return fail(GLRM_ERR_UNSUPPORTED, "regularizers that carry a vector are not available in reference-order mode (glrm_options.sum_order = 1): they run on the general sweeps");
    if (h->dense || h->kp > 64)
      return fail(GLRM_ERR_UNSUPPORTED, "regularizers that carry a vector need a sparse-view handle with k <= 64 (like the wrapped regularizers)");
  }
  if (const int rc = check_side("rx", rx, n_rx, vx, h->k, nullptr, 0, 0, 0)) return rc;
  if (const int rc = check_side("ry", ry, n_ry, vy, h->k, h->losses_h.data(), (int64_t)h->losses_h.size(), h->side[GLRM_COLS].begin, h->side[GLRM_COLS].nseg)) return rc;
  try { // the descriptors that carry no vector: everything glrm_hip_set_regularizers refuses
    std::vector<glrm_reg> px, py;
    to_placeholders(rx, n_rx, px);
    to_placeholders(ry, n_ry, py);
    for (int64_t i = 0; i < n_rx; ++i) if (glrm_regvec_carries(rx[i])) px[(size_t)i] = glrm_reg{GLRM_REG_ZERO, 0, 1.0};
    for (int64_t i = 0; i < n_ry; ++i) if (glrm_regvec_carries(ry[i])) py[(size_t)i] = glrm_reg{GLRM_REG_ZERO, 0, 1.0};
    return glrm_check_regularizers(h, px.data(), n_rx, py.data(), n_ry);
  } catch (const std::bad_alloc&) {
    return fail(GLRM_ERR_OOM, "out of host memory");
  }
}

extern "C" int glrm_hip_set_regularizers_vec(glrm_handle* h, const glrm_reg* rx, int64_t n_rx, const glrm_regvec* vx, const glrm_reg* ry,
                                             int64_t n_ry, const glrm_regvec* vy) {
  if (const int rc = glrm_check_regularizers_vec(h, rx, n_rx, vx, ry, n_ry, vy)) return rc;
  const glrm_reg* r[2] = {rx, ry};
  const int64_t cnt[2] = {n_rx, n_ry};
  const glrm_regvec* v[2] = {vx, vy};
  const bool carries[2] = {side_carries(rx, n_rx), side_carries(ry, n_ry)};
  // Neither a vector-carrying descriptor nor a table: the plain call (it drops the tables of an earlier call).  A table whose lengths are
  // all 0 still moves the handle to the general sweeps: how the shards of one problem stay on ONE family when only some hold a vector.
  if (!carries[0] && !carries[1] && !vx && !vy) return glrm_hip_set_regularizers(h, rx, n_rx, ry, n_ry);
  DeviceScope dg(h->device);
  if (!h->multi && h->finalized && !h->sum_order_opt) // the handle moves to the general sweeps: the part of set-up it still needs (nothing has changed yet)
    if (const int rc = glrm_setup_multi_split(h)) return rc;
  const int k = h->k;
  std::vector<double> tv[2];
  std::vector<int32_t> tl[2];
  std::vector<glrm_reg> nr[2];
  try {
    for (int s = 0; s < 2; ++s) {
      nr[s].assign(r[s], r[s] + cnt[s]);
      if (!carries[s]) continue;
      tv[s].assign((size_t)cnt[s] * k, 0.0);
      tl[s].assign(v[s]->len, v[s]->len + cnt[s]);
      for (int64_t i = 0; i < cnt[s]; ++i)
        for (int c = 0; c < tl[s][(size_t)i]; ++c) tv[s][(size_t)i * k + c] = v[s]->vec[(size_t)i * k + c];
    }
  } catch (const std::bad_alloc&) {
    return fail(GLRM_ERR_OOM, "out of host memory for the regularizer vectors");
  }
  // the new device tables first, in an arena of their own: until they are complete the handle is untouched
  DevArena fresh;
  double* dv[2] = {nullptr, nullptr};
  int32_t* dl[2] = {nullptr, nullptr};
  hipError_t e = hipSuccess;
  for (int s = 0; s < 2 && e == hipSuccess; ++s) {
    if (!carries[s]) continue;
    if (const int rc = fresh.alloc(&dv[s], tv[s].size())) return rc;
    if (const int rc = fresh.alloc(&dl[s], tl[s].size())) return rc;
    e = hipMemcpyAsync(dv[s], tv[s].data(), tv[s].size() * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dl[s], tl[s].data(), tl[s].size() * 4, hipMemcpyHostToDevice, h->stream);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h->side[GLRM_ROWS].regs, rx, (size_t)n_rx * sizeof(glrm_reg), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->side[GLRM_COLS].regs, ry, (size_t)n_ry * sizeof(glrm_reg), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(GLRM_ERR_HIP, "installing the regularizer vectors failed: %s", hipGetErrorString(e));
  glrm_regvec_drop(h); // the previous call's tables (the stream is idle)
  for (int s = 0; s < 2; ++s) {
    h->side[s].regvec = dv[s];
    h->side[s].reglen = dl[s];
    fresh.move_to(h->mem, dv[s]);
    fresh.move_to(h->mem, dl[s]);
    h->side[s].regvec_h.swap(tv[s]);
    h->side[s].reglen_h.swap(tl[s]);
  }
  for (int s = 0; s < 2; ++s) h->side[s].regs_h.swap(nr[s]);
  h->multi = true; // checked above: this handle can run the general sweeps
  h->side[GLRM_ROWS].vecreg = carries[0] || any_vector_kind(rx, n_rx);
  h->side[GLRM_COLS].vecreg = carries[1] || any_vector_kind(ry, n_ry);
  if (h->iter_exec) { // a captured iteration holds the launches of the other family and the old table pointers
    (void)hipGraphExecDestroy(h->iter_exec);
    h->iter_exec = nullptr;
  }
  return GLRM_OK;
}

// glrm_hip_subset: the child was created from the parent's descriptors with the vector codes taken out; it now gets the parent's
// descriptors and vectors (a subset keeps m, n and the shard's ranges, so the tables carry over unchanged).
int glrm_regvec_inherit(glrm_handle* child, const glrm_handle* parent) {
  const glrm_handle::Side &rows = parent->side[GLRM_ROWS], &cols = parent->side[GLRM_COLS];
  if (!rows.regvec && !cols.regvec) return GLRM_OK;
  const glrm_regvec vx{rows.regvec_h.data(), rows.reglen_h.data()}, vy{cols.regvec_h.data(), cols.reglen_h.data()};
  return glrm_hip_set_regularizers_vec(child, rows.regs_h.data(), (int64_t)rows.regs_h.size(), rows.regvec ? &vx : nullptr, cols.regs_h.data(),
                                       (int64_t)cols.regs_h.size(), cols.regvec ? &vy : nullptr);
}
