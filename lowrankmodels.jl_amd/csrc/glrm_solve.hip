// glrm_solve.hip -- the fused row solver of glrm_hip_solve_x (include/glrm_hip_transform.h, glrm_solve.hpp): the double instantiations of
// regcached_solve_kernel and the launch both storages go through.  The entry points and the T launches of the longer rows are
// glrm_hip.hip's; which rows run here is class 0 of a glrm_class_plan (glrm_engine.hpp), built and launched like run_sweep's.
#include <hip/hip_runtime.h>

#include "glrm_solve.hpp"

using namespace glrm;

// `inner` X half-steps of the local rows seglist[0..nlist) -- every one of at most glrm_cached_reg_maxlen(h->G) observations, `cap` trips of
// the lane layout for the longest -- in one launch on `st`.  step: a line-search request for the rows, never ranged.
int glrm_run_solve(glrm_handle* h, const glrm_step& step, const int32_t* seglist, int64_t nlist, int cap, int inner, hipStream_t st) {
  if (nlist <= 0) return GLRM_OK;
  CachedArgs a{};
  glrm_fill_side(a, h, step);
  a.cap = cap;
  a.seg_lo = 0;
  a.seg_hi = h->side[GLRM_ROWS].nseg;
  a.seglist = seglist;
  a.nseg = nlist;
  a.fixed_alpha = 0.0;
  int rc;
  if (h->storage == GLRM_STORAGE_F32) { // the float instantiations live in a unit of their own
    rc = glrm_launch_solve_f32(a, h->G, step.loss, inner, st);
  } else {
    // layouts (4, 8) and (8, 8) only (the predicate of glrm_setup_cached)
    auto by_layout = [&](auto g, auto r) {
      constexpr int G = decltype(g)::value, R = decltype(r)::value;
      auto by_loss = [&](auto LOSS) {
        constexpr int L = decltype(LOSS)::value;
        return a.vecreg ? launch_solve_inst<G, R, L, true>(a, inner, st) : launch_solve_inst<G, R, L, false>(a, inner, st);
      };
      return glrm_dispatch<LOSS_QUAD_UNIFORM, LOSS_SEGMENT, LOSS_SEGMENT_NOTRIG, LOSS_PER_OBS_NOTRIG>(step.loss, by_loss, [&] { return by_loss(glrm_const<LOSS_PER_OBS>{}); });
    };
    rc = glrm_dispatch_layout<32>(h->G, 8, by_layout, [&] { return by_layout(glrm_const<8>{}, glrm_const<8>{}); });
  }
  if (rc) return rc;
  HIPCK(hipGetLastError());
  return GLRM_OK;
}
