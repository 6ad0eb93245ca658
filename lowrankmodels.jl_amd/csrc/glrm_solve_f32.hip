// glrm_solve_f32.hip -- glrm_options.storage = 1 on the fused row solver: the ST = float instantiations of regcached_solve_kernel
// (glrm_solve.hpp; the double ones are glrm_solve.hip's).  VR = false: a float handle refuses vector regularizers.  A unit of its own, as
// glrm_cached_f32.hip is, so that the two sets of kernels compile side by side.

#include <hip/hip_runtime.h>

#include "glrm_solve.hpp"

using namespace glrm;

int glrm_launch_solve_f32(const CachedArgs& a, int G, int loss, int inner, hipStream_t st) {
  // layouts (4, 8) and (8, 8) only (the predicate of glrm_setup_cached)
  auto by_layout = [&](auto g, auto r) {
    constexpr int GG = decltype(g)::value, RR = decltype(r)::value;
    auto by_loss = [&](auto LOSS) { return launch_solve_inst<GG, RR, decltype(LOSS)::value, false, float>(a, inner, st); };
    return glrm_dispatch<LOSS_QUAD_UNIFORM, LOSS_SEGMENT, LOSS_SEGMENT_NOTRIG, LOSS_PER_OBS_NOTRIG>(loss, by_loss, [&] { return by_loss(glrm_const<LOSS_PER_OBS>{}); });
  };
  return glrm_dispatch_layout<32>(G, 8, by_layout, [&] { return by_layout(glrm_const<8>{}, glrm_const<8>{}); });
}
