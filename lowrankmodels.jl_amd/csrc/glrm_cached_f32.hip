// glrm_cached_f32.hip -- glrm_options.storage = 1 on the cached row sweep: the ST = float instantiations of the register variant
// (glrm_cached.hpp; the double ones are glrm_cached.hip's).  Two waves per row, VR = false, line search only: a float handle refuses
// vector regularizers and glrm_hip_fit_sparse, and the 1- / 4-wave experiment kernels and the LDS variant have no float form.  A unit of
// its own, so that a second set of kernels of this size compiles beside the first instead of behind it.

#include <hip/hip_runtime.h>

#include "glrm_cached.hpp"

using namespace glrm;

int glrm_launch_cached_f32(const CachedArgs& a, int G, int loss, hipStream_t st, glrm_handle* h) {
  // layouts (4, 8) and (8, 8) only (glrm_setup_cached)
  auto by_layout = [&](auto g, auto r) {
    constexpr int GG = decltype(g)::value, RR = decltype(r)::value;
    auto by_loss = [&](auto LOSS) { return launch_reg_inst<GG, RR, decltype(LOSS)::value, false, float>(a, st, h); };
    return glrm_dispatch<LOSS_QUAD_UNIFORM, LOSS_SEGMENT, LOSS_SEGMENT_NOTRIG, LOSS_PER_OBS_NOTRIG>(loss, by_loss, [&] { return by_loss(glrm_const<LOSS_PER_OBS>{}); });
  };
  return glrm_dispatch_layout<32>(G, 8, by_layout, [&] { return by_layout(glrm_const<8>{}, glrm_const<8>{}); });
}
