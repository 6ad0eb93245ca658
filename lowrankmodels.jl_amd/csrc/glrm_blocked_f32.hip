// glrm_blocked_f32.hip -- glrm_options.storage = 1 on the phase-aligned gather passes: the ST = float instantiations of
// tiled_col_pass_kernel<..., L2 = true>, col_reduce_kernel and col_decide_kernel (glrm_tiled.hpp; the double ones are glrm_blocked.hip's and
// glrm_tiled.hip's).  VR = false, line search only: a float handle refuses vector regularizers, the fixed-step entry points, arrival
// blocks and shard ranges; the LDS-tiled and lane forms have no float form.  A unit of its own, so that the second set of pass kernels
// compiles beside the first instead of behind it.

#include <hip/hip_runtime.h>

#include "glrm_blocked.hpp"

using namespace glrm;

int glrm_launch_blocked_f32(glrm_handle* h, int loss, bool grad, const TiledArgs& a, int side, glrm_arrivals* arr, const std::vector<int>& sup_order) { return launch_blocked_st<float>(h, loss, grad, a, side, arr, sup_order); }

void glrm_launch_col_small_f32(int kp, int stage, const TiledArgs& a, hipStream_t st) { launch_col_small_st<float>(kp, stage, a, st); }
