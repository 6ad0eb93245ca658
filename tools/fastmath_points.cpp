// Host build of csrc/glrm_fastmath.hpp on arrays of points, for tests/test_loss_ref.py (the same points the device test uses):
//   g++ -O2 -ffp-contract=off -shared -fPIC tools/fastmath_points.cpp -o libfastmath_points.so
// op: 1 fm_exp, 2 fm_log_ge1, 3 fm_log, 4 fm_rcp, 5 / 6 fm_logistic<true / false>(scale[i], aa[i], x[i]) -- the numbering of glrm_test_loss_pointwise.
#include "../lowrankmodels.jl_amd/csrc/glrm_fastmath.hpp"

extern "C" int fastmath_points(int op, const double* x, const double* scale, const double* aa, long n, double* out, double* dout) {
  if (op < 1 || op > 6) return 1;
  for (long i = 0; i < n; ++i) {
    double L = 0.0, dL = 0.0;
    switch (op) {
      case 1: L = glrm::fm_exp(x[i]); break;
      case 2: L = glrm::fm_log_ge1(x[i]); break;
      case 3: L = glrm::fm_log(x[i]); break;
      case 4: L = glrm::fm_rcp(x[i]); break;
      case 5: glrm::fm_logistic<true>(scale[i], aa[i], x[i], L, dL); break;
      default: glrm::fm_logistic<false>(scale[i], aa[i], x[i], L, dL); break;
    }
    out[i] = L;
    dout[i] = dL;
  }
  return 0;
}
