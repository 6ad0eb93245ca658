// glrm_testhooks.hip -- the engine's test hooks in ONE place, compiled twice (lowrankmodels.jl_amd/build.py):
//   libglrm_hip.so           the product library: every hook is a constant -- no environment variable can inject a failure, point the engine at
//                            another RCCL, or switch the link emulator on (these were env-gated code in the production library)
//   libglrm_hip_testing.so   the same objects with this file and csrc/glrm_multigpu.hip rebuilt under -DGLRM_HIP_TESTING: GLRM_HIP_TEST_FAIL_FINALIZE,
//                            GLRM_HIP_RCCL_LIB / GLRM_HIP_RCCL_ALLOW_SHARED (tests/stubs/rccl_stub.cpp) and the link emulator
//                            (GLRM_EXCHANGE_EMULATE_*) exist only there; tests and `bench.py --emulate-link-gbps` load it by name.
#include <atomic>
#include <cstdlib>

#include "glrm_engine.hpp"

// (not part of the C ABI of include/glrm_hip.h: how a test tells the two builds apart)
extern "C" int glrm_build_is_testing(void) {
#ifdef GLRM_HIP_TESTING
  return 1;
#else
  return 0;
#endif
}

int glrm_test_fail_finalize() {
#ifdef GLRM_HIP_TESTING
  return knob(Knob::TEST_FAIL_FINALIZE) != 0;
#else
  return 0;
#endif
}

// ------------------------------------------------------------------ DevArena's allocator (csrc/glrm_devmem.hpp): the engine's only hipMalloc / hipFree.
// The test build counts the live allocations (tests/test_gpu_devmem.py: every handle and every extension call gives back what it took).
#ifdef GLRM_HIP_TESTING
static std::atomic<long long> g_live_allocations{0};
#endif

hipError_t glrm_device_alloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
#ifdef GLRM_HIP_TESTING
  if (e == hipSuccess) ++g_live_allocations;
#endif
  return e;
}

void glrm_device_free(void* p) {
  if (!p) return;
  (void)hipFree(p);
#ifdef GLRM_HIP_TESTING
  --g_live_allocations;
#endif
}

// live device allocations of this library's arenas; -1 in the product library, which does not count
extern "C" long long glrm_test_live_device_allocations(void) {
#ifdef GLRM_HIP_TESTING
  return g_live_allocations.load();
#else
  return -1;
#endif
}

#ifdef GLRM_HIP_TESTING
// ------------------------------------------------------------------ regularizer hook (tests/test_gpu_regularizers_extra.py)
// prox!(r, u, alpha) and evaluate(r, .) of the input and of the result on a batch of host vectors, through ONE of the code paths a fit
// can take: a lane layout (G, R) of the sweep families (csrc/glrm_device.hpp), the reference-order path (csrc/glrm_refreg.hpp) or the
// general sweeps' vector path (csrc/glrm_blockreg.hpp, the only one that knows the wrappers).
#include <vector>

#include "glrm_blockreg.hpp"
#include "glrm_launch.hpp"
#include "glrm_refreg.hpp"

namespace {
using namespace glrm;

struct RegHookArgs {
  glrm_reg reg;
  int k, kp;
  double alpha;
  int64_t nvec;
  double* vec; // nvec x kp, zero padded, replaced by the prox
  double* ein; // evaluate(r, u)
  double* eout; // evaluate(r, prox(r, u, alpha))
};

template <int G, int R>
__global__ void __launch_bounds__(64) reg_hook_layout(const RegHookArgs a) {
  const int lane = threadIdx.x, j = lane % G;
  const int64_t v = (int64_t)blockIdx.x * (64 / G) + lane / G;
  if (v >= a.nvec) return; // a whole group leaves
  const RegDesc rd{a.reg.kind, a.reg.scale};
  double2* p = reinterpret_cast<double2*>(a.vec + v * (G * R));
  Vec<G, R> u;
#pragma unroll
  for (int i = 0; i < R / 2; ++i) u.v[i] = p[i * G + j];
  const double e0 = reg_eval<G, R, true>(rd, u, j, a.k);
  reg_prox<G, R, true>(rd, u, a.alpha, j, a.k);
  const double e1 = reg_eval<G, R, true>(rd, u, j, a.k);
#pragma unroll
  for (int i = 0; i < R / 2; ++i) p[i * G + j] = u.v[i];
  if (j == 0) { a.ein[v] = e0; a.eout[v] = e1; }
}

template <int KP>
__global__ void __launch_bounds__(64) reg_hook_ref(const RegHookArgs a) {
  const int64_t v = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (v >= a.nvec) return;
  const RegDesc rd{a.reg.kind, a.reg.scale};
  double u[KP];
#pragma unroll
  for (int c = 0; c < KP; ++c) u[c] = a.vec[v * KP + c];
  a.ein[v] = ref_reg_eval<KP, true>(rd, u, a.k);
  ref_reg_prox<KP, true>(rd, u, a.k, a.alpha);
  a.eout[v] = ref_reg_eval<KP, true>(rd, u, a.k);
#pragma unroll
  for (int c = 0; c < KP; ++c) a.vec[v * KP + c] = u[c];
}

// one wave per vector, the k x 1 block in LDS with the general sweeps' stride
__global__ void __launch_bounds__(64) reg_hook_block(const RegHookArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, S = a.kp + 1;
  double* blk = sm;
  double* tmp = sm + S;
  double* red = tmp + S;
  double* g = a.vec + (int64_t)blockIdx.x * a.kp;
  for (int c = tid; c < a.kp; c += 64) blk[c] = g[c];
  __syncthreads();
  const double e0 = block_reg_eval<1, true>(blk, S, a.k, 1, a.reg, red);
  block_prox<1, true>(blk, S, a.k, 1, a.reg, a.alpha, tmp);
  const double e1 = block_reg_eval<1, true>(blk, S, a.k, 1, a.reg, red);
  for (int c = tid; c < a.kp; c += 64) g[c] = blk[c];
  if (tid == 0) { a.ein[blockIdx.x] = e0; a.eout[blockIdx.x] = e1; }
}

int reg_hook_launch(int path, int G, int R, const RegHookArgs& a) {
  if (path == 0) {
    const unsigned grid = (unsigned)((a.nvec * G + 63) / 64);
    auto go = [&](auto g, auto r) {
      hipLaunchKernelGGL((reg_hook_layout<decltype(g)::value, decltype(r)::value>), dim3(grid), dim3(64), 0, 0, a);
      return GLRM_OK;
    };
    if (G == 2 && R == 16) return go(glrm_const<2>{}, glrm_const<16>{}); // the lane-per-segment form at kp = 32
    return glrm_dispatch_layout<8, 16, 32, 64, 128>(G, R, go, [&] { return fail(GLRM_ERR_INVALID, "no lane layout (%d, %d)", G, R); });
  }
  if (path == 1)
    return glrm_dispatch<8, 16, 32, 64>(
        a.kp,
        [&](auto KP) {
          hipLaunchKernelGGL((reg_hook_ref<decltype(KP)::value>), dim3((unsigned)((a.nvec + 63) / 64)), dim3(64), 0, 0, a);
          return GLRM_OK;
        },
        [&] { return fail(GLRM_ERR_INVALID, "no reference-order kernel for a padded rank of %d", a.kp); });
  hipLaunchKernelGGL(reg_hook_block, dim3((unsigned)a.nvec), dim3(64), (size_t)(2 * (a.kp + 1) + 16) * 8, 0, a);
  return GLRM_OK;
}
} // namespace

// path: 0 = lane layout (G, R), kp = G R; 1 = reference order, kp = G R in {8, 16, 32, 64}; 2 = general sweeps, kp = G R <= 64 (G, R only give kp).
// u: nvec x k (host), prox_out: nvec x kp (host, the padded vectors as the kernels leave them), eval_in / eval_out: nvec.
extern "C" int glrm_test_reg_prox_eval(const glrm_reg* reg, int32_t k, double alpha, int32_t path, int32_t G, int32_t R, const double* u,
                                       int64_t nvec, double* prox_out, double* eval_in, double* eval_out) {
  if (!reg || !u || !prox_out || !eval_in || !eval_out || nvec <= 0 || nvec > (1 << 20)) return fail(GLRM_ERR_INVALID, "bad argument");
  const int kp = G * R;
  if (path < 0 || path > 2 || G < 1 || R < 2 || kp > 128 || k < 1 || k > kp || (path != 0 && kp > 64))
    return fail(GLRM_ERR_INVALID, "bad path / layout / rank (path %d, G %d, R %d, k %d)", path, G, R, k);
  if (reg->wrap && path != 2) return fail(GLRM_ERR_INVALID, "only the general-sweep path knows the wrappers");
  std::vector<double> padded((size_t)nvec * kp, 0.0);
  for (int64_t v = 0; v < nvec; ++v)
    for (int c = 0; c < k; ++c) padded[(size_t)v * kp + c] = u[(size_t)v * k + c];
  DevArena scratch;
  double* d = nullptr;
  const size_t nb = (size_t)nvec * kp * 8, ne = (size_t)nvec * 8;
  if (const int rca = scratch.alloc(&d, (nb + 2 * ne) / 8)) return rca;
  RegHookArgs a{*reg, k, kp, alpha, nvec, d, d + (size_t)nvec * kp, d + (size_t)nvec * kp + nvec};
  hipError_t e = hipMemcpy(d, padded.data(), nb, hipMemcpyHostToDevice);
  int rc = GLRM_OK;
  if (e == hipSuccess) rc = reg_hook_launch(path, G, R, a);
  if (e == hipSuccess && !rc) e = hipGetLastError();
  if (e == hipSuccess && !rc) e = hipDeviceSynchronize();
  if (e == hipSuccess && !rc) e = hipMemcpy(prox_out, d, nb, hipMemcpyDeviceToHost);
  if (e == hipSuccess && !rc) e = hipMemcpy(eval_in, a.ein, ne, hipMemcpyDeviceToHost);
  if (e == hipSuccess && !rc) e = hipMemcpy(eval_out, a.eout, ne, hipMemcpyDeviceToHost);
  if (rc) return rc;
  if (e != hipSuccess) return fail(GLRM_ERR_HIP, "glrm_test_reg_prox_eval: %s", hipGetErrorString(e));
  return GLRM_OK;
}

// ------------------------------------------------------------------ vector-carrying regularizers (tests/test_gpu_regularizers_vec.py)
// The general sweeps' path (csrc/glrm_blockreg.hpp, VR = true) for a descriptor WITH its vector (include/glrm_hip_regvec.h): like
// reg_hook_block, one wave per vector, the k x 1 block in LDS with the general sweeps' stride.
namespace {
struct RegVecHookArgs {
  RegHookArgs a;
  const double* rv; // the descriptor's vector (device, a.k doubles)
  int rl;           // nfix / k
};

__global__ void __launch_bounds__(64) reg_hook_block_vec(const RegVecHookArgs h) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const RegHookArgs& a = h.a;
  const int tid = threadIdx.x, S = a.kp + 1;
  double* blk = sm;
  double* tmp = sm + S;
  double* red = tmp + 64;
  double* g = a.vec + (int64_t)blockIdx.x * a.kp;
  for (int c = tid; c < a.kp; c += 64) blk[c] = g[c];
  __syncthreads();
  const double e0 = block_reg_eval<1, true>(blk, S, a.k, 1, a.reg, red, h.rv, h.rl);
  block_prox<1, true>(blk, S, a.k, 1, a.reg, a.alpha, tmp, h.rv, h.rl);
  const double e1 = block_reg_eval<1, true>(blk, S, a.k, 1, a.reg, red, h.rv, h.rl);
  for (int c = tid; c < a.kp; c += 64) g[c] = blk[c];
  if (tid == 0) { a.ein[blockIdx.x] = e0; a.eout[blockIdx.x] = e1; }
}
} // namespace

// reg with its vector `rvec` of `rlen` entries (nfix of a fixed wrapper, k of RemQuadReg); kp: the padded rank (k <= kp <= 64).  The
// descriptor is taken as it is: what glrm_hip_set_regularizers_vec refuses is the caller's business to leave out.
// u: nvec x k (host), prox_out: nvec x kp (host, the padded vectors as the kernel leaves them), eval_in / eval_out: nvec.
extern "C" int glrm_test_regvec_prox_eval(const glrm_reg* reg, const double* rvec, int32_t rlen, int32_t k, int32_t kp, double alpha, const double* u,
                                          int64_t nvec, double* prox_out, double* eval_in, double* eval_out) {
  if (!reg || !rvec || !u || !prox_out || !eval_in || !eval_out || nvec <= 0 || nvec > (1 << 20)) return fail(GLRM_ERR_INVALID, "bad argument");
  if (k < 1 || kp < k || kp > 64 || rlen < 1 || rlen > k) return fail(GLRM_ERR_INVALID, "bad rank / length (k %d, kp %d, length %d)", k, kp, rlen);
  std::vector<double> padded((size_t)nvec * kp, 0.0);
  for (int64_t v = 0; v < nvec; ++v)
    for (int c = 0; c < k; ++c) padded[(size_t)v * kp + c] = u[(size_t)v * k + c];
  DevArena scratch;
  double* d = nullptr;
  const size_t nb = (size_t)nvec * kp * 8, ne = (size_t)nvec * 8;
  if (const int rca = scratch.alloc(&d, (nb + 2 * ne) / 8 + (size_t)k)) return rca;
  double* drv = d + (size_t)nvec * kp + 2 * nvec;
  RegVecHookArgs h{RegHookArgs{*reg, k, kp, alpha, nvec, d, d + (size_t)nvec * kp, d + (size_t)nvec * kp + nvec}, drv, rlen};
  std::vector<double> rvk((size_t)k, 0.0);
  for (int c = 0; c < rlen; ++c) rvk[(size_t)c] = rvec[c];
  hipError_t e = hipMemcpy(d, padded.data(), nb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(drv, rvk.data(), (size_t)k * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(reg_hook_block_vec, dim3((unsigned)nvec), dim3(64), (size_t)((kp + 1) + 64 + 16) * 8, 0, h);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(prox_out, d, nb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(eval_in, h.a.ein, ne, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(eval_out, h.a.eout, ne, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(GLRM_ERR_HIP, "glrm_test_regvec_prox_eval: %s", hipGetErrorString(e));
  return GLRM_OK;
}

// ------------------------------------------------------------------ loss hooks (tests/test_gpu_loss_pointwise.py)
// The kernels' own device functions on a batch of points: loss_both (csrc/glrm_device.hpp), the primitives of csrc/glrm_fastmath.hpp and
// obs_loss (csrc/glrm_multi.hpp).  No formula is restated here.
#include "glrm_multi.hpp"

namespace {
struct LossHookArgs {
  const glrm_loss* desc; // n descriptors (nullptr for the primitives that take none)
  const double* u;
  const double* a;
  int64_t n;
  double* L;  // n
  double* dL; // n
};

// One lane per point; neighbouring lanes hold whatever kinds the caller put side by side, so the switch of loss_both runs divergently as it
// does in the per-observation kernels.  One kernel per instantiation: nothing of one can be shared with another by the compiler.
template <bool NEED_GRAD, bool TRIG>
__global__ void __launch_bounds__(64) loss_hook_pointwise(const LossHookArgs h) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= h.n) return;
  const LossDesc l = load_loss(h.desc, i);
  double L, dL;
  loss_both<NEED_GRAD, TRIG>(l, h.u[i], h.a[i], L, dL);
  h.L[i] = L;
  h.dL[i] = dL;
}

// op: 1 fm_exp(u), 2 fm_log_ge1(u), 3 fm_log(u), 4 fm_rcp(u), 5 / 6 fm_logistic<true / false>(desc.scale, a, u) with a = +-1 as it is
template <int OP>
__global__ void __launch_bounds__(64) loss_hook_primitive(const LossHookArgs h) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= h.n) return;
  const double x = h.u[i];
  double L = 0.0, dL = 0.0;
  if constexpr (OP == 1) L = fm_exp(x);
  else if constexpr (OP == 2) L = fm_log_ge1(x);
  else if constexpr (OP == 3) L = fm_log(x);
  else if constexpr (OP == 4) L = fm_rcp(x);
  else fm_logistic<OP == 5>(h.desc[i].scale, h.a[i], x, L, dL);
  h.L[i] = L;
  h.dL[i] = dL;
}

struct ObsHookArgs {
  const glrm_loss* desc; // n
  const int32_t* d;      // n: 0 = idle slot, 1 = scalar loss, else the embedding dimension
  const double* level;   // n: the observation's value (level 1 .. max; the scalar losses' a)
  const double* u;       // n x P
  int64_t n;
  int lg;
  double* Lg; // n x P: obs_loss<true> as every lane of the slot returns it
  double* G;  // n x P: cg of lane sub
  double* Lt; // n x P: obs_loss<false>
};

// One wave per workgroup, observation i in slot i % (64 / P) of wave i / (64 / P); the slots behind the last observation are idle.  EVERY
// lane runs the call (obs_loss's contract); only the stores are guarded.
template <bool GRAD, int KM>
__global__ void __launch_bounds__(64) loss_hook_obs(const ObsHookArgs h) {
  const int lane = threadIdx.x, lg = h.lg, P = 1 << lg, SL = 64 >> lg, slot = lane >> lg, sub = lane & (P - 1);
  const int64_t i = (int64_t)blockIdx.x * SL + slot;
  const bool valid = i < h.n;
  const int64_t ic = valid ? i : h.n - 1;
  const LossDesc l = load_loss(h.desc, ic);
  const int dd = valid ? h.d[ic] : 0;
  const double av = h.level[ic];
  const double u = sub < dd ? h.u[ic * P + sub] : 0.0; // the lanes past the dimension hold 0, as multi_pass leaves them
  const double u0 = dd > 0 ? h.u[ic * P] : 0.0;
  double cg = 0.0;
  const double L = obs_loss<GRAD, true, KM>(l, u, u0, av, dd, sub, lg, lane - sub, nullptr, cg);
  if (!valid) return;
  if constexpr (GRAD) {
    h.Lg[i * P + sub] = L;
    h.G[i * P + sub] = cg;
  } else {
    h.Lt[i * P + sub] = L;
  }
}

template <int KM>
void obs_hook_launch(const ObsHookArgs& h, unsigned grid) {
  hipLaunchKernelGGL((loss_hook_obs<true, KM>), dim3(grid), dim3(64), 0, 0, h);
  hipLaunchKernelGGL((loss_hook_obs<false, KM>), dim3(grid), dim3(64), 0, 0, h);
}
} // namespace

// op 0: L and dL of loss_both<true, true>, <false, true>, <true, false>, <false, false> at the n points (desc[i], u[i], a[i]); L and dL are
// 4 x n (host), instantiation major.  op 1 .. 6: one primitive of csrc/glrm_fastmath.hpp (loss_hook_primitive) on u[i]; L and dL are n (dL is
// 0 except for op 5).  desc may be null for op 1 .. 4, a for op 1 .. 4.
extern "C" int glrm_test_loss_pointwise(const glrm_loss* desc, const double* u, const double* a, int64_t n, int32_t op, double* L, double* dL) {
  if (!u || !L || !dL || n <= 0 || n > (1 << 20) || op < 0 || op > 6) return fail(GLRM_ERR_INVALID, "bad argument");
  const bool need_desc = op == 0 || op >= 5;
  if (need_desc && (!desc || !a)) return fail(GLRM_ERR_INVALID, "op %d needs descriptors and a", op);
  const size_t nout = op == 0 ? 4 : 1, N = (size_t)n;
  DevArena scratch;
  double* d = nullptr; // [desc: 4 n][u: n][a: n][L: nout n][dL: nout n]
  if (const int rca = scratch.alloc(&d, (6 + 2 * nout) * N)) return rca;
  double *du = d + 4 * N, *da = du + N, *dLo = da + N, *ddL = dLo + nout * N;
  static_assert(sizeof(glrm_loss) == 32, "a descriptor is four doubles wide");
  hipError_t e = hipMemcpy(du, u, N * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess && need_desc) e = hipMemcpy(d, desc, N * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess && need_desc) e = hipMemcpy(da, a, N * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    LossHookArgs h{reinterpret_cast<const glrm_loss*>(d), du, da, n, dLo, ddL};
    auto at = [&](size_t v) { LossHookArgs w = h; w.L += v * N; w.dL += v * N; return w; };
    switch (op) {
      case 0:
        hipLaunchKernelGGL((loss_hook_pointwise<true, true>), grid, block, 0, 0, at(0));
        hipLaunchKernelGGL((loss_hook_pointwise<false, true>), grid, block, 0, 0, at(1));
        hipLaunchKernelGGL((loss_hook_pointwise<true, false>), grid, block, 0, 0, at(2));
        hipLaunchKernelGGL((loss_hook_pointwise<false, false>), grid, block, 0, 0, at(3));
        break;
      case 1: hipLaunchKernelGGL(loss_hook_primitive<1>, grid, block, 0, 0, h); break;
      case 2: hipLaunchKernelGGL(loss_hook_primitive<2>, grid, block, 0, 0, h); break;
      case 3: hipLaunchKernelGGL(loss_hook_primitive<3>, grid, block, 0, 0, h); break;
      case 4: hipLaunchKernelGGL(loss_hook_primitive<4>, grid, block, 0, 0, h); break;
      case 5: hipLaunchKernelGGL(loss_hook_primitive<5>, grid, block, 0, 0, h); break;
      default: hipLaunchKernelGGL(loss_hook_primitive<6>, grid, block, 0, 0, h); break;
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(L, dLo, nout * N * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(dL, ddL, nout * N * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(GLRM_ERR_HIP, "glrm_test_loss_pointwise: %s", hipGetErrorString(e));
  return GLRM_OK;
}

// obs_loss on n observations (desc[i], d[i], level[i], u[i * P .. i * P + d[i])), P = 2^lg lanes per slot, lg in 2 .. 6; observation i sits in
// slot i % (64 / P) of wave i / (64 / P).  kmask: 0 MULTI_KM_ALL, 1 MULTI_KM_MNL, 2 MULTI_KM_MNL | MULTI_KM_SCALAR, 3 MULTI_KM_ORD (the four
// glrm_multi.hip instantiates).  Lg, G, Lt: n x P (host): obs_loss<true>'s value and gradient component, obs_loss<false>'s value, per lane.
extern "C" int glrm_test_obs_loss(const glrm_loss* desc, const int32_t* d, const double* level, const double* u, int64_t n, int32_t lg, int32_t kmask,
                                  double* Lg, double* G, double* Lt) {
  if (!desc || !d || !level || !u || !Lg || !G || !Lt || n <= 0 || n > (1 << 20)) return fail(GLRM_ERR_INVALID, "bad argument");
  if (lg < 2 || lg > 6 || kmask < 0 || kmask > 3) return fail(GLRM_ERR_INVALID, "bad slot width / kind mask (lg %d, mask %d)", lg, kmask);
  const size_t N = (size_t)n, P = (size_t)1 << lg;
  for (size_t i = 0; i < N; ++i)
    if (d[i] < 0 || (size_t)d[i] > P) return fail(GLRM_ERR_INVALID, "observation %zu: dimension %d does not fit a slot of %zu lanes", i, d[i], P);
  DevArena scratch;
  double* dev = nullptr; // [desc: 4 n][level: n][u: n P][Lg: n P][G: n P][Lt: n P][d: n int32]
  if (const int rca = scratch.alloc(&dev, 5 * N + 4 * N * P + (N + 1) / 2)) return rca;
  double *dlev = dev + 4 * N, *du = dlev + N, *dLg = du + N * P, *dG = dLg + N * P, *dLt = dG + N * P;
  int32_t* dd = reinterpret_cast<int32_t*>(dLt + N * P);
  hipError_t e = hipMemcpy(dev, desc, N * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dlev, level, N * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(du, u, N * P * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dd, d, N * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const size_t SL = 64 / P;
    const unsigned grid = (unsigned)((N + SL - 1) / SL);
    const ObsHookArgs h{reinterpret_cast<const glrm_loss*>(dev), dd, dlev, du, n, lg, dLg, dG, dLt};
    if (kmask == 0) obs_hook_launch<MULTI_KM_ALL>(h, grid);
    else if (kmask == 1) obs_hook_launch<MULTI_KM_MNL>(h, grid);
    else if (kmask == 2) obs_hook_launch<MULTI_KM_MNL | MULTI_KM_SCALAR>(h, grid);
    else obs_hook_launch<MULTI_KM_ORD>(h, grid);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(Lg, dLg, N * P * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(G, dG, N * P * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(Lt, dLt, N * P * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(GLRM_ERR_HIP, "glrm_test_obs_loss: %s", hipGetErrorString(e));
  return GLRM_OK;
}
#endif
