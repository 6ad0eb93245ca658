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
  const char* v = getenv("GLRM_HIP_TEST_FAIL_FINALIZE");
  return v && *v && atoi(v) != 0;
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
#endif
