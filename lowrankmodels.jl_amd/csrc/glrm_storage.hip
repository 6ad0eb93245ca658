// glrm_storage.hip -- glrm_options.storage = 1 (include/glrm_hip_storage.h): A, X and Y stored as floats on the gather sweeps, all
// arithmetic in fp64.  This unit holds the ST = float instantiations of the gather sweeps and the penalty kernel (glrm_sweep.hpp; the
// double ones are glrm_hip.hip's), the narrowing / widening copies, and what create checks for such a handle.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "glrm_sweep.hpp"

using namespace glrm;

// ------------------------------------------------------------------ narrowing / widening copies

// dst[i] = (float)src[i] (round to nearest even).  *flag = 1 when a finite value leaves float's range.
__global__ void narrow_kernel(const double* __restrict__ src, float* __restrict__ dst, int64_t n, int* flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = src[i];
    const float f = (float)v;
    if (isinf(f) && !isinf(v)) *flag = 1;
    dst[i] = f;
  }
}

// factor copies between the host's unpadded k x nvec doubles (staged on the device) and the handle's floats of leading dimension kp
__global__ void narrow_factor_kernel(const double* __restrict__ src, float* __restrict__ dst, int k, int kp, int64_t nvec) {
  const int64_t n = nvec * kp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / kp;
    const int c = (int)(i - v * kp);
    dst[i] = c < k ? (float)src[v * k + c] : 0.0f; // the padding stays exactly zero
  }
}

__global__ void widen_factor_kernel(const float* __restrict__ src, double* __restrict__ dst, int k, int kp, int64_t nvec) {
  const int64_t n = nvec * k;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / k;
    const int c = (int)(i - v * k);
    dst[i] = (double)src[v * kp + c];
  }
}

static unsigned copy_grid(int64_t n) { return (unsigned)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 4096); }

// One view's values: a float array of the handle's own replaces the double one, which is released.
static int narrow_values(glrm_handle* h, double** vals, int64_t nnz, int* dflag) {
  float* f = nullptr;
  if (const int rc = h->mem.alloc(&f, (size_t)std::max<int64_t>(nnz, 0))) return rc;
  if (nnz > 0) hipLaunchKernelGGL(narrow_kernel, dim3(copy_grid(nnz)), dim3(256), 0, h->stream, *vals, f, nnz, dflag);
  const hipError_t e = nnz > 0 ? hipGetLastError() : hipSuccess;
  const hipError_t e2 = hipStreamSynchronize(h->stream);
  h->mem.release(vals);
  *vals = reinterpret_cast<double*>(f); // glrm_handle::storage: floats behind the double* field
  HIPCK(e);
  HIPCK(e2);
  return GLRM_OK;
}

int glrm_narrow_views(glrm_handle* h) {
  DevArena scratch;
  int* dflag = nullptr;
  int rc = scratch.alloc(&dflag, 1);
  if (rc) return rc;
  int flag = 0;
  hipError_t e = hipMemsetAsync(dflag, 0, sizeof(int), h->stream);
  rc = e == hipSuccess ? GLRM_OK : fail(GLRM_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
  if (!rc) rc = narrow_values(h, &h->side[GLRM_ROWS].vals, h->side[GLRM_ROWS].nnz, dflag);
  if (!rc) rc = narrow_values(h, &h->side[GLRM_COLS].vals, h->side[GLRM_COLS].nnz, dflag);
  if (!rc) {
    e = hipMemcpy(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(GLRM_ERR_HIP, "hipMemcpy failed: %s", hipGetErrorString(e));
  }
  if (rc) return rc;
  if (flag) return fail(GLRM_ERR_NONFINITE, "storage = f32: an observed value is finite as a double and +-Inf as a float");
  return GLRM_OK;
}

int glrm_check_narrowable(const char* name, const double* v, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (std::isfinite(v[i]) && std::isinf((float)v[i]))
      return fail(GLRM_ERR_NONFINITE, "storage = f32: %s holds %g at position %lld, which is finite as a double and +-Inf as a float", name, v[i],
                  (long long)i);
  return GLRM_OK;
}

int glrm_narrow_factor(glrm_handle* h, const double* host, void* dev, int64_t nvec) {
  if (nvec <= 0) return GLRM_OK;
  DevArena scratch;
  double* stage = nullptr;
  const size_t bytes = (size_t)h->k * nvec * sizeof(double);
  if (const int rc = scratch.alloc(&stage, (size_t)h->k * nvec)) return rc;
  hipError_t e = hipMemcpyAsync(stage, host, bytes, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(narrow_factor_kernel, dim3(copy_grid(nvec * h->kp)), dim3(256), 0, h->stream, stage, (float*)dev, h->k, h->kp, nvec);
    e = hipGetLastError();
  }
  const hipError_t e2 = hipStreamSynchronize(h->stream);
  HIPCK(e);
  HIPCK(e2);
  return GLRM_OK;
}

int glrm_widen_factor(glrm_handle* h, const void* dev, double* host, int64_t nvec) {
  if (nvec <= 0) return GLRM_OK;
  DevArena scratch;
  double* stage = nullptr;
  const size_t bytes = (size_t)h->k * nvec * sizeof(double);
  if (const int rc = scratch.alloc(&stage, (size_t)h->k * nvec)) return rc;
  hipLaunchKernelGGL(widen_factor_kernel, dim3(copy_grid(nvec * h->k)), dim3(256), 0, h->stream, (const float*)dev, stage, h->k, h->kp, nvec);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host, stage, bytes, hipMemcpyDeviceToHost, h->stream);
  const hipError_t e2 = hipStreamSynchronize(h->stream);
  HIPCK(e);
  HIPCK(e2);
  return GLRM_OK;
}

// ------------------------------------------------------------------ what a float handle refuses at create

int glrm_check_storage_regs(const glrm_reg* rx, int64_t n_rx, const glrm_reg* ry, int64_t n_ry) {
  for (int side = 0; side < 2; ++side) {
    const glrm_reg* r = side ? ry : rx;
    const int64_t cnt = side ? n_ry : n_rx;
    for (int64_t i = 0; i < cnt; ++i) {
      if (r[i].wrap != 0)
        return fail(GLRM_ERR_UNSUPPORTED, "storage = f32: %s[%lld] is a wrapped regularizer; they run on the general sweeps, which have no f32 form",
                    side ? "ry" : "rx", (long long)i);
      if (r[i].kind >= GLRM_REG_QUAD_CONSTRAINT)
        return fail(GLRM_ERR_UNSUPPORTED, "storage = f32: %s[%lld] is a vector regularizer (kind %d); the f32 sweeps take scales and element-wise kinds only",
                    side ? "ry" : "rx", (long long)i, r[i].kind);
    }
  }
  return GLRM_OK;
}

int glrm_check_storage(const glrm_problem* p, const glrm_options* o) {
  if (!o || o->storage == GLRM_STORAGE_F64) return GLRM_OK;
  if (o->storage != GLRM_STORAGE_F32) return fail(GLRM_ERR_INVALID, "glrm_options.storage must be 0 (f64) or 1 (f32), got %d", o->storage);
  if (p->dense_A) return fail(GLRM_ERR_UNSUPPORTED, "storage = f32: the dense_A hand-over has no f32 form (hand over observation lists)");
  if (o->sum_order == 1) return fail(GLRM_ERR_UNSUPPORTED, "storage = f32: the reference-order mode (sum_order = 1) has no f32 form");
  if (o->tiled == 2) return fail(GLRM_ERR_UNSUPPORTED, "storage = f32: the LDS-tiled sweeps (tiled = 2) have no f32 form; f32 runs the gather sweeps");
  if (o->quad_gram == 1) return fail(GLRM_ERR_UNSUPPORTED, "storage = f32: quad_gram belongs to the dense path, which has no f32 form");
  if (p->flags & GLRM_PROBLEM_DEFER_SETUP) return fail(GLRM_ERR_UNSUPPORTED, "storage = f32: sharded fits (GLRM_PROBLEM_DEFER_SETUP) are not available");
  if (!(p->row_begin == 0 && p->row_end == p->m && p->col_begin == 0 && p->col_end == p->n))
    return fail(GLRM_ERR_UNSUPPORTED, "storage = f32: sharded fits (a row / column range that is not the whole problem) are not available");
  for (int64_t i = 0; i < p->n_losses; ++i)
    if (p->losses[i].dim > 1)
      return fail(GLRM_ERR_UNSUPPORTED, "storage = f32: loss %lld has dim = %d; multi-dimensional losses run on the general sweeps, which have no f32 form",
                  (long long)i, p->losses[i].dim);
  return glrm_check_storage_regs(p->rx, p->n_rx, p->ry, p->n_ry);
}

extern "C" int glrm_hip_storage(glrm_handle* h) { return h ? h->storage : fail(GLRM_ERR_INVALID, "NULL handle"); }

// ------------------------------------------------------------------ the float instantiations

void glrm_launch_sweep_f32(int G, int R, int waves, int loss, int side, const SweepArgs& a, hipStream_t st) {
  launch_sweep_st<float>(G, R, waves, loss, side, a, st);
}

void glrm_launch_penalty_f32(glrm_handle* h, int side) { launch_penalty_st<float>(h, side); }
