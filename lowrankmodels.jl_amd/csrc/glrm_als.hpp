// glrm_als.hpp -- the kernel of glrm_hip_als_solve (include/glrm_hip_als.h, which states the arithmetic and its order; this file only says
// how the work is dealt out).  One workgroup per segment:
//   stage      ALS_CHUNK observations at a time: the opposing vectors go through registers into LDS with 16-byte loads (a rank-64 vector
//              is 512 B, 32 lanes), a_t behind each vector (column KP of the staged row), w_t beside them.  The loads of chunk c + 1 are
//              issued before the arithmetic of chunk c and stored after it.
//   accumulate the lower triangle of the KP x KP Gram matrix in ALS_B x ALS_B blocks, one block per lane, in registers; the right-hand side
//              is block column KP / ALS_B of the same scheme (the staged a_t is "component KP" of v_t), so every lane runs the same
//              code.  Per observation a lane reads 2 x ALS_B doubles from LDS for ALS_B^2 multiply-adds; u = w * v is formed in registers.
//              Every entry has one accumulator that walks t ascending, so the chunk, the block shape and the lane count change no bit.
//   factorise  the triangle is written packed into LDS (over the stage) and wave 0 -- lane i = row i -- runs the left-looking Cholesky
//              and the two substitutions (als_factor_solve); values cross lanes by LDS (L) and by shuffles (the pivots, z_c, x_c).
// The first two stages are als_gram below, which cd_solve_kernel (glrm_cd.hpp) calls too.
// Blocks: KP = 64 -> 136 triangle + 16 right-hand-side blocks on 192 lanes; KP = 32 -> 36 + 8 on 64; KP = 16 -> 10 + 4; KP = 8 -> 3 + 2.
#pragma once

#include "../../include/glrm_hip_als.h"
#include "glrm_engine.hpp"

namespace glrm {

constexpr int ALS_CHUNK = 32;                       // observations per staging chunk (tests/test_gpu_als.py names it)
constexpr int ALS_B = 4;                            // block edge
constexpr int als_threads(int KP) { return KP == 64 ? 192 : 64; }
constexpr int als_ld(int KP) { return KP + ALS_B; } // doubles per staged observation: v_t, a_t, zeros
// waves per SIMD the register allocation is held to: a short row is bound by the latency of its gathers, so several workgroups per CU
// (KP = 32: 9.5 KB of LDS and one wave each) must be resident
constexpr int als_min_waves(int KP) { return KP == 64 ? 3 : 4; }

struct AlsArgs {
  const int64_t* ptr; const int32_t* idx; const double* vals; // the solved side's view
  const double* opp;                                          // opposing factor, ld kp
  double* own;                                                // solved factor, ld kp
  const glrm_loss* losses; int loss_single;
  const glrm_reg* regs; int reg_single;
  const int32_t* order;                                       // workgroup -> local segment, longest first
  int8_t* status;
  int64_t nseg;
  int k, side;
};

__device__ __forceinline__ int als_tri(int a, int b) { return a * (a + 1) / 2 + b; } // a >= b

// LDS writes of one lane, read by another lane of the SAME wave in a later instruction
__device__ __forceinline__ void als_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The stage and the accumulation above, for the segment [lo, lo + len) of the solved side's view: on return (after a workgroup barrier)
// the packed lower triangle of G stands at lds[als_tri(r, c)] and b at lds[KP * (KP + 1) / 2 + r].  Called by every lane of the workgroup;
// als_solve_kernel and cd_solve_kernel (glrm_cd.hpp) share it, so the two solvers see the same G and b bit for bit.
template <int KP>
__device__ __forceinline__ void als_gram(const AlsArgs& a, const int64_t lo, const int64_t len, const double wseg, double* const lds, double* const wl) {
  constexpr int T = als_threads(KP), LD = als_ld(KP), NB = KP / ALS_B, NTRI = NB * (NB + 1) / 2, NBLK = NTRI + NB;
  constexpr int P = KP / 2;                                  // 16-byte pieces per vector
  constexpr int NIT = (ALS_CHUNK * P + T - 1) / T;           // pieces per lane and chunk
  static_assert(NBLK <= T && ALS_CHUNK <= T && KP <= 64 && KP % ALS_B == 0, "one block per lane, one row per lane of wave 0");
  const int tid = threadIdx.x;

  // this lane's block: rows ALS_B * br .., columns ALS_B * bc .. (bc == NB: the right-hand side)
  int br = 0, bc = 0;
  const bool work = tid < NBLK;
  if (tid < NTRI) {
    while ((br + 1) * (br + 2) / 2 <= tid) ++br;
    bc = tid - br * (br + 1) / 2;
  } else if (work) {
    br = tid - NTRI;
    bc = NB;
  }
  double acc[ALS_B][ALS_B];
#pragma unroll
  for (int i = 0; i < ALS_B; ++i)
#pragma unroll
    for (int j = 0; j < ALS_B; ++j) acc[i][j] = 0.0;
  for (int o = tid; o < ALS_CHUNK; o += T) {                 // the columns behind a_t
    lds[o * LD + KP + 1] = 0.0; lds[o * LD + KP + 2] = 0.0; lds[o * LD + KP + 3] = 0.0;
  }

  double2 pv[NIT];
  double pa = 0.0, pw = 0.0;                                 // lane o < ALS_CHUNK: a_t and w_t of observation o of the chunk
  auto fetch = [&](int64_t base) {                           // chunk [base, base + ALS_CHUNK) of the list -> registers
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int p = tid + it * T, o = p / P, piece = p % P;
      pv[it] = make_double2(0.0, 0.0);
      if (o < ALS_CHUNK && base + o < len) {
        const int64_t j = a.idx[lo + base + o];
        pv[it] = *reinterpret_cast<const double2*>(a.opp + j * KP + 2 * piece);
      }
    }
    if (tid < ALS_CHUNK && base + tid < len) {
      pa = a.vals[lo + base + tid];
      pw = a.side == GLRM_COLS ? wseg : a.losses[a.loss_single ? 0 : a.idx[lo + base + tid]].scale;
    }
  };
  auto stash = [&]() {                                       // registers -> LDS
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int p = tid + it * T, o = p / P, piece = p % P;
      if (o < ALS_CHUNK) *reinterpret_cast<double2*>(&lds[o * LD + 2 * piece]) = pv[it];
    }
    if (tid < ALS_CHUNK) { lds[tid * LD + KP] = pa; wl[tid] = pw; }
  };

  if (len > 0) fetch(0);
  for (int64_t base = 0; base < len; base += ALS_CHUNK) {
    __syncthreads();                                         // the reads of the chunk before
    stash();
    __syncthreads();
    if (base + ALS_CHUNK < len) fetch(base + ALS_CHUNK);     // in flight behind the arithmetic
    const int cnt = len - base < ALS_CHUNK ? (int)(len - base) : ALS_CHUNK;
    if (work) {
      for (int t = 0; t < cnt; ++t) {
        const double w = wl[t];
        const double2 r0 = *reinterpret_cast<const double2*>(&lds[t * LD + ALS_B * br]), r1 = *reinterpret_cast<const double2*>(&lds[t * LD + ALS_B * br + 2]);
        const double2 c0 = *reinterpret_cast<const double2*>(&lds[t * LD + ALS_B * bc]), c1 = *reinterpret_cast<const double2*>(&lds[t * LD + ALS_B * bc + 2]);
        const double u[ALS_B] = {w * r0.x, w * r0.y, w * r1.x, w * r1.y}, v[ALS_B] = {c0.x, c0.y, c1.x, c1.y};
#pragma unroll
        for (int i = 0; i < ALS_B; ++i)
#pragma unroll
          for (int j = 0; j < ALS_B; ++j) {
            const double prod = u[i] * v[j];                 // a multiply, then an add (-ffp-contract=off)
            acc[i][j] = acc[i][j] + prod;
          }
      }
    }
  }

  // the packed triangle and the right-hand side, over the stage
  double* const tri = lds;
  double* const rhs = lds + KP * (KP + 1) / 2;
  __syncthreads();
  if (work) {
#pragma unroll
    for (int i = 0; i < ALS_B; ++i) {
      const int r = ALS_B * br + i;
      if (bc == NB) {
        rhs[r] = acc[i][0];
      } else {
#pragma unroll
        for (int j = 0; j < ALS_B; ++j) {
          const int c = ALS_B * bc + j;
          if (r >= c) tri[als_tri(r, c)] = acc[i][j];
        }
      }
    }
  }
  __syncthreads();
}

// doubles of LDS a kernel over als_gram needs: the stage, or the packed triangle and the right-hand side written over it
constexpr int als_lds_doubles(int KP) { return ALS_CHUNK * als_ld(KP) > KP * (KP + 1) / 2 + KP ? ALS_CHUNK * als_ld(KP) : KP * (KP + 1) / 2 + KP; }

// Wave 0 of a workgroup after als_gram, lane i = row i of the leading k x k system: the diagonal M_aa = G_aa + gamma, the pivot tolerance,
// the left-looking Cholesky and the two substitutions of include/glrm_hip_als.h.  Returns GLRM_ALS_SOLVED with x_i in `x` of lane i < k, or
// GLRM_ALS_KEPT_PIVOT (wave-uniform).  als_solve_kernel and stream_kernel (glrm_stream.hpp) both call it: one statement of the solve.
__device__ __forceinline__ int als_factor_solve(double* const tri, const double* const rhs, const int k, const double gamma, double& x) {
  const int i = threadIdx.x;
  const bool row = i < k;
  if (row) tri[als_tri(i, i)] = tri[als_tri(i, i)] + gamma;
  als_wave_sync();
  double maxd = tri[0];
  for (int c = 1; c < k; ++c) {
    const double d = tri[als_tri(c, c)];
    if (d > maxd) maxd = d;
  }
  const double tol = ((double)k * 0x1p-52) * maxd;
  for (int j = 0; j < k; ++j) {
    double s = 0.0;
    if (row && i >= j) {
      s = tri[als_tri(i, j)];
      const double *li = tri + als_tri(i, 0), *lj = tri + als_tri(j, 0);
      for (int c = 0; c < j; ++c) {
        const double prod = li[c] * lj[c];
        s = s - prod;
      }
    }
    const double sj = __shfl(s, j, 64);
    if (!(sj > tol)) return GLRM_ALS_KEPT_PIVOT;             // the pivot rule (wave-uniform); the point keeps every bit
    const double d = sqrt(sj);
    if (row && i >= j) tri[als_tri(i, j)] = i == j ? d : s / d;
    als_wave_sync();
  }
  // forward: lane i carries b_i minus the products so far; z_c leaves lane c when its turn comes
  double s = row ? rhs[i] : 0.0;
  for (int c = 0; c < k; ++c) {
    const double zc = __shfl(s, c, 64) / tri[als_tri(c, c)];
    if (i == c) s = zc;
    else if (row && i > c) {
      const double prod = tri[als_tri(i, c)] * zc;
      s = s - prod;
    }
  }
  // back: c descending
  for (int c = k - 1; c >= 0; --c) {
    const double xc = __shfl(s, c, 64) / tri[als_tri(c, c)];
    if (i == c) s = xc;
    else if (i < c) {
      const double prod = tri[als_tri(c, i)] * xc;
      s = s - prod;
    }
  }
  x = s;
  return GLRM_ALS_SOLVED;
}

template <int KP>
__global__ void __launch_bounds__(als_threads(KP), als_min_waves(KP)) als_solve_kernel(const AlsArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[als_lds_doubles(KP)];
  __shared__ double wl[ALS_CHUNK];

  const int tid = threadIdx.x, k = a.k;
  const int64_t seg = a.order[blockIdx.x];
  const int64_t lo = a.ptr[seg], len = a.ptr[seg + 1] - lo;
  const glrm_reg reg = a.regs[a.reg_single ? 0 : seg];
  const double gamma = reg.kind == GLRM_REG_QUAD ? reg.scale : 0.0;
  if (gamma == 0.0 && len < k) {                             // the short rule (workgroup-uniform)
    if (tid == 0) a.status[seg] = GLRM_ALS_KEPT_SHORT;
    return;
  }
  const double wseg = a.side == GLRM_COLS ? a.losses[a.loss_single ? 0 : seg].scale : 0.0;
  als_gram<KP>(a, lo, len, wseg, lds, wl);
  if (tid >= 64) return;

  // wave 0: lane i = row i of the leading k x k system
  double x = 0.0;
  const int st = als_factor_solve(lds, lds + KP * (KP + 1) / 2, k, gamma, x);
  if (st == GLRM_ALS_SOLVED && tid < k) a.own[seg * KP + tid] = x;
  if (tid == 0) a.status[seg] = (int8_t)st;
}

} // namespace glrm
