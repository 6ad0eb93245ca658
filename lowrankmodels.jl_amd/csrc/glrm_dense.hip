// glrm_dense.hip -- host side of the fully observed QuadLoss path on the fp64 matrix cores
// (kernels in glrm_dense.hpp; line-search bookkeeping kernels shared with glrm_tiled.hpp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "glrm_engine.hpp"
#include "glrm_launch.hpp"
#include "glrm_tiled.hpp"
#include "glrm_dense.hpp"

using namespace glrm;

static int64_t round_up(int64_t v, int64_t q) { return (v + q - 1) / q * q; }

// super-tiles over the opposing dimension: a function of that dimension only (never of the shard layout),
// so the partial-sum order -- and therefore the result bits -- do not depend on the number of GPUs
static void pick_sup(int64_t n_other, int& nsup, int64_t& vps) {
  int64_t s = (n_other + 32767) / 32768;
  if (s < 1) s = 1;
  if (s > 4096) s = 4096;
  vps = round_up((n_other + s - 1) / s, DENSE_TN);
  nsup = (int)((n_other + vps - 1) / vps);
}

static int pack_view(glrm_handle* h, const double* dsrc, int64_t ldsrc, int colmajor, int transpose, int64_t seg0,
                     int64_t nseg, int64_t nother, double** dst, int64_t* lda) {
  const int64_t nseg_pad = round_up(nseg > 0 ? nseg : 1, 256); // whole 16-wave workgroups stay in bounds
  *lda = round_up(nother, 64);
  if (const int rc = h->mem.alloc(dst, (size_t)nseg_pad * (size_t)*lda)) return rc;
  const dim3 grid((unsigned)(*lda / 32), (unsigned)(nseg_pad / 32));
  hipLaunchKernelGGL(dense_pack_kernel, grid, dim3(256), 0, h->stream, dsrc, ldsrc, colmajor, transpose, seg0, nseg, nother, *dst, *lda);
  HIPCK(hipGetLastError());
  return GLRM_OK;
}

int glrm_setup_dense(glrm_handle* h, const glrm_problem* p) {
  if (p->rowptr || p->colidx || p->rowvals || p->colptr || p->rowidx || p->colvals)
    return fail(GLRM_ERR_INVALID, "dense_A and the observation lists are mutually exclusive");
  if (p->dense_reserved != 0) return fail(GLRM_ERR_INVALID, "glrm_problem.dense_reserved must be 0");
  if (!(p->n_losses == 1 && p->losses[0].kind == GLRM_LOSS_QUAD))
    return fail(GLRM_ERR_UNSUPPORTED, "the dense path needs one QuadLoss descriptor for all columns; pass observation lists otherwise");
  if (!(h->kp == 16 || h->kp == 32 || h->kp == 64))
    return fail(GLRM_ERR_UNSUPPORTED, "the dense path supports ranks 9..64; pass observation lists otherwise");
  const int64_t need_ld = p->dense_colmajor ? p->m : p->n;
  if (p->dense_ld < need_ld) return fail(GLRM_ERR_INVALID, "dense_ld is smaller than the matrix dimension");
  h->dense = true;
  h->dense_scale = p->losses[0].scale;
  h->side[GLRM_ROWS].nnz = h->side[GLRM_ROWS].nseg * h->n;
  h->side[GLRM_COLS].nnz = h->side[GLRM_COLS].nseg * h->m;
  // Bring the caller's matrix to the device if needed.  Whole problem on this handle: one upload, both packed views come from it.
  // A shard of a multi-GPU fit only needs its row block (for the X half-step) and its column block (for the Y half-step): those
  // two sub-matrices are uploaded one after the other (2D copies), never the whole matrix -- at C3 on 8 GPUs 10 + 10 GB per
  // device instead of 80 GB.  The NaN check (src/glrm.jl:63-71) covers the shard's row block; the row blocks partition A.
  const bool on_dev = (p->flags & GLRM_PROBLEM_DEVICE_ARRAYS) != 0;
  const bool whole = h->side[GLRM_ROWS].begin == 0 && h->side[GLRM_ROWS].end == h->m && h->side[GLRM_COLS].begin == 0 && h->side[GLRM_COLS].end == h->n;
  const int cm = p->dense_colmajor ? 1 : 0;
  const int64_t ld = p->dense_ld;
  if (!on_dev) { // walk along the contiguous dimension of the caller's storage order (column-major: what the Julia shim passes)
    bool bad = false;
    int64_t bi = 0, bj = 0;
    if (cm) {
      for (int64_t j = 0; j < h->n && !bad; ++j) {
        const double* col = p->dense_A + j * ld;
        for (int64_t i = h->side[GLRM_ROWS].begin; i < h->side[GLRM_ROWS].end; ++i)
          if (std::isnan(col[i])) { bad = true; bi = i; bj = j; break; }
      }
    } else {
      for (int64_t i = h->side[GLRM_ROWS].begin; i < h->side[GLRM_ROWS].end && !bad; ++i) {
        const double* row = p->dense_A + i * ld;
        for (int64_t j = 0; j < h->n; ++j)
          if (std::isnan(row[j])) { bad = true; bi = i; bj = j; break; }
      }
    }
    if (bad) return fail(GLRM_ERR_NONFINITE, "Observed value in entry (%lld, %lld) is NaN.", (long long)bi, (long long)bj);
  }
  int rc = GLRM_OK;
  DevArena scratch; // the staged upload of the caller's host matrix
  if (on_dev) {
    for (int s = 0; s < 2 && !rc; ++s) rc = pack_view(h, p->dense_A, ld, cm, s, h->side[s].begin, h->side[s].nseg, h->side[s ^ 1].nglob, &h->side[s].A, &h->side[s].lda);
    if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(GLRM_ERR_HIP, "dense pack failed");
  } else if (whole) {
    double* tmp = nullptr;
    const size_t runs = cm ? (size_t)p->n : (size_t)p->m, run = cm ? (size_t)p->m : (size_t)p->n; // contiguous runs and their length
    if ((rc = scratch.alloc(&tmp, runs * run))) return rc;
    if (hipMemcpy2DAsync(tmp, run * 8, p->dense_A, (size_t)ld * 8, run * 8, runs, hipMemcpyHostToDevice, h->stream) != hipSuccess)
      rc = fail(GLRM_ERR_HIP, "upload of the dense matrix failed");
    for (int s = 0; s < 2 && !rc; ++s) rc = pack_view(h, tmp, (int64_t)run, cm, s, 0, h->side[s].nseg, h->side[s ^ 1].nglob, &h->side[s].A, &h->side[s].lda);
    if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(GLRM_ERR_HIP, "dense pack failed");
    scratch.release(&tmp);
  } else {
    // (first segment, segments, extent of the other dimension) of the row block and of the column block
    for (int side = 0; side < 2 && !rc; ++side) {
      glrm_handle::Side& v = h->side[side];
      const int64_t s0 = v.begin, ns = v.nseg, other = h->side[side ^ 1].nglob;
      if (ns <= 0) { rc = pack_view(h, p->dense_A, ld, cm, side, 0, 0, other, &v.A, &v.lda); continue; }
      // the block as a dense sub-matrix in the caller's own storage order: segments run along the caller's rows (row block) / columns
      const bool seg_is_run = (side == GLRM_ROWS) != (cm != 0); // are whole segments contiguous runs of the source?
      const size_t width = (size_t)(seg_is_run ? other : ns) * 8, height = (size_t)(seg_is_run ? ns : other);
      const double* src = p->dense_A + (seg_is_run ? s0 * ld : s0);
      double* tmp = nullptr;
      if ((rc = scratch.alloc(&tmp, width / 8 * height))) return rc;
      if (hipMemcpy2DAsync(tmp, width, src, (size_t)ld * 8, width, height, hipMemcpyHostToDevice, h->stream) != hipSuccess)
        rc = fail(GLRM_ERR_HIP, "upload of the dense block failed");
      // inside tmp the block starts at segment 0 and has leading dimension width / 8
      if (!rc) rc = pack_view(h, tmp, (int64_t)(width / 8), cm, side, 0, ns, other, &v.A, &v.lda);
      if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(GLRM_ERR_HIP, "dense pack failed");
      scratch.release(&tmp);
    }
  }
  if (rc) return rc;
  for (int s = 0; s < 2; ++s) pick_sup(h->side[s ^ 1].nglob, h->side[s].pass.nsup, h->side[s].vps);
  for (int s = 0; s < 2; ++s)
    if ((rc = glrm_alloc_pass_buffers(h, s))) return rc;
  // glrm_options.quad_gram: line-search trials from the quadratic form, no pass over A per trial
  h->dense_gram = h->opts.quad_gram != 0;
  if (h->dense_gram) {
    if ((rc = h->mem.alloc(&h->gramH, (size_t)h->kp * h->kp))) return rc;
    if ((rc = h->mem.alloc(&h->gram_part, (size_t)GRAM_BLOCKS * h->kp * h->kp))) return rc;
    for (glrm_handle::Side& v : h->side)
      if ((rc = h->mem.alloc(&v.jloss, (size_t)(v.nseg > 0 ? v.nseg : 1)))) return rc;
  }
  return GLRM_OK;
}

// stage 0: H = other other' (kp x kp); stage 1: the trial objectives of the active segments from the quadratic form
static void launch_gram(int kp, int stage, const TiledArgs& a, const double* other, int64_t n_other, double* part, double* H, double scale, hipStream_t st) {
  auto by_kp = [&](auto kpc) {
    constexpr int KP = decltype(kpc)::value;
    if (stage == 0) {
      hipLaunchKernelGGL((dense_gram_partial_kernel<KP>), dim3(GRAM_BLOCKS), dim3(256), 0, st, other, n_other, part);
      hipLaunchKernelGGL((dense_gram_final_kernel<KP>), dim3((KP * KP + 255) / 256), dim3(256), 0, st, part, H);
    } else {
      hipLaunchKernelGGL((dense_gram_trial_kernel<KP>), dim3((unsigned)((a.nseg + 255) / 256)), dim3(256), 0, st, a, H, scale);
    }
    return GLRM_OK;
  };
  glrm_dispatch<16, 32>(kp, by_kp, [&] { return by_kp(glrm_const<64>{}); }); // (glrm_setup_dense admits kp 16 / 32 / 64)
}

template <int KP, int NWD>
static void launch_dense_inst(bool grad, const DenseArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.nseg + NWD * 16 - 1) / (NWD * 16)), (unsigned)a.nsup);
  if (grad) hipLaunchKernelGGL((dense_pass_kernel<KP, true, NWD>), grid, dim3(NWD * 64), 0, st, a);
  else hipLaunchKernelGGL((dense_pass_kernel<KP, false, NWD>), grid, dim3(NWD * 64), 0, st, a);
}

static void launch_dense_any(int kp, bool grad, const DenseArgs& a, hipStream_t st) {
  auto by_kp = [&](auto kpc) {
    constexpr int KP = decltype(kpc)::value;
    // 16-wave workgroups (256 segments share one staged tile) unless the problem is too small to fill the chip with them
    if (a.nseg * (int64_t)a.nsup >= 256 * 256) launch_dense_inst<KP, 16>(grad, a, st);
    else launch_dense_inst<KP, 4>(grad, a, st);
    return GLRM_OK;
  };
  glrm_dispatch<16, 32>(kp, by_kp, [&] { return by_kp(glrm_const<64>{}); });
}

// One half-step on the dense path: pass 1 (residuals, objective, gradient on the matrix cores) -> per-segment
// reduce + first trial point -> rounds of (trial objective pass, decide) until no segment is still searching.
int glrm_run_dense(glrm_handle* h, const glrm_step& step) { // (no row range: glrm_hip_step_x_range refuses the dense path)
  const int side = step.side;
  const glrm_handle::Side& v = h->side[side];
  if (v.nseg <= 0) return GLRM_OK;
  TiledArgs a{};
  glrm_fill_side(a, h, step);
  DenseArgs d{}; // the side as the MFMA kernels read it: what `a` says, plus the packed matrix
  d.nseg = a.nseg; d.xsrc = a.own; d.own_offset = a.own_offset; d.other = a.other;
  d.n_other = h->side[side ^ 1].nglob;
  d.A = v.A; d.lda = v.lda; d.vec_per_sup = v.vps;
  d.scale = h->dense_scale;
  a.ptr = nullptr; // no view: every segment has dense_len observations
  a.dense_len = d.n_other;
  glrm_bind_pass_buffers(a, h, side);
  d.nsup = a.nsup;
  d.part = a.part;
  d.active = a.active;
  const bool gram = h->dense_gram && !step.eval_only && !step.fixed();
  a.jloss = gram ? v.jloss : nullptr;
  HIPCK(hipMemsetAsync(h->nactive, 0, 4, h->stream));
  if (gram) launch_gram(h->kp, 0, a, d.other, d.n_other, h->gram_part, h->gramH, d.scale, h->stream);
  launch_dense_any(h->kp, true, d, h->stream);
  glrm_launch_col_small(h->kp, 0, a, h->stream);
  HIPCK(hipGetLastError());
  if (step.eval_only || step.fixed()) return GLRM_OK;
  DenseArgs t = d;
  t.xsrc = a.trial; // trial points are stored per local segment
  t.own_offset = 0;
  return glrm_run_rounds(
      h, a, step.min_stepsize, glrm_act_lists{},
      [&](int, unsigned int, int32_t*) {
        if (gram) launch_gram(h->kp, 1, a, d.other, d.n_other, h->gram_part, h->gramH, d.scale, h->stream);
        else launch_dense_any(h->kp, false, t, h->stream);
        return GLRM_OK;
      },
      [&](const TiledArgs& dd) { glrm_launch_col_small(h->kp, 1, dd, h->stream); });
}
