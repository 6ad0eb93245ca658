// glrm_multi.hip -- host side of the general sweeps (glrm_multi.hpp): multi-dimensional losses, block
// regularizers and offsets.  Part of libglrm_hip.so.
#include "glrm_multi.hpp"

#include "glrm_engine.hpp"
#include "glrm_launch.hpp"

using namespace glrm;

// The kernels that apply a regularizer exist twice: VR = true holds the vector regularizers and is launched when a descriptor of the
// side names one or carries a vector (glrm_handle::Side::vecreg -> MultiArgs::vecreg; csrc/glrm_device.hpp, DESIGN.md sections
// 4.11 and 4.14).
#define MULTI_SWEEP(threads, ...)                                                                                                        \
  do {                                                                                                                                   \
    if (a.vecreg) hipLaunchKernelGGL((multi_sweep_kernel<true, __VA_ARGS__>), dim3((unsigned)a.nseg), dim3(threads), lds, h->stream, a);  \
    else hipLaunchKernelGGL((multi_sweep_kernel<false, __VA_ARGS__>), dim3((unsigned)a.nseg), dim3(threads), lds, h->stream, a);          \
  } while (0)
#define MULTI_COLDECIDE(...)                                                                  \
  do {                                                                                        \
    if (sa.m.vecreg) hipLaunchKernelGGL(multi_coldecide_kernel<true>, __VA_ARGS__, sa);       \
    else hipLaunchKernelGGL(multi_coldecide_kernel<false>, __VA_ARGS__, sa);                  \
  } while (0)

// Column spans of Y (get_yidxs, src/losses.jl:76-93) and the routing decision.  Called for every handle: the spans
// are also what a scalar problem uses (ystart[f] = f) if its regularizers are later replaced by wrapped ones.
int glrm_setup_multi(glrm_handle* h, const glrm_problem* p) {
  std::vector<int64_t> ys((size_t)p->n + 1);
  ys[0] = 0;
  h->dmax = 1;
  h->multi_kmask = 0;
  bool multi = false;
  for (int64_t f = 0; f < p->n; ++f) {
    const glrm_loss& l = p->n_losses == 1 ? p->losses[0] : p->losses[f];
    const int d = l.dim > 1 ? l.dim : 1;
    h->multi_kmask |= l.kind >= GLRM_LOSS_MULTINOMIAL ? (1 << l.kind) : MULTI_KM_SCALAR; // the kinds of the WHOLE model (never the shard's)
    if (d > 1) multi = true;
    if (d > h->dmax) h->dmax = d;
    ys[f + 1] = ys[f] + d;
  }
  h->d = ys[p->n];
  for (int64_t i = 0; i < p->n_rx; ++i) if (p->rx[i].wrap) multi = true;
  for (int64_t i = 0; i < p->n_ry; ++i) if (p->ry[i].wrap) multi = true;
  h->multi = multi;
  if (multi && h->kp > 64)
    return fail(GLRM_ERR_UNSUPPORTED, "multi-dimensional losses / wrapped regularizers need k <= 64 (got %d)", h->k);
  if (multi && p->dense_A)
    return fail(GLRM_ERR_UNSUPPORTED, "the dense hand-over covers scalar QuadLoss with unwrapped regularizers only");
  if (const int rc = h->mem.alloc(&h->ystart, (size_t)p->n + 1)) return rc;
  HIPCK(hipMemcpyAsync(h->ystart, ys.data(), ((size_t)p->n + 1) * 8, hipMemcpyHostToDevice, h->stream));
  HIPCK(hipStreamSynchronize(h->stream)); // ys is a local
  h->ys_cb = ys[p->col_begin];
  return GLRM_OK;
}

// A column longer than one chunk (8192 observations; GLRM_HIP_MULTI_CHUNK overrides, 0 = never) is swept by several
// workgroups.  The chunk is a constant, so the grouping of a column's partial sums depends on its own list only.
int glrm_setup_multi_split(glrm_handle* h) {
  if (h->mtrial || h->col_nsplit < 0) return GLRM_OK;
  const int64_t chunk = knob(Knob::MULTI_CHUNK);
  // split or not is decided from the longest column of the WHOLE problem (glrm_signature) and the global column count, so that every
  // shard of a sharded fit runs the same kernels
  const int64_t longest = h->sig.max_col_len;
  const size_t blk = (size_t)h->dmax * h->kp;
  const int64_t nsplit = chunk > 0 ? (longest + chunk - 1) / chunk : 1;
  if (nsplit <= 1 || nsplit > 65535 || (size_t)h->n * nsplit * blk * 8 > ((size_t)2 << 30)) { h->col_nsplit = -1; return GLRM_OK; }
  h->col_chunk = chunk;
  h->col_nsplit = (int)nsplit;
  int rc;
  if ((rc = h->mem.alloc(&h->mtrial, (size_t)h->d * h->kp)) || (rc = h->mem.alloc(&h->mpart_loss, (size_t)h->side[GLRM_COLS].nseg * nsplit)) ||
      (rc = h->mem.alloc(&h->mpart_G, (size_t)h->side[GLRM_COLS].nseg * nsplit * blk)) || (rc = h->mem.alloc(&h->mgtot, (size_t)h->side[GLRM_COLS].nseg * blk)) ||
      (rc = h->mem.alloc(&h->mobjold, (size_t)h->side[GLRM_COLS].nseg)) || (rc = h->mem.alloc(&h->mactive, (size_t)h->side[GLRM_COLS].nseg)))
    return rc;
  return h->mem.alloc(&h->mnactive, 1);
}

// GDC = 8 when no embedding is wider (gradient registers per lane: 8 instead of 32); TRIG: see LOSS_*_NOTRIG in glrm_engine.hpp
// kind-specialised instantiations (glrm_multi.hpp: MULTI_KM_*) exist for the small-dimension, no-PeriodicLoss variants
static int kind_class(const glrm_handle* h) { // 0 = all kinds, 1 = MultinomialLoss only, 2 = MultinomialLoss + scalar losses, 3 = ordinal
  if (!knob(Knob::MULTI_KINDS)) return 0; // (BvSLoss / MultinomialOrdinalLoss: the columns of an ordinal data frame)
  if (h->multi_kmask == MULTI_KM_MNL) return 1;
  if ((h->multi_kmask & ~(MULTI_KM_MNL | MULTI_KM_SCALAR)) == 0 && (h->multi_kmask & MULTI_KM_MNL)) return 2;
  return h->multi_kmask != 0 && (h->multi_kmask & ~MULTI_KM_ORD) == 0 ? 3 : 0;
}

template <bool GRAD>
static void launch_colpass(bool small, bool trig, int kc, dim3 grid, size_t lds, hipStream_t st, const SplitArgs& sa) {
  constexpr int D = GLRM_MAX_EMBEDDING_DIM;
  if (small) {
    if (trig) hipLaunchKernelGGL((multi_colpass_kernel<GRAD, 8, true>), grid, dim3(512), lds, st, sa);
    else if (kc == 1) hipLaunchKernelGGL((multi_colpass_kernel<GRAD, 8, false, MULTI_KM_MNL>), grid, dim3(512), lds, st, sa);
    else if (kc == 2) hipLaunchKernelGGL((multi_colpass_kernel<GRAD, 8, false, MULTI_KM_MNL | MULTI_KM_SCALAR>), grid, dim3(512), lds, st, sa);
    else if (kc == 3) hipLaunchKernelGGL((multi_colpass_kernel<GRAD, 8, false, MULTI_KM_ORD>), grid, dim3(512), lds, st, sa);
    else hipLaunchKernelGGL((multi_colpass_kernel<GRAD, 8, false>), grid, dim3(512), lds, st, sa);
  } else {
    if (trig) hipLaunchKernelGGL((multi_colpass_kernel<GRAD, D, true>), grid, dim3(512), lds, st, sa);
    else hipLaunchKernelGGL((multi_colpass_kernel<GRAD, D, false>), grid, dim3(512), lds, st, sa);
  }
}

static int run_split_cols(glrm_handle* h, const MultiArgs& a) {
  SplitArgs sa{};
  sa.m = a;
  sa.nsplit = h->col_nsplit;
  sa.chunk = h->col_chunk;
  sa.trial = h->mtrial;
  sa.part_loss = h->mpart_loss; sa.part_G = h->mpart_G; sa.gtot = h->mgtot; sa.objold = h->mobjold;
  sa.active = h->mactive; sa.nactive = h->mnactive;
  const int S = h->kp + 1, sl = 64 >> a.lgP;
  const size_t lds_pass = ((size_t)2 * h->dmax * S + 16 + (size_t)8 * sl * (S + 64)) * 8;
  const size_t lds_dec = ((size_t)2 * h->dmax * S + 64 + 16) * 8;
  const dim3 grid((unsigned)a.nseg, (unsigned)sa.nsplit);
  const bool small = h->dmax <= 8; // gradient registers per lane: 8 instead of 32 -> 4 waves per SIMD instead of 2
  hipStream_t st = h->stream;
  sa.point = a.own;
  if (a.mode == 1) { // losses only
    sa.round = -1;
    launch_colpass<false>(small, h->has_trig, kind_class(h), grid, lds_pass, st, sa);
    MULTI_COLDECIDE(dim3((unsigned)a.nseg), dim3(512), lds_dec, st);
    HIPCK(hipGetLastError());
    return GLRM_OK;
  }
  sa.round = 0;
  HIPCK(hipMemsetAsync(h->mnactive, 0, 4, st));
  launch_colpass<true>(small, h->has_trig, kind_class(h), grid, lds_pass, st, sa);
  MULTI_COLDECIDE(dim3((unsigned)a.nseg), dim3(512), lds_dec, st);
  HIPCK(hipGetLastError());
  if (a.mode == 2) return GLRM_OK;
  sa.point = h->mtrial;
  for (int round = 1; round < 4096; ++round) { // a column makes at most ~13 + log(alpha growth) trials
    unsigned int nact = 0;
    HIPCK(hipMemcpyAsync(&nact, h->mnactive, 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (nact == 0) break;
    sa.round = round;
    HIPCK(hipMemsetAsync(h->mnactive, 0, 4, st));
    launch_colpass<false>(small, h->has_trig, kind_class(h), grid, lds_pass, st, sa);
    MULTI_COLDECIDE(dim3((unsigned)a.nseg), dim3(512), lds_dec, st);
    HIPCK(hipGetLastError());
  }
  return GLRM_OK;
}

int glrm_run_multi(glrm_handle* h, const glrm_step& step) {
  const int side = step.side;
  MultiArgs a{};
  glrm_fill_side(a, h, step);
  a.ystart = h->ystart;
  a.loss_single = h->n_losses == 1;
  a.kp = h->kp; a.dmax = h->dmax;
  a.lgP = 2;
  while ((1 << a.lgP) < h->k || (1 << a.lgP) < h->dmax) ++a.lgP;
  a.mode = step.eval_only ? 1 : (step.fixed() ? 2 : 0);
  if (a.mode != 0) a.trials = a.accepts = nullptr; // the counters belong to the line-search steps
  // the vectors of the side's descriptors (include/glrm_hip_regvec.h), indexed like the descriptors
  a.regvec = h->side[side].regvec;
  a.reglen = h->side[side].reglen;
  a.regvec_single = a.reg_single;
  if (step.ranged()) {
    glrm_apply_row_range(a, step);
    if (a.regvec && !a.reg_single) { a.regvec += step.row_begin * h->k; a.reglen += step.row_begin; }
  }
  if (a.nseg <= 0) return GLRM_OK;
  if (side == GLRM_ROWS) {
    const size_t lds = multi_lds_doubles(true, 1, h->kp, h->dmax, a.lgP) * 8;
    // every embedding dimension <= 8: the opposing block of an observation is held in registers (glrm_multi.hpp: multi_pass, RD)
    const bool regs = h->dmax <= 8 && knob(Knob::MULTI_REGS);
    const int kc = kind_class(h);
    if (regs) {
      if (h->has_trig) MULTI_SWEEP(64, true, 1, GLRM_MAX_EMBEDDING_DIM, true, 8);
      else if (kc == 1) MULTI_SWEEP(64, true, 1, GLRM_MAX_EMBEDDING_DIM, false, 8, MULTI_KM_MNL);
      else if (kc == 2) MULTI_SWEEP(64, true, 1, GLRM_MAX_EMBEDDING_DIM, false, 8, MULTI_KM_MNL | MULTI_KM_SCALAR);
      else if (kc == 3) MULTI_SWEEP(64, true, 1, GLRM_MAX_EMBEDDING_DIM, false, 8, MULTI_KM_ORD);
      else MULTI_SWEEP(64, true, 1, GLRM_MAX_EMBEDDING_DIM, false, 8);
    } else if (h->has_trig) MULTI_SWEEP(64, true, 1, GLRM_MAX_EMBEDDING_DIM, true);
    else MULTI_SWEEP(64, true, 1, GLRM_MAX_EMBEDDING_DIM, false);
  } else {
    if (h->col_nsplit > 1) return run_split_cols(h, a); // (glrm_setup_multi_split decided at set-up whether the columns are long enough to split)
    const size_t lds = multi_lds_doubles(false, 8, h->kp, h->dmax, a.lgP) * 8;
    if (h->dmax <= 8) {
      const int kc = kind_class(h);
      if (h->has_trig) MULTI_SWEEP(512, false, 8, 8, true, 8);
      else if (kc == 1) MULTI_SWEEP(512, false, 8, 8, false, 8, MULTI_KM_MNL);
      else if (kc == 2) MULTI_SWEEP(512, false, 8, 8, false, 8, MULTI_KM_MNL | MULTI_KM_SCALAR);
      else if (kc == 3) MULTI_SWEEP(512, false, 8, 8, false, 8, MULTI_KM_ORD);
      else MULTI_SWEEP(512, false, 8, 8, false, 8);
    } else {
      if (h->has_trig) MULTI_SWEEP(512, false, 8, GLRM_MAX_EMBEDDING_DIM, true);
      else MULTI_SWEEP(512, false, 8, GLRM_MAX_EMBEDDING_DIM, false);
    }
  }
  HIPCK(hipGetLastError());
  return GLRM_OK;
}

int glrm_run_multi_penalty(glrm_handle* h, int side) {
  const glrm_handle::Side& v = h->side[side];
  if (v.nseg <= 0) return GLRM_OK;
  PenaltyArgs a{};
  a.nseg = v.nseg; a.own = v.factor; a.own_offset = v.begin; a.out = v.obj;
  a.ystart = side == GLRM_ROWS ? nullptr : h->ystart; // (a row is one vector, a column its block of Y)
  a.regs = v.regs; a.reg_single = a.regvec_single = v.n_regs == 1;
  a.k = h->k; a.kp = h->kp;
  a.vecreg = v.vecreg ? 1 : 0; a.regvec = v.regvec; a.reglen = v.reglen;
  const size_t lds = ((size_t)(side == GLRM_ROWS ? 1 : h->dmax) * (h->kp + 1) + 16) * 8;
  if (a.vecreg) hipLaunchKernelGGL(multi_penalty_kernel<true>, dim3((unsigned)a.nseg), dim3(64), lds, h->stream, a);
  else hipLaunchKernelGGL(multi_penalty_kernel<false>, dim3((unsigned)a.nseg), dim3(64), lds, h->stream, a);
  HIPCK(hipGetLastError());
  return GLRM_OK;
}
