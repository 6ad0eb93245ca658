// glrm_launch.hpp -- the host-side launch layer the run functions of every sweep family go through: describing one side of a half-step in
// a kernel-argument struct, the pass buffers of a side, the line-search rounds of the multi-pass families, and the ladders from run-time
// layout / loss variant to template arguments.  Templates over the argument struct that assign by field name: SweepArgs, TiledArgs,
// CachedArgs, MultiArgs and RefArgs keep their own member lists (they are what the device code reads).  Host code only.
#pragma once

#include <type_traits>

#include "glrm_engine.hpp"

// ------------------------------------------------------------------ one side of a half-step

namespace glrm_detail {
// fields only some of the argument structs have: assigned where present (the int overload is preferred and drops out by SFINAE)
template <class A, class V> auto set_obj(A& a, V v, int) -> decltype(void(a.obj = v)) { a.obj = v; }
template <class A, class V> void set_obj(A&, V, long) {}
template <class A, class V> auto set_n_other(A& a, V v, int) -> decltype(void(a.n_other = v)) { a.n_other = v; }
template <class A, class V> void set_n_other(A&, V, long) {}
template <class A, class V> auto set_eval_only(A& a, V v, int) -> decltype(void(a.eval_only = v)) { a.eval_only = v; }
template <class A, class V> void set_eval_only(A&, V, long) {}
template <class A, class V> auto set_fixed_alpha(A& a, V v, int) -> decltype(void(a.fixed_alpha = v)) { a.fixed_alpha = v; }
template <class A, class V> void set_fixed_alpha(A&, V, long) {}
template <class A, class V> auto set_vecreg(A& a, V v, int) -> decltype(void(a.vecreg = v)) { a.vecreg = v; }
template <class A, class V> void set_vecreg(A&, V, long) {}
} // namespace glrm_detail

// The view, factors, step sizes, descriptors and counters of the side the request names (rows: X half-step, columns: Y half-step), and
// the request's own min_stepsize / eval_only / fixed step.  What a family does differently (nullable trials, its own mode fields, the
// loss variant) follows at the call site.
template <class A>
void glrm_fill_side(A& a, const glrm_handle* h, const glrm_step& step) {
  const int side = step.side;
  const glrm_handle::Side& v = h->side[side];
  a.nseg = v.nseg;
  a.ptr = v.ptr;
  a.idx = v.idx;
  a.vals = v.vals;
  a.own = v.factor;
  a.own_offset = v.begin;
  a.other = h->side[side ^ 1].factor;
  a.alpha = v.alpha;
  a.losses = h->losses;
  a.regs = v.regs;
  a.reg_single = v.n_regs == 1;
  glrm_detail::set_vecreg(a, v.vecreg ? 1 : 0, 0);
  a.k = h->k;
  a.min_stepsize = step.min_stepsize;
  a.trials = v.trials;
  a.accepts = v.accepts;
  glrm_detail::set_obj(a, side == GLRM_ROWS ? nullptr : v.obj, 0);
  glrm_detail::set_n_other(a, h->side[side ^ 1].nglob, 0);
  glrm_detail::set_eval_only(a, step.eval_only ? 1 : 0, 0);
  glrm_detail::set_fixed_alpha(a, step.fixed() ? step.fixed_alpha : 0.0, 0);
}

// glrm_hip_step_x_range: the description restricted to the request's local rows [row_begin, row_end) (the caller asks step.ranged() first
// and returns when a.nseg <= 0)
template <class A>
void glrm_apply_row_range(A& a, const glrm_step& step) {
  const int64_t rng_b = step.row_begin;
  a.nseg = step.row_end - rng_b;
  a.ptr += rng_b; a.alpha += rng_b; a.own_offset += rng_b;
  if (!a.reg_single) a.regs += rng_b;
  if (a.trials) a.trials += rng_b;
  if (a.accepts) a.accepts += rng_b;
}

// points the pass-buffer fields of a TiledArgs at a side's buffers (GLRM_ROWS / GLRM_COLS), from local segment s0 on
template <class A>
void glrm_bind_pass_buffers(A& a, const glrm_handle* h, int side, int64_t s0 = 0) {
  const glrm_handle::PassBuffers& b = h->side[side].pass;
  a.nsup = b.nsup;
  a.tiles_per_sup = b.tiles_per_sup;
  a.part = b.part + s0 * (int64_t)b.nsup * (h->kp + 2);
  a.gsum = b.gsum + s0 * (int64_t)h->kp;
  a.trial = b.trial + s0 * (int64_t)h->kp;
  a.jold = b.jold + s0;
  a.active = b.active + s0;
  a.ntrial = b.ntrial + s0;
  a.suppos = b.suppos ? b.suppos + s0 * (int64_t)b.nsup : nullptr;
  a.nactive = h->nactive;
}

// ------------------------------------------------------------------ line-search rounds

// the two lists of still-searching segments the decide kernel reads and writes in turn (TiledArgs::actlist_in / actlist_out); both
// nullptr where the side runs without lists
struct glrm_act_lists {
  int32_t* list[2] = {nullptr, nullptr};
};
inline glrm_act_lists glrm_active_lists(const glrm_handle* h, int side, int64_t nseg) {
  glrm_act_lists l;
  if (h->actlist && (h->tile_rounds & (1 << side)) && nseg <= h->actlist_cap) {
    l.list[0] = h->actlist;
    l.list[1] = h->actlist + h->actlist_cap;
  }
  return l;
}

// A segment leaves the search when a trial is accepted or its step size is no longer above min_stepsize (`while alpha > min_stepsize`,
// proxgrad.jl:136,180): at most log(alpha / min_stepsize) / log(1 / 0.7) rounds (13 from alpha = 1 and the default 0.01).  With
// min_stepsize = 0 a search whose trials are all rejected never ends in the reference either: 0.7 x 4.9e-324 rounds back to 4.9e-324,
// alpha never reaches 0 (~2 090 rounds from alpha = 1 to the smallest denormal, then forever).  The bound is a guard against exactly that
// loop, never a silent cut: running into it is an error where the reference would hang.
constexpr int GLRM_MAX_ROUNDS = 4096;

// Rounds of (trial pass, decide) until no segment is still searching: the count is read back once per round.
//   trial(round, nact, list) -> int   launches the round's trial pass; `list` holds the nact searching segments (nullptr without lists)
//   decide(d)                         launches the decide kernel on d = `full` with this round's lists set
template <class A, class Trial, class Decide>
int glrm_run_rounds(glrm_handle* h, const A& full, double min_stepsize, const glrm_act_lists& lists, Trial&& trial, Decide&& decide) {
  int cur = 0; // the list the previous stage appended to
  for (int round = 0;; ++round) {
    if (round == GLRM_MAX_ROUNDS) return fail(GLRM_ERR_INVALID, "line search still running after %d rounds (min_stepsize %g)", GLRM_MAX_ROUNDS, min_stepsize);
    unsigned int nact = 0;
    HIPCK(hipMemcpyAsync(&nact, h->nactive, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    if (nact == 0) break;
    HIPCK(hipMemsetAsync(h->nactive, 0, 4, h->stream));
    const int rc = trial(round, nact, lists.list[cur]);
    if (rc) return rc;
    A d = full;
    if (lists.list[0]) {
      d.actlist_in = lists.list[cur];
      d.nact_in = nact;
      d.actlist_out = lists.list[cur ^ 1];
      cur ^= 1;
    }
    decide(d);
    HIPCK(hipGetLastError());
  }
  return GLRM_OK;
}

// ------------------------------------------------------------------ run-time value -> template argument

template <int V>
using glrm_const = std::integral_constant<int, V>;

// f(glrm_const<V>{}) for the V of the list that equals v, otherwise() for a value outside it; returns what the call returns.  The list
// is the set of instantiations the site asks for: nothing outside it is compiled.
template <int... V, class F, class Else>
int glrm_dispatch(int v, F&& f, Else&& otherwise) {
  int rc = GLRM_OK;
  const bool hit = ((v == V ? (rc = f(glrm_const<V>{}), true) : false) || ...);
  return hit ? rc : otherwise();
}

// lane layout (lanes per observation G, components per lane R) of a padded rank: pick_layout's table
constexpr int glrm_layout_g(int kp) { return kp <= 32 ? 4 : kp / 8; }
constexpr int glrm_layout_r(int kp) { return kp / glrm_layout_g(kp); }

// f(glrm_const<G>{}, glrm_const<R>{}) for the padded rank of the list whose layout is (G, R)
template <int... KP, class F, class Else>
int glrm_dispatch_layout(int G, int R, F&& f, Else&& otherwise) {
  int rc = GLRM_OK;
  const bool hit = ((G == glrm_layout_g(KP) && R == glrm_layout_r(KP) ? (rc = f(glrm_const<glrm_layout_g(KP)>{}, glrm_const<glrm_layout_r(KP)>{}), true) : false) || ...);
  return hit ? rc : otherwise();
}
