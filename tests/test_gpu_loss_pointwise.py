"""-m gpu: every loss formula of the device, point by point, against exact references (tests/loss_ref.py; test build only).

The hooks glrm_test_loss_pointwise and glrm_test_obs_loss (csrc/glrm_testhooks.hip) call the kernels' own device functions -- loss_both in its
four instantiations, the primitives of csrc/glrm_fastmath.hpp, obs_loss under the four kind masks glrm_multi.hip instantiates -- on the point
sets of tests/loss_ref.py; neighbouring lanes hold different kinds, neighbouring slots different kinds and widths.

  1. Quad, L1, Huber, Quantile, OrdinalHinge, WeightedHinge: value and gradient EQUAL the oracle's (`==`, same NaN positions) on the bulk and on
     every kink, branch boundary, +-0, tiny, huge and non-finite point.
  2. The gradient pass and the trial pass return one L: loss_both<true, .> and <false, .>, obs_loss<true> and <false>, bit for bit.
  3. TRIG = false has TRIG = true's bits for every kind but Periodic, and NaN for Periodic.
  4. fm_exp, fm_log_ge1, fm_log, fm_rcp on the device at the bounds of tests/test_fastmath.py (2.5e-16, 5e-16 relative), fm_rcp < 2^-52 on
     [1, 3], denormal exp results within two denormal spacings and never flushed to zero, special values by class.
  5. LogisticLoss: L is 0 / +Inf / NaN exactly where the oracle's literal formula is; elsewhere L is scale * log(w') to 5e-16 for a w' among
     fl(1 + fl(exp(-z))) and its two neighbours; the derivative to 6e-16 against the exact one and in its class (-+scale, +-0) where the exact
     derivative rounds to that class; test/loss_test.jl's two known answers to the last digit.
     DEVIATION from the oracle's class, asserted as such: device and oracle derivatives of a saturated class differ ONLY for z inside
     (-37.43, -36.73) and (709.78, 745.14), and there only as the double next to -+scale or a value below scale 2^-1024 of the same sign.
     The oracle's literal -aa s / (1 + exp(aa u)) reaches the classes EARLIER than the function does -- for z in (-37.43, -36.74) its
     1 + exp(z) already rounds to 1, for z in (709.78, 745.13) its exp(z) is already Inf -- and there the device returns the correctly rounded
     derivative (scale (1 - 2^-53), a denormal; the zero class is taken where the exact derivative is below a quarter of the smallest denormal): the derivative comes from the ONE exponential (csrc/glrm_fastmath.hpp) and is only ever summed.
  6. Periodic, Poisson, Logistic and the five multi-dimensional kinds: the largest error per bucket, in ulps of the exact value, is at most
     4 x the oracle's largest error on the same bucket + 2 (loss_ref.device_bound; the oracle's maxima are measured on the CPU by
     tests/test_loss_ref.py).  obs_loss at every slot width that holds the dimension; a kind-specialised mask has MULTI_KM_ALL's bits;
     d = 1 through obs_loss has loss_both's bits; every slot of a mixed wave gives what its observation gives alone in a wave.
  7. The bucket maxima of Periodic, Poisson and Logistic are those of the worst-conditioned point of the bucket (1 - cos(w) next to a zero, a
     Poisson loss that cancels, log(1 + E) for a small E), for the oracle and the device alike.  So the three kinds are ALSO held next to
     the oracle: the same expression on the same doubles with another exp / log / cos / sin differs by at most 8 ulps of the largest value
     the formula passes through (loss_ref.computation_scale), at every point.  The five multi-dimensional kinds likewise
     (loss_ref.multi_computation_scale, 8 + d ulps): that is the check that bites on the special buckets, whose maxima are set by a
     dominant category or a clamped threshold.

Measured (MI355X; ulps of the exact value; `pytest -s` prints the whole table, LABNOTES.md "Pointwise loss errors" keeps it):
largest error per bucket, oracle (CPU, libm) and device; multi-dimensional buckets: the largest over the slot widths
bucket                               oracle L   device L  oracle dL  device dL
Periodic/bulk                        7.53e+06   7.53e+06   1.05e+05   1.05e+05
Poisson/bulk                            2e+08      2e+08   1.08e+03   1.08e+03
Logistic/bulk                        4.29e+12   4.29e+12       1.81       2.74
Logistic/saturation                       inf        inf   1.12e+15       1.52
Poisson/cancellation                 1.62e+32   1.62e+32   7.53e+15   7.53e+15
Periodic/large                       1.19e+88   1.19e+88   8.77e+51   8.77e+51
Multinomial/d2/bulk                  8.61e+03   8.62e+03   6.23e+03   6.23e+03
Multinomial/d2/special               6.82e+15   6.82e+15   6.82e+15   6.82e+15
OvA/d2/bulk                              49.8       50.8       1.93       2.79
OvA/d2/special                          0.338      0.338      0.455      0.455
BvS/d2/bulk                              26.1       26.1       2.14       2.65
BvS/d2/special                       7.86e+15   7.86e+15      0.576       1.03
Ordistic/d2/bulk                     6.71e+15   6.71e+15   8.39e+15   8.39e+15
Ordistic/d2/special                   5.5e+15    5.5e+15   8.59e+15   8.59e+15
MultinomialOrdinal/d2/bulk           1.43e+03   1.43e+03   4.07e+03   4.07e+03
MultinomialOrdinal/d2/special         8.2e+15    8.2e+15   2.08e+05   2.08e+05
Multinomial/d3/bulk                       517        517        389        389
Multinomial/d3/special               6.82e+15   6.82e+15   6.82e+15   6.82e+15
OvA/d3/bulk                              5.76       4.78          2       2.45
OvA/d3/special                          0.753      0.753       1.16       1.03
BvS/d3/bulk                              6.64       6.64       2.35       2.69
BvS/d3/special                            1.5        1.5      0.455       1.03
Ordistic/d3/bulk                     2.58e+04   2.58e+04   1.27e+04   1.27e+04
Ordistic/d3/special                   5.5e+15    5.5e+15   8.59e+15   8.59e+15
MultinomialOrdinal/d3/bulk                358        579   4.33e+03   5.88e+03
MultinomialOrdinal/d3/special         8.2e+15    8.2e+15   2.08e+05   2.08e+05
Multinomial/d4/bulk                       750        750   1.19e+03   1.19e+03
Multinomial/d4/special               8.27e+15   8.27e+15   8.27e+15   8.27e+15
OvA/d4/bulk                               5.8        3.8       2.22       2.57
OvA/d4/special                           1.06      0.753       1.16       1.15
BvS/d4/bulk                              4.21       4.21          2       2.71
BvS/d4/special                       4.77e+15   4.77e+15      0.455      0.942
Ordistic/d4/bulk                          385        385        702        702
Ordistic/d4/special                   5.5e+15    5.5e+15   8.59e+15   8.59e+15
MultinomialOrdinal/d4/bulk                345        464   3.91e+03   5.95e+03
MultinomialOrdinal/d4/special         8.2e+15    8.2e+15   2.08e+05   7.92e+05
Multinomial/d5/bulk                       459        459        359        359
Multinomial/d5/special               6.82e+15   6.82e+15   6.82e+15   6.82e+15
OvA/d5/bulk                              2.81       2.81       2.08       2.74
OvA/d5/special                           1.76       1.76      0.455       1.15
BvS/d5/bulk                              3.65       4.12       2.15       2.86
BvS/d5/special                       6.45e+15   6.45e+15       1.16       1.15
Ordistic/d5/bulk                         40.2       37.2       38.8       38.8
Ordistic/d5/special                  6.34e+15   6.34e+15   8.59e+15   8.59e+15
MultinomialOrdinal/d5/bulk                390        521   4.03e+03   6.24e+03
MultinomialOrdinal/d5/special         8.2e+15    8.2e+15   2.08e+05   7.92e+05
Multinomial/d8/bulk                      35.7         34       38.9       38.6
Multinomial/d8/special               5.97e+15   5.97e+15   5.97e+15   5.97e+15
OvA/d8/bulk                              3.55       2.11       2.17       2.91
OvA/d8/special                           4.99      0.989       1.16       1.15
BvS/d8/bulk                              2.74       2.02       2.29       2.65
BvS/d8/special                       6.82e+15   6.82e+15      0.455       1.15
Ordistic/d8/bulk                         3.79       2.34       23.5       23.9
Ordistic/d8/special                   5.5e+15    5.5e+15   8.59e+15   8.59e+15
MultinomialOrdinal/d8/bulk                365        590   4.41e+03   6.43e+03
MultinomialOrdinal/d8/special         8.2e+15    8.2e+15   2.08e+05   7.92e+05
Multinomial/d9/bulk                      83.3        171        101        188
Multinomial/d9/special               6.82e+15   6.82e+15   6.82e+15   6.82e+15
OvA/d9/bulk                              2.75        2.4       2.38       2.89
OvA/d9/special                           5.06       1.06       1.16       1.15
BvS/d9/bulk                              2.56       2.69       2.09       2.78
BvS/d9/special                           3.06       1.14      0.455       1.15
Ordistic/d9/bulk                         2.42       2.54         20       30.2
Ordistic/d9/special                   5.5e+15    5.5e+15   8.59e+15   8.59e+15
MultinomialOrdinal/d9/bulk                393        574   5.45e+03   6.42e+03
MultinomialOrdinal/d9/special         8.2e+15    8.2e+15   2.08e+05   7.92e+05
Multinomial/d16/bulk                      109       31.5        118       20.1
Multinomial/d16/special              6.39e+15   6.39e+15   6.39e+15   6.39e+15
OvA/d16/bulk                             2.96       1.86       2.22       2.93
OvA/d16/special                           7.6       1.05       1.16       1.15
BvS/d16/bulk                             3.88       2.43       2.22       2.98
BvS/d16/special                      4.54e+15   4.54e+15      0.821       1.03
Ordistic/d16/bulk                        2.12       2.24       20.4       27.8
Ordistic/d16/special                  5.5e+15    5.5e+15   8.59e+15   8.59e+15
MultinomialOrdinal/d16/bulk               396        558   5.87e+03   6.26e+03
MultinomialOrdinal/d16/special        8.2e+15    8.2e+15   2.09e+05   7.93e+05
Multinomial/d17/bulk                     26.8       11.8       26.3       10.4
Multinomial/d17/special              6.82e+15   6.82e+15   6.82e+15   6.82e+15
OvA/d17/bulk                             3.65       2.84       2.23       2.92
OvA/d17/special                          9.68       1.39       1.16       1.15
BvS/d17/bulk                             3.44       2.38       2.38          3
BvS/d17/special                      5.07e+15   5.07e+15      0.821       1.15
Ordistic/d17/bulk                        2.17       2.07       32.7       40.7
Ordistic/d17/special                  5.5e+15    5.5e+15   8.59e+15   8.59e+15
MultinomialOrdinal/d17/bulk               400        577   4.53e+03   6.58e+03
MultinomialOrdinal/d17/special        8.2e+15    8.2e+15   2.09e+05   7.93e+05
Multinomial/d31/bulk                     38.1       28.5       41.7       21.8
Multinomial/d31/special              6.39e+15   6.39e+15   6.39e+15   6.39e+15
OvA/d31/bulk                             3.46       2.15       2.49       2.76
OvA/d31/special                          20.7       1.16       1.16       1.15
BvS/d31/bulk                             3.89       2.49       2.43       3.18
BvS/d31/special                      4.63e+15   4.63e+15       1.05       1.15
Ordistic/d31/bulk                        2.34       2.02       28.2       34.7
Ordistic/d31/special                  5.5e+15    5.5e+15   8.59e+15   8.59e+15
MultinomialOrdinal/d31/bulk               377        546   4.81e+03    7.9e+03
MultinomialOrdinal/d31/special        8.2e+15    8.2e+15   2.09e+05   7.93e+05
Multinomial/d32/bulk                       22       3.57       16.4       10.7
Multinomial/d32/special              6.61e+15   6.61e+15   6.61e+15   6.61e+15
OvA/d32/bulk                              4.5       1.96       2.27       3.52
OvA/d32/special                          20.8       1.29       1.16       1.15
BvS/d32/bulk                             4.07        2.1       2.37       3.47
BvS/d32/special                      4.77e+15   4.77e+15       1.05       1.15
Ordistic/d32/bulk                        2.44       2.13       23.2       30.6
Ordistic/d32/special                  5.5e+15    5.5e+15   8.59e+15   8.59e+15
MultinomialOrdinal/d32/bulk               384        562   5.87e+03   7.93e+03
MultinomialOrdinal/d32/special        8.2e+15    8.2e+15   2.09e+05   7.93e+05
primitives, relative error against the exact value
fm_exp/range             n  20000  device max rel err 1.28e-16
fm_exp/logistic-range    n   4000  device max rel err 1.3e-16
fm_exp/denormal          n   2000  device max rel err 8.96e-17
fm_exp/special           n     23  device max rel err 9.77e-17
fm_log_ge1/near-1        n  10000  device max rel err 3.45e-16
fm_log_ge1/range         n  10000  device max rel err 1.4e-16
fm_log_ge1/special       n      9  device max rel err 1.11e-16
fm_log/unit              n   8000  device max rel err 3.38e-16
fm_log/exponents         n   8000  device max rel err 1.59e-16
fm_log/below-1           n   4000  device max rel err 3.19e-16
fm_log/special           n     11  device max rel err 5.94e-17
fm_rcp/1-3               n  20006  device max rel err 1.1e-16
|device - oracle| in ulps of the computation's scale
Periodic/bulk            L  n  20000  largest |device - oracle|: 2 ulp of the scale
Periodic/bulk            dL n  20000  largest |device - oracle|: 1 ulp of the scale
Poisson/bulk             L  n  20000  largest |device - oracle|: 2 ulp of the scale
Poisson/bulk             dL n  20000  largest |device - oracle|: 1 ulp of the scale
Logistic/bulk            L  n  20000  largest |device - oracle|: 2 ulp of the scale
Logistic/bulk            dL n  20000  largest |device - oracle|: 1 ulp of the scale
Logistic/saturation      L  n    820  largest |device - oracle|: 6.94e-18 ulp of the scale
Logistic/saturation      dL n    964  largest |device - oracle|: 1 ulp of the scale
Poisson/cancellation     L  n     63  largest |device - oracle|: 0 ulp of the scale
Poisson/cancellation     dL n     63  largest |device - oracle|: 0 ulp of the scale
Periodic/large           L  n    168  largest |device - oracle|: 0 ulp of the scale
Periodic/large           dL n    168  largest |device - oracle|: 0 ulp of the scale
d 2: largest |device - oracle| in ulps of the scale: L 4, grad 2 (allowed 10)
d 3: largest |device - oracle| in ulps of the scale: L 3, grad 2 (allowed 11)
d 4: largest |device - oracle| in ulps of the scale: L 4, grad 2 (allowed 12)
d 5: largest |device - oracle| in ulps of the scale: L 4, grad 2 (allowed 13)
d 8: largest |device - oracle| in ulps of the scale: L 5, grad 2 (allowed 16)
d 9: largest |device - oracle| in ulps of the scale: L 6, grad 3 (allowed 17)
d 16: largest |device - oracle| in ulps of the scale: L 10, grad 3 (allowed 24)
d 17: largest |device - oracle| in ulps of the scale: L 9, grad 2 (allowed 25)
d 31: largest |device - oracle| in ulps of the scale: L 20, grad 2.78 (allowed 39)
d 32: largest |device - oracle| in ulps of the scale: L 21, grad 3.94 (allowed 40)
"""
import ctypes as C
import functools

import numpy as np
import pytest

import loss_ref as R
from lowrankmodels.jl_amd import _capi

pytestmark = pytest.mark.gpu
LD = R.LD
KM_KINDS = {1: {R.MULTINOMIAL}, 2: {R.MULTINOMIAL, "scalar"}, 3: {R.BVS, R.MULTINOMIAL_ORDINAL}}


# ---------------------------------------------------------------------------------------------------------------- the hooks

def pointwise(desc, u, a, op=0):
    fn = _capi.hip_testing_api().lib.glrm_test_loss_pointwise
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    u = np.ascontiguousarray(u, dtype=np.float64)
    n, nout = len(u), 4 if op == 0 else 1
    desc = None if desc is None else np.ascontiguousarray(desc)
    a = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    L, dL = np.full((nout, n), 7.0), np.full((nout, n), 7.0)
    rc = fn(None if desc is None else desc.ctypes.data, u.ctypes.data, None if a is None else a.ctypes.data, n, op, L.ctypes.data, dL.ctypes.data)
    assert rc == 0, (rc, _capi.hip_testing_api().last_error())
    return (L, dL) if op == 0 else (L[0], dL[0])


def obs_loss(desc, d, level, U, lg, km):
    """U: n x 2^lg.  Returns Lg, G, Lt (n x 2^lg)"""
    fn = _capi.hip_testing_api().lib.glrm_test_obs_loss
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    desc, d = np.ascontiguousarray(desc), np.ascontiguousarray(d, dtype=np.int32)
    level, U = np.ascontiguousarray(level, dtype=np.float64), np.ascontiguousarray(U, dtype=np.float64)
    n, P = len(d), 1 << lg
    assert U.shape == (n, P)
    out = [np.full((n, P), 7.0) for _ in range(3)]
    rc = fn(desc.ctypes.data, d.ctypes.data, level.ctypes.data, U.ctypes.data, n, lg, km, *(o.ctypes.data for o in out))
    assert rc == 0, (rc, _capi.hip_testing_api().last_error())
    return out


def same_bits(x, y):
    """equal as doubles, zeros by sign, NaN where NaN"""
    x, y = np.asarray(x), np.asarray(y)
    return (x.shape == y.shape) and bool(np.all(((x == y) & (np.signbit(x) == np.signbit(y))) | (np.isnan(x) & np.isnan(y))))


def widen(U, P):
    out = np.zeros((len(U), P))
    out[:, :U.shape[1]] = U
    return out


# ---------------------------------------------------------------------------------------------------------------- the scalar batch

@functools.lru_cache(maxsize=None)
def scalar_run():
    """ONE launch per instantiation over every scalar bucket, the points shuffled so that a wave holds all kinds side by side.
    name -> (L (4, n), dL (4, n)) in the bucket's own order."""
    bs = R.scalar_buckets()
    desc = np.concatenate([b.desc for b in bs])
    u, a = np.concatenate([b.u for b in bs]), np.concatenate([b.a for b in bs])
    perm = np.random.default_rng(5).permutation(len(u))
    L, dL = pointwise(desc[perm], u[perm], a[perm])
    Lo, dLo = np.empty_like(L), np.empty_like(dL)
    Lo[:, perm], dLo[:, perm] = L, dL
    out, at = {}, 0
    for b in bs:
        out[b.name] = (Lo[:, at:at + len(b.u)], dLo[:, at:at + len(b.u)])
        at += len(b.u)
    return out


SCALAR_NAMES = [b.name for b in R.scalar_buckets()]
EXACT_NAMES = [b.name for b in R.scalar_buckets() if b.kind in R.EXACT_KINDS]
MEASURED_NAMES = [b.name for b in R.scalar_buckets() if b.kind not in R.EXACT_KINDS]


@pytest.mark.parametrize("name", EXACT_NAMES)
def test_piecewise_kinds_equal_the_oracle(name):
    b, eL, eG, idx, oL, oG = R.scalar_reference(name)
    L, dL = scalar_run()[name]
    for got, want, what in ((L[0][idx], oL, "L"), (dL[0][idx], oG, "dL")):
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        assert not bad.any(), (name, what, b.desc[idx][bad][:3], b.u[idx][bad][:3], b.a[idx][bad][:3], got[bad][:3], want[bad][:3])


@pytest.mark.parametrize("name", SCALAR_NAMES)
def test_both_passes_return_one_loss_and_notrig_changes_only_periodic(name):
    b = {x.name: x for x in R.scalar_buckets()}[name]
    L, dL = scalar_run()[name]
    assert same_bits(L[0], L[1]) and same_bits(L[2], L[3]), name           # <true, .> against <false, .>
    assert np.all(dL[1] == 0.0) and (b.kind == R.PERIODIC or np.all(dL[3] == 0.0))
    if b.kind == R.PERIODIC:
        assert np.all(np.isnan(L[2])) and np.all(np.isnan(dL[2])) and np.all(np.isnan(L[3])), name
        assert not np.all(np.isnan(L[0]))
    else:
        assert same_bits(L[2], L[0]) and same_bits(dL[2], dL[0]), name


def _print(name, n, oracle, device, bound):
    print("%-34s n %6d  L: oracle %-9.3g device %-9.3g (bound %-9.3g)  grad: oracle %-9.3g device %-9.3g (bound %-9.3g)"
          % (name, n, oracle[0], device[0], bound[0], oracle[1], device[1], bound[1]))


def _held_to_the_bucket_bound(name, b, eL, eG, oL, oG, L, G):
    """the device's largest error against 4 x the oracle's + 2 ulp; by class where the exact value is not finite"""
    so, sd = R.error_stats(oL, oG, eL, eG), R.error_stats(L, G, eL, eG)
    bound = (R.device_bound(so.max_L), R.device_bound(so.max_G))
    _print(name, so.n, (so.max_L, so.max_G), (sd.max_L, sd.max_G), bound)
    assert sd.max_L <= bound[0] and sd.max_G <= bound[1], (name, so, sd)
    for got, orc, ex in ((L, oL, eL), (G, oG, eG)):
        out = ~R.ulps(np.ravel(got), np.ravel(ex))[1]
        assert np.array_equal(R.classes(np.ravel(got))[out], R.classes(np.ravel(orc))[out]), name
    return so, sd


@pytest.mark.parametrize("name", MEASURED_NAMES)
def test_transcendental_scalar_kinds_within_the_bucket_bound(name):
    b, eL, eG, idx, oL, oG = R.scalar_reference(name)
    L, dL = scalar_run()[name]
    _held_to_the_bucket_bound(name, b, eL, eG, oL, oG, L[0][idx], dL[0][idx])


@pytest.mark.parametrize("name", MEASURED_NAMES)
def test_transcendental_scalar_kinds_stay_next_to_the_oracle(name):
    """device against oracle, in ulps of the computation's scale (loss_ref.computation_scale): sharp where the bucket bound is not"""
    b, eL, eG, idx, oL, oG = R.scalar_reference(name)
    L, dL = (x[0][idx] for x in scalar_run()[name])
    ML, MG = R.computation_scale(b, idx)
    for got, orc, M, what in ((L, oL, ML, "L"), (dL, oG, MG, "dL")):
        both = np.isfinite(got) & np.isfinite(orc) & np.isfinite(M)
        with np.errstate(all="ignore"):
            off = np.abs(got - orc) / R.ulp(M)
        print("%-24s %-2s n %6d  largest |device - oracle|: %.3g ulp of the scale" % (name, what, both.sum(), off[both].max(initial=0.0)))
        bad = both & ~(off <= R.SCALE_ULPS)
        assert not bad.any(), (name, what, b.u[idx][bad][:4], b.a[idx][bad][:4], got[bad][:4], orc[bad][:4], off[bad][:4])
        assert both.mean() >= (0.98 if not b.special else 0.5), (name, what, both.mean())


# ---------------------------------------------------------------------------------------------------------------- primitives

@pytest.mark.parametrize("name", [b.name for b in R.primitive_buckets()])
def test_primitives_on_the_device(name):
    b = {x.name: x for x in R.primitive_buckets()}[name]
    got, _ = pointwise(None, b.x, None, op=b.op)
    bad, worst = R.primitive_failures(b, got)
    print("%-24s n %6d  device max rel err %.3g" % (b.name, len(b.x), worst))
    assert len(bad) == 0, (b.name, b.x[bad][:5], got[bad][:5])


def test_primitive_special_values():
    nan, inf = float("nan"), float("inf")
    e, _ = pointwise(None, np.array([800.0, -800.0, nan, 0.0, -0.0, inf, -inf]), None, op=1)
    assert e[0] == inf and e[1] == 0.0 and np.isnan(e[2]) and e[3] == 1.0 and e[4] == 1.0 and e[5] == inf and e[6] == 0.0
    g, _ = pointwise(None, np.array([0.0, -1.0, inf, nan, 1.0]), None, op=3)
    assert g[0] == -inf and np.isnan(g[1]) and g[2] == inf and np.isnan(g[3]) and g[4] == 0.0 and not np.signbit(g[4])
    w, _ = pointwise(None, np.array([1.0, inf, nan]), None, op=2)
    assert w[0] == 0.0 and w[1] == inf and np.isnan(w[2])
    r, _ = pointwise(None, np.array([1.0, 2.0, 3.0]), None, op=4)
    assert np.all(np.abs(r * np.array([1.0, 2.0, 3.0]) - 1.0) < 2.0 ** -52)


# ---------------------------------------------------------------------------------------------------------------- LogisticLoss

#: z = (2a - 1) u between which the oracle's literal derivative -aa s / (1 + exp(z)) is already in its class and the function is not:
#: 1 + exp(z) rounds to 1 from exp(z) <= 2^-53 (z <= -36.7368) while 1 - 1 / (1 + exp(-z)) rounds to 1 only from z <= -37.4299; exp(z) is Inf
#: from z > 709.7827 while scale exp(-z) rounds to 0 only beyond z = 745.14
EARLY_ONE, EARLY_ZERO = (-37.43, -36.73), (709.78, 745.14)


def test_logistic_structure():
    nearest = 0
    for name in ("Logistic/bulk", "Logistic/saturation"):
        b, eL, eG, idx, oL, oG = R.scalar_reference(name)
        L, dL = (x[0][idx] for x in scalar_run()[name])
        s, aa, u = b.desc["scale"][idx], 2 * b.a[idx] - 1, b.u[idx]
        z = aa * u
        assert np.array_equal(L == 0.0, oL == 0.0) and not np.any(np.signbit(L[L == 0.0])), name
        assert np.array_equal(L == np.inf, oL == np.inf) and np.array_equal(np.isnan(L), np.isnan(oL)), name
        assert np.array_equal(np.isnan(dL), np.isnan(oG)), name
        # elsewhere: scale * log(w') for a w' among fl(1 + fl(exp(-z))) and its neighbours, exp exact
        open_ = np.isfinite(L) & (L != 0.0)
        with np.errstate(all="ignore"):
            E = np.exp(-z[open_].astype(LD)).astype(np.float64)
            w = 1.0 + E
            cands = np.stack([w, np.nextafter(w, np.inf), np.maximum(np.nextafter(w, -np.inf), 1.0)])
            target = s[open_].astype(LD) * np.log(cands.astype(LD))
            rel = np.where(target != 0, np.abs((L[open_].astype(LD) - target) / np.where(target != 0, target, LD(1))), LD(np.inf))
            best = rel.min(axis=0).astype(np.float64)
        assert np.all(best < R.LOG_REL), (name, z[open_][~(best < R.LOG_REL)][:5], best[~(best < R.LOG_REL)][:5])
        # the derivative: to 6e-16 against the exact one where that is a normal double, within two denormal spacings below, and in the
        # class (-+scale, +-0) where the exact derivative rounds to the class
        fin = ~np.isnan(z)
        with np.errstate(all="ignore"):
            ex = eG[fin]
            got, orc, sc = dL[fin], oG[fin], s[fin]
            e64 = ex.astype(np.float64)
            normal = np.abs(e64) >= 2.0 ** -1022
            rel = np.abs((got.astype(LD) - ex) / np.where(ex != 0, ex, LD(1))).astype(np.float64)
            assert np.all(rel[normal] < R.DLOGISTIC_REL), (name, z[fin][normal][~(rel[normal] < R.DLOGISTIC_REL)][:5])
            assert np.all(np.abs(got.astype(LD) - ex)[~normal] <= LD(R.DENORMAL_SPACINGS * 2.0 ** -1074)), name
            one = np.abs(ex) >= sc.astype(LD) * (LD(1) - LD(2.0) ** -54)   # rounds to -+scale
            zero = np.abs(ex) <= LD(2.0) ** -1076                           # a quarter of the smallest denormal: exp(-z) itself rounds to 0
            assert one.any() and zero.any() if name.endswith("saturation") else True
            assert np.array_equal(got[one], orc[one]) and np.all(np.abs(got[one]) == sc[one]), name
            assert np.all(got[zero] == 0.0) and np.array_equal(np.signbit(got[zero]), np.signbit(orc[zero])), name
            # the oracle's class everywhere its literal formula is in a class, EXCEPT inside the two ranges of z where that formula
            # saturates before the function does (csrc/glrm_fastmath.hpp): there the device may return the correctly rounded derivative
            # instead -- the double next to -+scale towards 0, or a value of the oracle's sign no larger than scale 2^-1024 -- and nothing else
            zz = z[fin]
            in_class = (np.abs(orc) == sc) | (orc == 0.0)
            differ = in_class & ~((got == orc) & (np.signbit(got) == np.signbit(orc)))
            early_one = (zz > EARLY_ONE[0]) & (zz < EARLY_ONE[1]) & (np.abs(orc) == sc)
            early_zero = (zz > EARLY_ZERO[0]) & (zz < EARLY_ZERO[1]) & (orc == 0.0)
            assert not np.any(differ & ~(early_one | early_zero)), (name, zz[differ & ~(early_one | early_zero)][:5])
            d1, d0 = differ & early_one, differ & early_zero
            assert np.array_equal(got[d1], np.nextafter(orc[d1], 0.0)), (name, zz[d1][:5], got[d1][:5])
            assert np.all((np.signbit(got[d0]) == np.signbit(orc[d0])) & (np.abs(got[d0]) <= sc[d0] * 2.0 ** -1024)), (name, zz[d0][:5], got[d0][:5])
            nearest += int(differ.sum())
    assert nearest > 0   # the point sets reach into both ranges
    print("LogisticLoss: %d points where the oracle's literal derivative is already -+scale / +-0 and the device's is its neighbour" % nearest)
    d = R.descs(R.LOGISTIC, 2, 1.0)
    L, _ = pointwise(d, np.array([1.0, 1.0]), np.array([1.0, 0.0]))
    assert L[0][0] == 0.31326168751822286 and L[0][1] == 1.3132616875182228      # test/loss_test.jl
    assert L[1][0] == 0.31326168751822286 and L[1][1] == 1.3132616875182228


def test_fm_logistic_is_what_loss_both_runs():
    """the bare primitive (op 5 / 6) against the LogisticLoss case of loss_both, bit for bit"""
    b = {x.name: x for x in R.scalar_buckets()}["Logistic/saturation"]
    L, dL = scalar_run()[b.name]
    pL, pdL = pointwise(b.desc, b.u, 2 * b.a - 1, op=5)
    tL, tdL = pointwise(b.desc, b.u, 2 * b.a - 1, op=6)
    assert same_bits(pL, L[0]) and same_bits(pdL, dL[0]) and same_bits(tL, L[1]) and np.all(tdL == 0.0)


# ---------------------------------------------------------------------------------------------------------------- obs_loss

def _lgs(d):
    return [lg for lg in range(2, 7) if (1 << lg) >= max(d, 4)]


@pytest.mark.parametrize("d", R.DIMS)
def test_multidimensional_kinds_within_the_bucket_bound(d):
    bs = R.multi_buckets(d)
    refs = {b.name: R.multi_reference(d, b.name) for b in bs}
    desc = np.concatenate([b.desc for b in bs])
    level, U = np.concatenate([b.level for b in bs]), np.concatenate([b.U for b in bs])
    n = len(desc)
    perm = np.random.default_rng(100 + d).permutation(n)       # a wave holds the five kinds side by side
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    dims = np.full(n, d, np.int32)
    worst, nearest = {}, {"L": 0.0, "grad": 0.0}
    for lg in _lgs(d):
        P = 1 << lg
        runs = {}
        for km in (0, 1, 2, 3):   # every kind mask at every slot width
            runs[km] = [x[inv] for x in obs_loss(desc[perm], dims, level[perm], widen(U[perm], P), lg, km)]
        Lg, G, Lt = runs[0]
        assert same_bits(Lg, np.repeat(Lg[:, :1], P, axis=1)), ("L is uniform over the slot", d, lg)
        assert same_bits(Lg, Lt), ("one L for both passes", d, lg)
        assert np.all(G[:, d:] == 0.0), ("no gradient past the dimension", d, lg)
        for km, (Lk, Gk, Ltk) in runs.items():
            if km == 0:
                continue
            m = np.isin(desc["kind"], [k for k in KM_KINDS[km] if k != "scalar"])
            assert m.any() and same_bits(Lk[m], Lg[m]) and same_bits(Gk[m], G[m]) and same_bits(Ltk[m], Lt[m]), ("kind mask", km, d, lg)
        at = 0
        for b in bs:
            _, eL, eG, idx, oL, oG = refs[b.name]
            sl = slice(at, at + len(b.desc))
            at += len(b.desc)
            so, sd = _held_to_the_bucket_bound("%s lg %d" % (b.name, lg), b, eL, eG, oL, oG, Lg[sl][idx, 0], G[sl][idx, :d])
            # and next to the oracle at every observation, in ulps of the computation's scale: sharp where the bucket's maximum is the
            # figure of one ill-conditioned point (every special bucket)
            ML, MG = R.multi_computation_scale(b, idx)
            for got, orc, M, what in ((Lg[sl][idx, 0], oL, ML, "L"), (G[sl][idx, :d], oG, MG, "grad")):
                with np.errstate(all="ignore"):
                    both = np.isfinite(got) & np.isfinite(orc) & np.isfinite(M)
                    off = np.abs(got - orc) / R.ulp(M)
                assert np.array_equal(R.classes(got)[~both], R.classes(orc)[~both]), (b.name, lg, what)
                bad = both & ~(off <= R.MULTI_SCALE_ULPS(d))
                assert not bad.any(), (b.name, lg, what, np.argwhere(bad)[:3], got[bad][:3], orc[bad][:3], off[bad][:3])
                nearest[what] = max(nearest[what], float(off[both].max(initial=0.0)))
            w = worst.setdefault(b.name, [so, 0.0, 0.0])
            w[1], w[2] = max(w[1], sd.max_L), max(w[2], sd.max_G)
    print("d %d: largest |device - oracle| in ulps of the scale: L %.3g, grad %.3g (allowed %g)" % (d, nearest["L"], nearest["grad"], R.MULTI_SCALE_ULPS(d)))
    for name, (so, ml, mg) in worst.items():
        print("TABLE %-34s | %.3g | %.3g | %.3g | %.3g |" % (name, so.max_L, ml, so.max_G, mg))


def _scalar_sample():
    """every special point and every 16th bulk point of the scalar buckets, as observations of dimension 1"""
    parts = []
    for b in R.scalar_buckets():
        sel = np.arange(len(b.u)) if b.special else np.arange(0, len(b.u), 16)
        parts.append((b.desc[sel], b.u[sel], b.a[sel]))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def test_scalar_losses_through_obs_loss_have_the_bits_of_loss_both():
    desc, u, a = _scalar_sample()
    perm = np.random.default_rng(9).permutation(len(u))
    desc, u, a = desc[perm], u[perm], a[perm]
    L, dL = pointwise(desc, u, a)
    dims = np.ones(len(u), np.int32)
    for lg in range(2, 7):
        P = 1 << lg
        for km in (0, 2):
            Lg, G, Lt = obs_loss(desc, dims, a, widen(u[:, None], P), lg, km)
            for j in range(P):   # value and derivative are uniform over the slot
                assert same_bits(Lg[:, j], L[0]) and same_bits(G[:, j], dL[0]) and same_bits(Lt[:, j], L[1]), (lg, km, j)


def _mixed_waves(P, g):
    """(desc, dims, level, U (n x P)): whole waves of 64 / P slots each, put together on purpose"""
    SL = 64 // P
    nan = float("nan")

    def ob(kind, d, scalar=None):
        d = min(d, P)
        if kind is None:
            return (R.descs(R.QUAD, 1), 0, 1.0, np.zeros(P))
        if scalar is not None:
            dsc, u, a = scalar
            return (dsc, 1, a, widen(np.array([[u]]), P)[0])
        p0, p1 = R._bin_params(kind, 1, g)
        lv = float(g.integers(1, R.levels_of(kind, d) + 1))
        return (R.descs(kind, 1, g.choice([1.0, 0.7]), p0, p1, d), d, lv, widen(2.0 * g.standard_normal((1, d)), P)[0])

    sc = lambda kind, p0=0.0: (R.descs(kind, 1, 0.7, p0), float(3 * g.standard_normal()), float(g.integers(0, 2)))
    waves = []
    for _ in range(24):
        nanord = ob(R.MULTINOMIAL_ORDINAL, 5)
        nanord[3][int(g.integers(0, nanord[1]))] = nan
        patterns = [
            [ob(R.MULTINOMIAL_ORDINAL, 5), ob(R.MULTINOMIAL, 4), ob(None, 0), ob(None, 1, sc(R.LOGISTIC))],        # ordinal, Multinomial, idle, scalar
            [ob(R.MULTINOMIAL, 16), ob(R.OVA, 3), ob(R.ORDISTIC, 7), ob(None, 1, sc(R.HUBER, 1.0))],               # no ordinal slot
            [ob(None, 0)] * (SL - 1) + [ob(R.BVS, 9)],                                                             # idle but for the last slot
            [nanord, ob(R.MULTINOMIAL_ORDINAL, 16), ob(R.BVS, 2), ob(None, 1, sc(R.PERIODIC, 24.0))],              # a NaN threshold next door
            [ob(R.ORDISTIC, 32), ob(R.MULTINOMIAL_ORDINAL, 3), ob(R.MULTINOMIAL_ORDINAL, 31), ob(R.MULTINOMIAL, 2)],
        ]
        for pat in patterns:
            seq = list(pat) if len(pat) >= SL else (list(pat) * SL)[:SL]   # narrow slots: the pattern repeats along the wave
            seq += [ob(None, 0)] * (-len(seq) % SL)                         # wide slots: the pattern spans waves, idle slots behind it
            waves += seq
    desc = np.concatenate([w[0] for w in waves])
    return desc, np.array([w[1] for w in waves], np.int32), np.array([w[2] for w in waves]), np.array([w[3] for w in waves])


@pytest.mark.parametrize("lg", [2, 3, 4, 5, 6])
def test_every_slot_of_a_mixed_wave_gives_what_its_observation_gives_alone(lg):
    P, SL = 1 << lg, 64 >> lg
    desc, dims, level, U = _mixed_waves(P, np.random.default_rng(40 + lg))
    n = len(dims)
    assert n % SL == 0
    together = obs_loss(desc, dims, level, U, lg, 0)
    # alone: the observation in slot 0 of its own wave, the other slots idle
    d2 = np.repeat(desc, SL)
    dims2, level2, U2 = np.zeros(n * SL, np.int32), np.repeat(level, SL), np.repeat(U, SL, axis=0)
    dims2[::SL] = dims
    alone = [x[::SL] for x in obs_loss(d2, dims2, level2, U2, lg, 0)]
    live = dims > 0
    assert live.any() and (~live).any() or SL == 1
    for t, a_ in zip(together, alone):
        assert same_bits(t[live], a_[live]), lg
    assert np.all(together[0][~live] == 0.0) and np.all(together[1][~live] == 0.0)   # an idle slot contributes nothing


def test_the_hooks_refuse_bad_arguments():
    lib = _capi.hip_testing_api().lib
    one = np.zeros(4)
    d = R.descs(R.QUAD, 1)
    lib.glrm_test_loss_pointwise.restype = lib.glrm_test_obs_loss.restype = C.c_int
    lib.glrm_test_loss_pointwise.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    lib.glrm_test_obs_loss.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    p = one.ctypes.data
    assert lib.glrm_test_loss_pointwise(d.ctypes.data, p, p, 1, 7, p, p) != 0
    assert lib.glrm_test_loss_pointwise(None, p, p, 1, 0, p, p) != 0
    assert lib.glrm_test_loss_pointwise(d.ctypes.data, p, p, (1 << 20) + 1, 0, p, p) != 0
    dims = np.array([5], np.int32)
    for lg, km in ((1, 0), (7, 0), (2, 4), (2, 0)):   # the last: dimension 5 in a slot of 4 lanes
        assert lib.glrm_test_obs_loss(d.ctypes.data, dims.ctypes.data, p, p, 1, lg, km, p, p, p) != 0
