"""The exact references and point sets of tests/loss_ref.py, checked without a GPU.

  * the two reference implementations (numpy.longdouble, mpmath at 50 digits) agree on a subsample of every bulk bucket;
  * the oracle's loss_evaluate / loss_grad / vloss_evaluate / vloss_grad (libm and the literal formulas of src/losses.jl) against the exact
    values on EVERY bucket: a formula mistake on either side shows as an error of the size of the value, so the median error of a bulk bucket
    is held to 2 ulp and the piecewise kinds (a handful of roundings, no cancellation beyond u - a) to 8 ulp everywhere.  The maxima measured
    here are what tests/test_gpu_loss_pointwise.py derives the device's bounds from (loss_ref.device_bound);
  * no bulk bucket leaves more than 2 % of its values out of the statistic (exact value not finite as a double), and where a value is left
    out the oracle's result has the exact value's class (NaN, +Inf, -Inf);
  * the host build of csrc/glrm_fastmath.hpp on the primitive buckets, at the bounds the device is held to.

`pytest -s` prints the table of the oracle's per-bucket maxima (LABNOTES.md, "Pointwise loss errors")."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR_NAMES = [b.name for b in R.scalar_buckets()]
MULTI_NAMES = [(d, b.name) for d in R.DIMS for b in R.multi_buckets(d)]
#: oracle and exact value may differ in CLASS only where the literal double formula overflows and the function does not (log(1 + exp(710)))
OVERFLOWING = {"Logistic/saturation"}
#: bulk medians, in ulp.  2 everywhere (a formula mistake is 2^52), except where the formula itself amplifies the rounding of its argument:
#: PeriodicLoss by |w| <= 2^8 on the bulk, MultinomialOrdinalLoss by |u| / TOL <= 2^13 between two clamped thresholds
MEDIAN_CAP = {R.PERIODIC: 1024.0, R.MULTINOMIAL_ORDINAL: 1024.0}


def test_the_point_sets_are_what_the_issue_lists():
    names = SCALAR_NAMES + [n for _, n in MULTI_NAMES] + [b.name for b in R.primitive_buckets()]
    assert len(set(names)) == len(names)
    for b in R.scalar_buckets():
        assert len(b.desc) == len(b.u) == len(b.a) and np.all(b.desc["kind"] == b.kind)
        assert len(b.u) == R.N_BULK if not b.special else 50 <= len(b.u) <= 6000, (b.name, len(b.u))
    assert {b.kind for b in R.scalar_buckets() if not b.special} == set(R.SCALAR_KINDS)
    for d in R.DIMS:
        bs = R.multi_buckets(d)
        assert {b.kind for b in bs if b.special} == {b.kind for b in bs if not b.special} == set(R.MULTI_KINDS)
        for b in bs:
            assert b.U.shape == (len(b.desc), d) and np.all(b.desc["dim"] == d)
            assert b.level.min() == 1 and b.level.max() == R.levels_of(b.kind, d), b.name   # the first and the last level
            assert len(b.desc) == R.N_BULK_MULTI if not b.special else len(b.desc) >= 8 * R.levels_of(b.kind, d), b.name
    again = R._scalar_bulk(R.LOGISTIC)
    assert np.array_equal(again.u, R.scalar_buckets()[R.LOGISTIC].u)   # fixed by seed


def _agree(a, b, slack):
    """longdouble against mpmath: 0.01 ulp, plus 2^-8 of the largest error the double evaluation (`slack`, the oracle's errors on the same
    points) makes: both follow the formula's conditioning -- a rounding of w in 1 - cos(w) costs longdouble 2^-11 of what it costs a double"""
    with np.errstate(all="ignore"):
        both = np.isfinite(a.astype(np.float64)) & np.isfinite(b.astype(np.float64))
        diff = (np.abs(a - b) / R.ulp(b.astype(np.float64))).astype(np.float64)
        assert np.array_equal(R.classes(a), R.classes(b))
        bad = both & ~(diff <= 0.01 + np.max(slack[np.isfinite(slack)], initial=0.0) / 256.0)
    assert not bad.any(), (np.flatnonzero(bad)[:5], diff[bad][:5])


@pytest.mark.skipif(not R.BULK_IS_LONGDOUBLE, reason="longdouble is a double here: the bulk uses mpmath itself")
@pytest.mark.parametrize("name", [n for n in SCALAR_NAMES if n.endswith("/bulk")])
def test_longdouble_and_mpmath_references_agree_scalar(name):
    b, eL, eG, idx, oL, oG = R.scalar_reference(name)
    sub = idx[:: len(idx) // 250]
    mL, mG = R.scalar_ref_mp(b.desc[sub], b.u[sub], b.a[sub])
    _agree(eL[:: len(idx) // 250], mL, R.ulps(oL[:: len(idx) // 250], mL)[0])
    _agree(eG[:: len(idx) // 250], mG, R.ulps(oG[:: len(idx) // 250], mG)[0])


@pytest.mark.skipif(not R.BULK_IS_LONGDOUBLE, reason="longdouble is a double here: the bulk uses mpmath itself")
@pytest.mark.parametrize("d", [2, 5, 32])
def test_longdouble_and_mpmath_references_agree_multi(d):
    for b in R.multi_buckets(d):
        for src in (b, ) if b.special else (b._replace(desc=b.desc[:60], level=b.level[:60], U=b.U[:60]),):
            if src.special and src.kind == R.MULTINOMIAL_ORDINAL:
                continue   # NaN thresholds: the special buckets ARE mpmath's
            lL, lG = R.multi_ref_ld(src.kind, src.desc, src.level, src.U)
            mL, mG = R.multi_ref_mp(src.kind, src.desc, src.level, src.U)
            oL, oG = R.oracle_multi(src.desc, src.level, src.U)
            _agree(lL, mL, R.ulps(oL, mL)[0])
            _agree(lG.ravel(), mG.ravel(), R.ulps(oG.ravel(), mG.ravel())[0])


def _check_oracle(b, eL, eG, idx, oL, oG):
    st = R.error_stats(oL, oG, eL, eG)
    print("%-34s n %6d  oracle max err: L %.3g ulp, grad %.3g ulp  (left out %.2f %%)" % (b.name, st.n, st.max_L, st.max_G, 100 * st.left_out))
    if not b.special:
        assert st.left_out <= 0.02, (b.name, st.left_out)
        for got, ex in ((oL, eL), (oG, eG)):
            e, counted = R.ulps(np.ravel(got), np.ravel(ex))
            assert np.median(e[counted]) <= MEDIAN_CAP.get(b.kind, 2.0), (b.name, np.median(e[counted]))
    if b.kind in R.EXACT_KINDS:
        # a point whose u - a rounds sits on the other side of a kink for the double formula than for the function (HuberLoss's gradient
        # jumps there): the statistic of the piecewise kinds takes the points whose difference is exact
        same = np.ones(len(oL), bool) if b.kind in (R.ORDINAL_HINGE, R.WEIGHTED_HINGE) else \
            (b.u[idx].astype(R.LD) - b.a[idx].astype(R.LD)) == (b.u[idx] - b.a[idx]).astype(R.LD)
        sx = R.error_stats(oL[same], oG[same], eL[same], eG[same])
        assert sx.max_L <= 8.0 and sx.max_G <= 8.0, (b.name, sx)
    if b.name not in OVERFLOWING:   # by class where the exact value is not finite
        for got, ex in ((oL, eL), (oG, eG)):
            out = ~R.ulps(np.ravel(got), np.ravel(ex))[1]
            assert np.array_equal(R.classes(np.ravel(got))[out], R.classes(np.ravel(ex))[out]), b.name
    return st


@pytest.mark.parametrize("name", SCALAR_NAMES)
def test_oracle_scalar_losses_against_the_exact_references(name):
    b, eL, eG, idx, oL, oG = R.scalar_reference(name)
    _check_oracle(b, eL, eG, idx, oL, oG)


@pytest.mark.parametrize("d", R.DIMS)
def test_oracle_multidimensional_losses_against_the_exact_references(d):
    for b in R.multi_buckets(d):
        b, eL, eG, idx, oL, oG = R.multi_reference(d, b.name)
        _check_oracle(b, eL, eG, idx, oL, oG)


@pytest.mark.parametrize("d", R.DIMS)
def test_oracle_within_the_computation_scale_of_the_exact_references(d):
    """loss_ref.multi_computation_scale, checked on the CPU: the oracle's own evaluation is within MULTI_SCALE_ULPS(d) ulps of that scale of
    the exact value at EVERY observation (the device test holds the device to the oracle in the same unit)"""
    for b in R.multi_buckets(d):
        b, eL, eG, idx, oL, oG = R.multi_reference(d, b.name)
        ML, MG = R.multi_computation_scale(b, idx)
        for got, ex, M in ((oL, eL, ML), (oG, eG, MG)):
            with np.errstate(all="ignore"):
                e64 = ex.astype(np.float64)
                both = np.isfinite(got) & np.isfinite(e64) & np.isfinite(M)
                off = (np.abs(got.astype(R.LD) - ex) / R.ulp(M)).astype(np.float64)
            assert both.mean() >= 0.98, (b.name, both.mean())
            assert not np.any(both & ~(off <= R.MULTI_SCALE_ULPS(d))), (b.name, np.max(off[both]))


@pytest.fixture(scope="module")
def host_fastmath(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    so = str(tmp_path_factory.mktemp("fm") / "libfastmath_points.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tools", "fastmath_points.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.fastmath_points.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]

    def run(op, x, scale=None, aa=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        scale = np.ones_like(x) if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
        aa = np.ones_like(x) if aa is None else np.ascontiguousarray(aa, dtype=np.float64)
        out, dout = np.zeros_like(x), np.zeros_like(x)
        assert lib.fastmath_points(op, x.ctypes.data, scale.ctypes.data, aa.ctypes.data, len(x), out.ctypes.data, dout.ctypes.data) == 0
        return out, dout
    return run


@pytest.mark.parametrize("name", [b.name for b in R.primitive_buckets()])
def test_host_build_of_the_primitives_on_the_device_tests_points(host_fastmath, name):
    b = {x.name: x for x in R.primitive_buckets()}[name]
    got, _ = host_fastmath(b.op, b.x)
    bad, worst = R.primitive_failures(b, got)
    print("%-24s n %6d  host max rel err %.3g" % (b.name, len(b.x), worst))
    assert len(bad) == 0, (b.name, b.x[bad][:5], got[bad][:5])


def test_host_logistic_is_zero_and_infinite_where_the_literal_formula_is(host_fastmath):
    b, eL, eG, idx, oL, oG = R.scalar_reference("Logistic/saturation")
    L, dL = host_fastmath(5, b.u, b.desc["scale"], 2 * b.a - 1)
    assert np.array_equal(L == 0.0, oL == 0.0) and np.array_equal(L == np.inf, oL == np.inf) and np.array_equal(np.isnan(L), np.isnan(oL))
    L6, _ = host_fastmath(6, b.u, b.desc["scale"], 2 * b.a - 1)
    assert np.array_equal(L, L6, equal_nan=True)
