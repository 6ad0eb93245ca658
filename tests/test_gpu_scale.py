"""-m gpu: glrm_hip_scale_columns (include/glrm_hip_scale.h) -- scale=True / equilibrate_variance_ / prob_scale_ on the device against the
host transcriptions tests/extras/scaling.py and tests/extras/prob_scale.py, which stay the yardstick.

Tolerances (derived, not tuned):
  * order statistics are exact data values, so the M-estimate of a median / quantile column agrees with numpy to 8 eps max|a|: the two
    libraries' mid-point / interpolation formulas each round at most three times;
  * scales of Quad / L1 / Huber / Quantile / OrdinalHinge / WeightedHinge columns: sums of nobs <= 65536 non-negative fp64 terms added in
    another order, 2 nobs 2^-53 <= 1.5e-11 -> rtol 1e-10 (the M-estimate enters at second order; |mean| / std <= 10 keeps the two-pass
    variance well conditioned);
  * Periodic / Poisson / Logistic columns evaluate sin / cos / exp / log in the kernel against libm: rtol 1e-9, the figure
    tests/test_gpu_jref.py uses for that on C5.
Every test prints the largest deviation it saw per kind before it asserts (run with -s)."""
import copy
import ctypes

import numpy as np
import pytest

import extras as E
import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.losses import pack_losses
from lowrankmodels.jl_amd.regularizers import pack_regs

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LDS_MAX = 4096   # csrc/glrm_scale.hip: SC_LDS_MAX, the only length threshold of the kernel (LDS-staged / streamed radix select)
LIBM_KINDS = (L.PeriodicLoss, L.PoissonLoss, L.LogisticLoss)


def hip():
    return _capi.hip_api()


def rtol_of(loss):
    return 1e-9 if isinstance(loss, LIBM_KINDS) else 1e-10


def colview(cols, losses, ry, lo=0, hi=None):
    """The column view of the columns [lo, hi) of the problem whose columns hold the values ``cols`` (a list of 1-d arrays)."""
    n = len(cols)
    hi = n if hi is None else hi
    lens = [len(c) for c in cols[lo:hi]]
    colptr = np.zeros(hi - lo + 1, dtype=np.int64)
    np.cumsum(lens, out=colptr[1:])
    colvals = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float64) for c in cols[lo:hi]] + [np.zeros(0)]))
    m = max(max(len(c) for c in cols), 1)
    return _capi.ProblemArrays(m, n, 2, None, None, None, colptr, None, colvals, pack_losses(losses), pack_regs([L.QuadReg()]),
                               pack_regs(ry[lo:hi]), col_begin=lo, col_end=hi)


def reldev(a, b):
    a, b = float(a), float(b)
    return 0.0 if a == b else abs(a - b) / max(abs(b), np.finfo(float).tiny)


# ---------------------------------------------------------------------------------------------------------------- 1 + 2
def every_kind_model(scale):
    rng = np.random.default_rng(11)
    m = 64
    cols = [
        (L.QuadLoss(), rng.standard_normal(m) * 3 + 1),
        (L.L1Loss(2.0), np.round(rng.standard_normal(m) * 2)),                        # duplicates
        (L.HuberLoss(1.0, crossover=0.7), rng.standard_normal(m)),
        (L.QuantileLoss(1.5, quantile=0.3), rng.standard_normal(m) - 2),
        (L.PeriodicLoss(2.0), rng.random(m) * 2),
        (L.PoissonLoss(20), rng.poisson(3.0, m).astype(float)),
        (L.OrdinalHingeLoss(1, 5), np.round(np.clip(3 + rng.standard_normal(m), 1, 5))),
        (L.LogisticLoss(), rng.random(m) < 0.3),
        (L.WeightedHingeLoss(1.0, case_weight_ratio=2.0), rng.random(m) < 0.4),
        # degenerate columns: the rules leave them alone
        (L.QuadLoss(3.0), np.full(m, 3.0)),                                            # constant: avg_loss = variance = 0
        (L.QuadLoss(2.0), rng.standard_normal(m)),                                     # ONE observation (mask below): variance NaN
        (L.LogisticLoss(2.0), np.ones(m, dtype=bool)),                                 # all true: M = +Inf, loss 0
        (L.LogisticLoss(2.0), np.zeros(m, dtype=bool)),                                # all false: M = 0 (not degenerate: log 2 per entry)
        (L.WeightedHingeLoss(1.5, case_weight_ratio=2.0), np.zeros(m, dtype=bool)),    # no positive: r = +Inf, M = -1, loss 0
    ]
    losses = [c[0] for c in cols]
    A = np.column_stack([np.asarray(c[1], dtype=float) for c in cols])
    mask = rng.random(A.shape) < 0.8
    mask[:, 10] = False
    mask[7, 10] = True
    mask[:, 0] |= ~mask.any(axis=1)   # no empty row
    I, J = np.nonzero(mask)
    ry = [copy.copy((L.QuadReg(0.5), L.OneReg(0.2), L.ZeroReg(), L.QuadReg(1.0), L.OneReg(0.3))[f % 5]) for f in range(len(cols))]
    g = L.GLRM(A, losses, L.QuadReg(0.5), ry, 3, obs=(I, J), scale=scale, rng=np.random.default_rng(5))
    return g, A, I, J


def test_scale_true_equals_the_transcription_on_every_scalar_kind():
    g, A, I, J = every_kind_model(True)                          # the engine (hip_api is the default engine)
    r, _, _, _ = every_kind_model(E.equilibrate_variance_)       # the host transcription
    start, _, _, _ = every_kind_model(False)
    worst = {}
    for f in range(g.n):
        name = type(g.losses[f]).__name__
        dl = reldev(g.losses[f].scale, r.losses[f].scale)
        dr = reldev(g.ry[f].scale, r.ry[f].scale) if not isinstance(g.ry[f], L.ZeroReg) else 0.0
        worst[name] = max(worst.get(name, 0.0), dl)
        worst["ry(variance)"] = max(worst.get("ry(variance)", 0.0), dr)
    print("max relative deviation of the scales per kind:", {k: f"{v:.2e}" for k, v in worst.items()})
    for f in range(g.n):
        assert reldev(g.losses[f].scale, r.losses[f].scale) <= rtol_of(g.losses[f]), (f, g.losses[f].scale, r.losses[f].scale)
        if not isinstance(g.ry[f], L.ZeroReg):
            assert reldev(g.ry[f].scale, r.ry[f].scale) <= 1e-10, (f, g.ry[f].scale, r.ry[f].scale)
    for f in (9, 11, 13):                                        # avg_loss = 0: the loss scale is unchanged, exactly
        assert g.losses[f].scale == start.losses[f].scale == r.losses[f].scale, f
    assert g.losses[10].scale == 2.0 and g.ry[10].scale == start.ry[10].scale    # one observation: loss 0, variance NaN
    assert g.ry[9].scale == start.ry[9].scale                    # constant column: variance 0
    assert g.losses[12].scale == pytest.approx(2.0 / (2.0 * np.log(2.0)), rel=1e-9)
    assert g.losses[0].scale != 1.0 and g.ry[0].scale != 0.5     # the ordinary columns did move


def test_m_estimates_and_diagnostics_against_numpy():
    g, A, I, J = every_kind_model(False)
    ls, rs, d = hip().scale_columns(L.scaling.column_view(g), _capi.SCALE_EQUILIBRATE, diagnostics=True)
    worst = {}
    for f in range(g.n):
        a = A[I[J == f], f]
        l = g.losses[f]
        want = E.M_estimator(l, a)
        got = d["m_est"][f]
        if isinstance(l, (L.L1Loss, L.HuberLoss, L.OrdinalHingeLoss, L.QuantileLoss)):
            dev, bound = abs(got - want), 8 * EPS * np.abs(a).max()
        elif np.isfinite(want):
            dev, bound = reldev(got, want), (1e-9 if isinstance(l, LIBM_KINDS) else 1e-10)
        else:
            dev, bound = (0.0 if got == want else np.inf), 0.0
        worst[type(l).__name__] = max(worst.get(type(l).__name__, 0.0), dev)
        assert dev <= bound, (f, type(l).__name__, got, want)
        if len(a) > 1:
            assert reldev(d["variance"][f], np.var(a, ddof=1)) <= 1e-10 or np.var(a, ddof=1) == d["variance"][f]
        else:
            assert np.isnan(d["variance"][f])
    print("max deviation of the M-estimates per kind:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_empty_column_and_all_zero_poisson_column_are_left_alone():
    """By hand: the transcription raises `math domain error` on log(0) where Julia gives -Inf.  All-zero Poisson: M = log(0) = -Inf,
    0 * -Inf = NaN, NaN > 0 is false -> unchanged; its variance is 0 -> ry unchanged."""
    pz = L.PoissonLoss(10)
    pz.mul_(2.5)
    losses = [L.QuadLoss(4.0), pz, L.L1Loss(3.0), L.QuadLoss(1.0)]
    ry = [L.QuadReg(0.7), L.QuadReg(0.6), L.OneReg(0.3), L.QuadReg(0.9)]
    cols = [np.zeros(0), np.zeros(17), np.zeros(0), np.arange(5.0)]
    ls, rs, d = hip().scale_columns(colview(cols, losses, ry), _capi.SCALE_EQUILIBRATE, diagnostics=True)
    assert ls[0] == 4.0 and rs[0] == 0.7 and ls[2] == 3.0 and rs[2] == 0.3
    assert ls[1] == 2.5 and rs[1] == 0.6
    assert d["m_est"][1] == -np.inf and np.isnan(d["avg_loss"][1]) and d["variance"][1] == 0.0
    assert ls[3] == pytest.approx(1.0 / 2.0, rel=1e-12) and rs[3] == pytest.approx(0.9 / 2.5, rel=1e-12)   # mean 2: avg (4+1+0+1+4)/5, var 10/4
    lp, rp = hip().scale_columns(colview(cols, losses, ry), _capi.SCALE_PROB)
    assert lp[0] == 4.0 and lp[2] == 3.0 and lp[1] == 1.0 and list(rp) == [0.7, 0.6, 0.3, 0.9]


# ---------------------------------------------------------------------------------------------------------------- 3
def ragged_columns():
    rng = np.random.default_rng(21)
    lengths = [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, LDS_MAX - 1, LDS_MAX, LDS_MAX + 1, LDS_MAX + 2, 2 * LDS_MAX + 1, 30001, 65535, 65536]
    cols, losses = [], []
    for i, n in enumerate(lengths):
        for variant in range(4):
            if variant == 0:
                a = rng.standard_normal(n) * 2 + 1                              # |mean| / std = 0.5
            elif variant == 1:                                                  # heavy duplicates around the median, both zeros
                a = np.round(rng.standard_normal(n) * 1.5)
                a[(a == 0) & (rng.random(n) < 0.5)] = -0.0
            elif variant == 2:
                a = -np.abs(rng.standard_normal(n)) * 1e3 - 1.0                 # negative values only
                if n < 8:
                    a = -100.0 * np.arange(1, n + 1)                            # (a random pair can sit far from 0 relative to its spread)
            else:
                a = np.where(rng.random(n) < 0.5, -1.0, 1.0) * np.exp(rng.standard_normal(n) * 8)   # many binades, both signs
            cols.append(a)
            losses.append((L.L1Loss(), L.QuantileLoss(quantile=0.3), L.HuberLoss(1.0, crossover=0.5), L.QuantileLoss(quantile=0.9))[(i + variant) % 4])
    return cols, losses


def test_long_and_ragged_columns_select_exactly():
    cols, losses = ragged_columns()
    ry = [L.QuadReg(1.0) for _ in cols]
    ls, rs, d = hip().scale_columns(colview(cols, losses, ry), _capi.SCALE_EQUILIBRATE, diagnostics=True)
    worst_m, worst_s = 0.0, 0.0
    for f, (a, l) in enumerate(zip(cols, losses)):
        n, got = len(a), d["m_est"][f]
        assert n <= 65536 and (n == 1 or abs(a.mean()) <= 10 * a.std(ddof=1)), "the derived tolerances need this of the INPUT"
        if isinstance(l, L.QuantileLoss):
            want = float(np.quantile(a, l.quantile))
        else:
            want = float(np.median(a))
            if n % 2 == 1:   # a data value, bit for bit (a zero comes back as +0.0 whichever zero numpy's partition left in the middle)
                assert np.float64(got + 0.0).tobytes() == np.float64(want + 0.0).tobytes(), (f, n, got, want)
        worst_m = max(worst_m, abs(got - want) / np.abs(a).max())
        assert abs(got - want) <= 8 * EPS * np.abs(a).max(), (f, n, type(l).__name__, got, want)
        if isinstance(l, L.L1Loss):
            avg = float(np.mean(np.abs(got - a)))
        elif isinstance(l, L.QuantileLoss):
            diff = a - got
            avg = float(np.mean(np.where(diff > 0, l.quantile * diff, -(1 - l.quantile) * diff)))
        elif isinstance(l, L.HuberLoss):
            ad = np.abs(got - a)
            avg = float(np.mean(np.where(ad > l.crossover, ad - l.crossover + l.crossover ** 2, ad ** 2)))
        if avg > 0:
            worst_s = max(worst_s, reldev(ls[f], 1.0 / avg))
            assert reldev(ls[f], 1.0 / avg) <= 1e-10, (f, n, ls[f], 1.0 / avg)
        else:
            assert ls[f] == l.scale
        if n > 1:
            assert reldev(rs[f], 1.0 / np.var(a, ddof=1)) <= 1e-10, (f, n)
        else:
            assert rs[f] == 1.0
    print(f"ragged columns: max |m_est - numpy| / max|a| = {worst_m:.2e}, max relative deviation of the loss scale = {worst_s:.2e}")


def test_a_column_far_beyond_the_staging_limit():
    """600 001 and 600 000 entries (the radix select streams the column once per digit); medians only: the scale tolerances above are
    derived for nobs <= 65536."""
    rng = np.random.default_rng(22)
    a = rng.standard_normal(600001) * 5 - 1
    b = np.round(rng.standard_normal(600000) * 3)      # even nobs, the two middle values are duplicates
    cols, losses = [a, b, a[:-1]], [L.L1Loss(), L.L1Loss(), L.QuantileLoss(quantile=0.75)]
    _, _, d = hip().scale_columns(colview(cols, losses, [L.QuadReg()] * 3), _capi.SCALE_EQUILIBRATE, diagnostics=True)
    assert np.float64(d["m_est"][0]).tobytes() == np.float64(np.median(a)).tobytes()
    assert d["m_est"][1] + 0.0 == np.median(b) + 0.0
    assert abs(d["m_est"][2] - np.quantile(a[:-1], 0.75)) <= 8 * EPS * np.abs(a).max()


# ---------------------------------------------------------------------------------------------------------------- 4
def mixed_problem():
    rng = np.random.default_rng(31)
    kinds = [lambda: L.QuadLoss(1.3), lambda: L.L1Loss(), lambda: L.HuberLoss(1.0, crossover=0.7), lambda: L.QuantileLoss(quantile=0.3),
             lambda: L.PeriodicLoss(2.0), lambda: L.PoissonLoss(20), lambda: L.OrdinalHingeLoss(1, 5), lambda: L.LogisticLoss(),
             lambda: L.WeightedHingeLoss(1.0, case_weight_ratio=2.0)]
    cols, losses, ry = [], [], []
    for f in range(45):
        n = int(rng.choice([0, 1, 2, 7, 100, 257, 3000, LDS_MAX, LDS_MAX + 1, 9001, 20000]))
        l = kinds[f % 9]()
        if isinstance(l, (L.LogisticLoss, L.WeightedHingeLoss)):
            a = (rng.random(n) < 0.35).astype(float)
        elif isinstance(l, L.PoissonLoss):
            a = rng.poisson(2.0, n).astype(float)
        elif isinstance(l, L.OrdinalHingeLoss):
            a = np.round(np.clip(3 + rng.standard_normal(n), 1, 5))
        else:
            a = rng.standard_normal(n) + 0.5
        cols.append(a)
        losses.append(l)
        ry.append(L.QuadReg(0.1 * (f + 1)))
    return cols, losses, ry


def as_bytes(res):
    ls, rs, d = res
    return b"".join(np.ascontiguousarray(x).tobytes() for x in (ls, rs, d["m_est"], d["avg_loss"], d["variance"]))


@pytest.mark.parametrize("mode", [_capi.SCALE_EQUILIBRATE, _capi.SCALE_PROB], ids=["equilibrate", "prob"])
def test_two_calls_column_blocks_and_device_arrays_give_the_same_bytes(mode):
    import torch
    cols, losses, ry = mixed_problem()
    api, n = hip(), len(cols)
    whole = api.scale_columns(colview(cols, losses, ry), mode, diagnostics=True)
    assert as_bytes(api.scale_columns(colview(cols, losses, ry), mode, diagnostics=True)) == as_bytes(whole)
    for c in (1, 17, n - 1):
        lo = api.scale_columns(colview(cols, losses, ry, 0, c), mode, diagnostics=True)
        hi = api.scale_columns(colview(cols, losses, ry, c, n), mode, diagnostics=True)
        cat = (np.concatenate([lo[0], hi[0]]), np.concatenate([lo[1], hi[1]]), {k: np.concatenate([lo[2][k], hi[2][k]]) for k in lo[2]})
        assert as_bytes(cat) == as_bytes(whole), c
    p = colview(cols, losses, ry)
    dptr, dval = torch.from_numpy(p.colptr).cuda(), torch.from_numpy(p.colvals).cuda()
    torch.cuda.synchronize()
    p.colptr, p.colvals, p.flags = dptr.data_ptr(), dval.data_ptr(), _capi.PROBLEM_DEVICE_ARRAYS
    assert as_bytes(api.scale_columns(p, mode, diagnostics=True)) == as_bytes(whole)
    del dptr, dval


# ---------------------------------------------------------------------------------------------------------------- 5
def test_prob_scale_equals_the_transcription():
    def model():
        rng = np.random.default_rng(3)
        A = np.column_stack([rng.standard_normal(30) * 2, rng.standard_normal(30), rng.random(30) < 0.5, 0.01 * rng.standard_normal(30),
                             np.full(30, 2.0)])
        return A, L.GLRM(A, [L.QuadLoss(), L.HuberLoss(), L.LogisticLoss(3.0), L.QuadLoss(), L.QuadLoss(5.0)], L.QuadReg(), L.QuadReg(0.4), 2,
                         rng=np.random.default_rng(1))
    A, g = model()
    _, r = model()
    L.prob_scale_(g, engine=hip())
    E.prob_scale_(r)
    for f in range(g.n):
        print(f"prob_scale column {f}: engine {g.losses[f].scale!r} transcription {r.losses[f].scale!r}")
        assert reldev(g.losses[f].scale, r.losses[f].scale) <= 1e-10, f
    assert g.losses[2].scale == 1.0                                       # mul!(l, 1) SETS the scale
    v = np.var(A[:, 3], ddof=1)
    assert 1e-12 < v < 1e-3 and g.losses[3].scale == pytest.approx(1 / (2 * v)) and g.losses[3].scale > 1000
    assert g.losses[4].scale == 5.0                                       # variance 0 <= TOL: not scaled
    assert all(x.scale == 0.4 for x in g.ry)                              # prob_scale! leaves the regularizers alone


# ---------------------------------------------------------------------------------------------------------------- 6
def test_scaled_model_with_offset_fits_like_the_oracle():
    rng = np.random.default_rng(2)
    m, n = 40, 4
    A = np.column_stack([rng.standard_normal(m) * 3 + 1, rng.random(m) < 0.3, np.round(np.clip(3 + rng.standard_normal(m), 1, 5)), rng.standard_normal(m)])
    make = lambda: [L.QuadLoss(), L.LogisticLoss(), L.OrdinalHingeLoss(1, 5), L.HuberLoss(2.0)]
    losses, initial = make(), make()
    I, J = np.nonzero(rng.random((m, n)) < 0.8)
    g = L.GLRM(A, losses, L.QuadReg(0.5), [L.QuadReg(0.5), L.OneReg(0.2), L.ZeroReg(), L.QuadReg(1.0)], 3, obs=(I, J), scale=True, offset=True, rng=rng)
    for f, (l0, r0) in enumerate(zip(initial, [0.5, 0.2, 1.0, 1.0])):   # scaling ran BEFORE the offset wrappers went on
        col = A[I[J == f], f].astype(float)
        assert g.losses[f].scale == pytest.approx(l0.scale / E.avgerror(l0, col), rel=1e-9)
        assert isinstance(g.ry[f], L.lastentry_unpenalized)
        if not isinstance(g.ry[f].r, L.ZeroReg):
            assert g.ry[f].r.scale == pytest.approx(r0 / np.var(col, ddof=1), rel=1e-10)
    assert all(isinstance(r, L.lastentry1) for r in g.rx)
    go = L.copy_estimate(g)                                              # the same descriptor objects, its own X / Y
    params = L.ProxGradParams(max_iter=20)
    _, _, ch = L.fit_b(g, params, verbose=False, engine=hip())
    _, _, cho = L.fit_b(go, params, verbose=False, engine=O.oracle_api())
    a, b = np.asarray(ch.objective), np.asarray(cho.objective)
    assert len(a) == len(b) and len(a) > 2
    # objective[0] includes rx: lastentry1 is +Inf at a random start (last entry != 1) in the reference, the oracle and the engine alike
    assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.isfinite(a[1:]).all()
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin])
    print("objective trajectory, max relative deviation engine vs oracle:", float(np.max(np.abs(a[fin] - b[fin]) / np.abs(b[fin]))))
    assert np.all(np.abs(a[fin] - b[fin]) <= 1e-5 * np.abs(b[fin]))
    assert np.isfinite(a[-1]) and a[-1] < a[1]


# ---------------------------------------------------------------------------------------------------------------- 7
def test_errors_carry_a_status_and_a_message():
    api = hip()
    cols = [np.arange(4.0), np.array([1.0, 2.0, 3.0, 1.0])]
    ry = [L.QuadReg(), L.QuadReg()]
    with pytest.raises(_capi.GLRMError) as ei:
        api.scale_columns(colview(cols, [L.QuadLoss(), L.MultinomialLoss(3)], ry), _capi.SCALE_EQUILIBRATE)
    assert ei.value.code == _capi.ERR_UNSUPPORTED and "multi-dimensional" in ei.value.message
    dense = _capi.ProblemArrays(4, 2, 2, None, None, None, None, None, None, pack_losses([L.QuadLoss()]), pack_regs([L.QuadReg()]),
                                pack_regs([L.QuadReg()]), dense_A=np.zeros((4, 2)), dense_ld=2, dense_colmajor=0)
    with pytest.raises(_capi.GLRMError) as ei:
        api.scale_columns(dense, _capi.SCALE_EQUILIBRATE)
    assert ei.value.code == _capi.ERR_UNSUPPORTED and "dense_A" in ei.value.message
    p = colview(cols, [L.QuadLoss(), L.L1Loss()], ry)
    cp, co = api._cproblem(p), _capi.COptions(-1, 0, 0, 0, None, 0, 0, 0, 0, 0, 0)
    out = np.zeros(2)
    for args in ((None, out.ctypes.data), (out.ctypes.data, None)):
        rc = api._f["scale_columns"](ctypes.byref(cp), ctypes.byref(co), 0, args[0], args[1], None, None, None)
        assert rc == _capi.ERR_INVALID and "NULL" in api.last_error()
    rc = api._f["scale_columns"](ctypes.byref(cp), ctypes.byref(co), 7, out.ctypes.data, out.ctypes.data, None, None, None)
    assert rc == _capi.ERR_INVALID and "mode" in api.last_error()
    with pytest.raises(_capi.GLRMError) as ei:   # the column view is what the pass reads: it cannot be NULL
        api.scale_columns(_capi.ProblemArrays(4, 2, 2, None, None, None, None, None, None, pack_losses([L.QuadLoss()]), pack_regs([L.QuadReg()]),
                                              pack_regs([L.QuadReg()])), _capi.SCALE_EQUILIBRATE)
    assert ei.value.code == _capi.ERR_INVALID


def test_columns_to_scale_leaves_the_other_columns_untouched():
    g, A, I, J = every_kind_model(False)
    ref, _, _, _ = every_kind_model(True)
    before = [(l.scale, r.scale) for l, r in zip(g.losses, g.ry)]
    L.equilibrate_variance_(g, columns_to_scale=[1, 4, 6], engine=hip())
    for f in range(g.n):
        if f in (1, 4, 6):
            assert (g.losses[f].scale, g.ry[f].scale) == (ref.losses[f].scale, ref.ry[f].scale) and g.losses[f].scale != before[f][0]
        else:
            assert (g.losses[f].scale, g.ry[f].scale) == before[f], f
    assert g._handle_cache is None
