"""-m gpu: glrm_options.storage = 1 (include/glrm_hip_storage.h) -- A, X and Y stored as floats on the gather
sweeps, every sum and the line search in fp64.

The half-steps are held to a lane-by-lane host reference bit for bit (tests/storage_f32_ref.py, anchored to the CPU oracle by
tests/test_storage_f32.py); what that reference does not model -- the other loss kinds, the per-observation row kernels, the objective and
penalty kernels -- is held to an fp64 gather handle on the same float-representable data, where the two must agree bit for bit."""
import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import oracle as O
import storage_f32_ref as S
from lowrankmodels.jl_amd import _capi
from test_sum_order import small_problem

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID, NONFINITE = _capi.ERR_UNSUPPORTED, _capi.ERR_INVALID, _capi.ERR_NONFINITE


def f32r(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64))


def make_representable(pa, X0, Y0, nonneg=False):
    pa.rowvals[:] = pa.rowvals.astype(np.float32)
    pa.colvals[:] = pa.colvals.astype(np.float32)
    if nonneg:
        X0, Y0 = np.abs(X0), np.abs(Y0)
    return pa, f32r(X0), f32r(Y0)


class Bound:
    """A handle with caller-owned buffers (glrm_hip_bind_buffers): float X / Y on an f32 handle, double objectives on both."""

    def __init__(self, pa, storage, **kw):
        import torch
        self.api, self.pa = _capi.hip_api(), pa
        self.h = self.api.create(pa, storage=storage, **kw)
        ld = self.api.factor_ld(self.h)
        dt = torch.float32 if storage else torch.float64
        self.dX = torch.zeros(ld * pa.m, dtype=dt, device="cuda")
        self.dY = torch.zeros(ld * pa.n, dtype=dt, device="cuda")
        self.dObjCol = torch.zeros(pa.n, dtype=torch.float64, device="cuda")
        self.dObjRow = torch.zeros(pa.m, dtype=torch.float64, device="cuda")
        self.api.bind_buffers(self.h, self.dX.data_ptr(), self.dY.data_ptr(), self.dObjCol.data_ptr(), self.dObjRow.data_ptr())
        self.ld = ld

    def factors(self):
        X, Y = np.zeros((self.pa.k, self.pa.m), order="F"), np.zeros((self.pa.k, self.pa.n), order="F")
        self.api.get_factors(self.h, X, Y)
        return X, Y

    def objcol(self):
        self.api.synchronize(self.h)
        return self.dObjCol.cpu().numpy().copy()

    def objrow(self):
        self.api.synchronize(self.h)
        return self.dObjRow.cpu().numpy().copy()

    def close(self):
        self.api.destroy(self.h)


# ------------------------------------------------------------------ 1. bit for bit against the host reference

CASES = [(5, 4, 2, 1, (S.REG_QUAD, 0, 0.3)), (32, 4, 8, 4, (S.REG_NONNEG, 0, 1.0)), (64, 8, 8, 1, (S.REG_QUAD, 0, 0.3)),
         (100, 16, 8, 8, (S.REG_ZERO, 0, 1.0))]


@pytest.mark.parametrize("k,G,R,waves,reg", CASES, ids=[f"k{c[0]}-w{c[3]}" for c in CASES])
def test_half_steps_equal_the_host_reference_bit_for_bit(k, G, R, waves, reg):
    """Rows of 0, 1, TG and TG U + 1 observations (TG = lane groups of the segment's waves, U = observations a group keeps in flight): the
    empty segment, one group with work, every group with one observation, one trip more than a full one.  Three outer iterations."""
    TG = (64 // G) * waves
    U = 8 if waves == 8 else 2
    m, n = 4, 16
    pa, X0, Y0 = small_problem(m, n, k, [0, 1, TG, TG * U + 1], seed=1000 + k, reg=reg)
    pa, X0, Y0 = make_representable(pa, X0, Y0, nonneg=reg[0] == S.REG_NONNEG)
    want = S.trajectory(pa, X0, Y0, G, R, reg, 3, waves=waves, min_stepsize=0.01)
    b = Bound(pa, 1, waves_row=waves, waves_col=waves)
    api, h = b.api, b.h
    try:
        assert api.storage(h) == _capi.STORAGE_F32
        for which in (0, 1):
            o = api.sum_order(h, which).asdict()
            assert (o["family_name"], o["lanes"], o["comps"], o["waves"], o["cached_maxlen"]) == ("strided", G, R, waves, -1), o
        assert api.kernel_stats(h)["tiled"] == 0
        api.set_factors(h, X0, Y0)
        api.reset_stepsizes(h, 1.0)
        for it, (X1, Y2, objcol, tx, ty, _) in enumerate(want):
            api.step_x(h, 0.01)
            Xg, Yg = b.factors()
            assert np.array_equal(Xg, X1), (it, np.abs(Xg - X1).max())
            assert np.array_equal(Yg, want[it - 1][1] if it else Y0)
            api.step_y(h, 0.01)
            Xg, Yg = b.factors()
            assert np.array_equal(Yg, Y2), (it, np.abs(Yg - Y2).max())
            assert np.array_equal(Xg, X1)
            assert S.is_f32(Xg) and S.is_f32(Yg)
            st = api.kernel_stats(h)
            assert (st["trials_x"], st["trials_y"]) == (tx, ty)
            assert np.array_equal(b.objcol(), objcol)
        # the bound float buffers hold the factors with leading dimension ld and zero padding
        dX = b.dX.cpu().numpy().reshape(m, b.ld)
        assert np.array_equal(dX[:, :k].astype(np.float64), want[-1][0].T) and not dX[:, k:].any()
    finally:
        b.close()


# ------------------------------------------------------------------ 2. against an fp64 gather handle on float-representable data

def mixed_problem(single=None, m=60, n=27, k=8, seed=5):
    """Columns cycle through the nine scalar loss kinds (or all carry `single`); values each kind accepts, all float-representable."""
    rng = np.random.default_rng(seed)
    kinds = [L.QuadLoss(0.8), L.L1Loss(0.6), L.HuberLoss(1.1, crossover=0.7), L.QuantileLoss(0.9, quantile=0.3), L.PeriodicLoss(2.5, 0.8),
             L.PoissonLoss(20), L.OrdinalHingeLoss(1, 5, 0.9), L.LogisticLoss(0.7), L.WeightedHingeLoss(1.2, case_weight_ratio=2.0)]
    objs = [single] * n if single is not None else [kinds[f % 9] for f in range(n)]
    mask = rng.random((m, n)) < 0.5
    mask[3, :] = False                       # an empty row
    mask[:, 4] = False                       # and an empty column
    A = np.zeros((m, n))
    for f, lo in enumerate(objs):
        if isinstance(lo, L.PoissonLoss):
            A[:, f] = rng.integers(0, 6, m)
        elif isinstance(lo, L.OrdinalHingeLoss):
            A[:, f] = rng.integers(1, 6, m)
        elif isinstance(lo, (L.LogisticLoss, L.WeightedHingeLoss)):
            A[:, f] = rng.random(m) < 0.5
        else:
            A[:, f] = rng.standard_normal(m).astype(np.float32)
    I, J = np.nonzero(mask)                  # row-major: the row view in order
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=m))]).astype(np.int64)
    colidx, rowvals = J.astype(np.int32), A[I, J]
    order = np.lexsort((I, J))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(J, minlength=n))]).astype(np.int64)
    rowidx, colvals = I[order].astype(np.int32), A[I, J][order]
    losses = np.array([lo.descriptor() for lo in (objs if single is None else objs[:1])], dtype=_capi.LOSS_DTYPE)
    r = np.array([(S.REG_QUAD, 0, 0.2)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, colidx, rowvals, colptr, rowidx, colvals, losses, r, r)
    return pa, f32r(0.3 * rng.standard_normal((k, m))), f32r(0.3 * rng.standard_normal((k, n)))


@pytest.mark.parametrize("single", [None, "huber"], ids=["nine-kinds", "one-huber"])
def test_f32_handle_equals_an_fp64_gather_handle_on_representable_data(single):
    """Nine kinds by column: LOSS_SEGMENT by segment on the column view, LOSS_PER_OBS with four observations per trip and one loss
    evaluation per lane on the row view (G = 4).  One HuberLoss: LOSS_SEGMENT with one descriptor on both views."""
    pa, X0, Y0 = mixed_problem(L.HuberLoss(1.1, crossover=0.7) if single else None)
    b32, b64 = Bound(pa, 1), Bound(pa, 0, tiled=1)
    api = b32.api
    try:
        assert api.storage(b64.h) == _capi.STORAGE_F64 and api.kernel_stats(b64.h)["tiled"] == 0
        # (a) the objective at the same representable point
        for reg in (True, False):
            assert api.objective(b32.h, X0, Y0, reg) == api.objective(b64.h, X0, Y0, reg)
        # (b) one iteration on the f32 handle; the losses of its (widened) factors on both handles
        api.reset_stepsizes(b32.h, 1.0)
        api.step_x(b32.h, 0.01)
        api.step_y(b32.h, 0.01)
        step_obj = b32.objcol()
        X1, Y1 = b32.factors()
        assert S.is_f32(X1) and S.is_f32(Y1) and not np.array_equal(X1, X0) and not np.array_equal(Y1, Y0)
        api.col_losses(b32.h)
        loss32 = b32.objcol()
        api.set_factors(b64.h, X1, Y1)
        api.col_losses(b64.h)
        assert np.array_equal(loss32, b64.objcol())
        api.row_penalties(b32.h)
        api.row_penalties(b64.h)
        assert np.array_equal(b32.objrow(), b64.objrow())
        # (c) what step_y recorded is the objective of what it stored: a trial evaluated before the rounding would miss by ~1e-8, the
        # fp64 sums of these list lengths in another order stay below 1e-13
        api.col_penalties(b32.h)
        total = loss32 + b32.objcol()
        err = np.abs(step_obj - total) / np.abs(total)
        print("step_y objective vs col_losses + col_penalties, max relative:", err.max())
        assert err.max() < 1e-12
        st = api.kernel_stats(b32.h)
        assert st["accepts_x"] > 0 and st["accepts_y"] > 0
    finally:
        b32.close()
        b64.close()


# ------------------------------------------------------------------ 3. fit: NNMF

def nnmf_problem(m=300, n=200, k=8, per_row=20, seed=7):
    rng = np.random.default_rng(seed)
    A = np.abs(rng.standard_normal((m, k))) @ np.abs(rng.standard_normal((k, n))) + 0.05 * np.abs(rng.standard_normal((m, n)))
    rows = [np.sort(rng.choice(n, per_row, replace=False)) for _ in range(m)]
    I = np.repeat(np.arange(m), per_row)
    J = np.concatenate(rows)
    rowptr = (np.arange(m + 1) * per_row).astype(np.int64)
    order = np.lexsort((I, J))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(J, minlength=n))]).astype(np.int64)
    losses = np.array([(0, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    r = np.array([(S.REG_NONNEG, 0, 1.0)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, J.astype(np.int32), A[I, J], colptr, I[order].astype(np.int32), A[I, J][order], losses, r, r)
    return pa, np.asfortranarray(np.abs(rng.standard_normal((k, m)))), np.asfortranarray(np.abs(rng.standard_normal((k, n))))


def test_fit_nnmf_decreases_and_returns_representable_nonnegative_factors():
    """(The fp64 oracle's trajectory on this input is itself non-increasing: checked when the test was written.)"""
    pa, X0, Y0 = nnmf_problem()
    prm = L.ProxGradParams(max_iter=20, abs_tol=-1e300, rel_tol=-1e300)
    api = _capi.hip_api()
    res = {}
    for storage in (1, 0):
        h = api.create(pa, storage=storage, tiled=1)
        try:
            X, Y = X0.copy(order="F"), Y0.copy(order="F")
            obj, sec = api.fit(h, prm, X, Y)
            res[storage] = (obj, sec, X, Y)
        finally:
            api.destroy(h)
    obj, sec, X, Y = res[1]
    assert len(obj) == len(sec) == 21 == len(res[0][0])
    assert sec[0] == 0.0 and np.all(np.diff(sec) > 0)
    assert np.all(np.isfinite(obj))
    assert all(obj[i + 1] <= obj[i] for i in range(1, 20)), obj
    assert obj[-1] < 0.5 * obj[1]
    assert S.is_f32(X) and S.is_f32(Y) and X.min() >= 0 and Y.min() >= 0
    assert not (S.is_f32(res[0][2]) and S.is_f32(res[0][3]))  # (the fp64 handle's factors are not: the property is the mode's)


# ------------------------------------------------------------------ 4. trajectory against the fp64 oracle

#: max_i |J32_i - J64_i| / J64_i over the 50 iterations below, measured once on the MI355X
TRAJECTORY_MEASURED = 8.713e-06


def test_trajectory_stays_near_the_fp64_oracle():
    """QuadLoss, QuadReg(0.1), 2 000 x 500, k = 32, 50 iterations.  The bound is 4 x the measured value: the margin allows for one
    line-search decision falling the other way."""
    rowptr, colidx, rowvals, colptr, rowidx, colvals, X0, Y0 = O.synth_cpu(2000, 500, 32, 50)   # 50 observations per row: 10 % observed
    losses = np.array([(0, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    r = np.array([(S.REG_QUAD, 0, 0.1)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(2000, 500, 32, rowptr, colidx, rowvals, colptr, rowidx, colvals, losses, r, r)
    X0, Y0 = np.asfortranarray(0.3 * X0), np.asfortranarray(0.3 * Y0)
    prm = L.ProxGradParams(max_iter=50, abs_tol=-1e300, rel_tol=-1e300)
    api, oapi = _capi.hip_api(), O.oracle_api()
    h = api.create(pa, storage=1)
    try:
        X, Y = X0.copy(order="F"), Y0.copy(order="F")
        j32, _ = api.fit(h, prm, X, Y)
    finally:
        api.destroy(h)
    O.set_threads(O.usable_cores())
    ho = oapi.create(pa)
    try:
        X, Y = X0.copy(order="F"), Y0.copy(order="F")
        j64, _ = oapi.fit(ho, prm, X, Y)
    finally:
        oapi.destroy(ho)
    assert len(j32) == len(j64) == 51
    dev = float(np.max(np.abs(j32 - j64) / j64))
    print(f"storage f32 vs fp64 oracle, max relative objective deviation over 50 iterations: {dev:.3e}")
    assert dev <= 4 * TRAJECTORY_MEASURED, (dev, TRAJECTORY_MEASURED)


# ------------------------------------------------------------------ 5. narrowing

def test_narrowing_is_the_float_conversion_and_overflow_is_refused():
    pa, X0, Y0 = small_problem(6, 20, 5, [3, 9], seed=2, reg=(S.REG_QUAD, 0, 0.3))
    X0, Y0 = f32r(X0), f32r(Y0)
    pa.rowvals[:] = 0.1
    pa.colvals[:] = 0.1
    api = _capi.hip_api()
    h32 = api.create(pa, storage=1)
    pa.rowvals[:] = float(np.float32(0.1))
    pa.colvals[:] = float(np.float32(0.1))
    h64 = api.create(pa, tiled=1)
    try:
        assert api.objective(h32, X0, Y0) == api.objective(h64, X0, Y0)
        # factors handed in as doubles are narrowed the same way
        Xd, Yd = X0 + 1e-9, Y0 * (1 + 1e-9)
        assert not S.is_f32(Xd)
        assert api.objective(h32, Xd, Yd) == api.objective(h64, f32r(Xd), f32r(Yd))
        Xg, Yg = np.zeros_like(X0), np.zeros_like(Y0)
        api.get_factors(h32, Xg, Yg)
        assert np.array_equal(Xg, f32r(Xd)) and np.array_equal(Yg, f32r(Yd))
        # a finite double beyond float's range
        Xbig = X0.copy(order="F")
        Xbig[1, 2] = 1e39
        with pytest.raises(_capi.GLRMError) as e:
            api.set_factors(h32, Xbig, Y0)
        assert e.value.code == NONFINITE and "f32" in e.value.message
        api.get_factors(h32, Xg, Yg)
        assert np.array_equal(Xg, f32r(Xd))  # the handle's factors were not touched
        Ybig = Y0.copy(order="F")
        Ybig[0, 0] = -1e39
        with pytest.raises(_capi.GLRMError) as e:
            api.objective(h32, X0, Ybig)
        assert e.value.code == NONFINITE
        api.set_factors(h64, Xbig, Y0)      # (fine in fp64)
    finally:
        api.destroy(h32)
        api.destroy(h64)
    pa.rowvals[4] = 1e39
    with pytest.raises(_capi.GLRMError) as e:
        api.create(pa, storage=1)
    assert e.value.code == NONFINITE and "f32" in e.value.message
    pa.rowvals[4] = np.nan                   # the NaN check comes first and reads the doubles
    with pytest.raises(_capi.GLRMError) as e:
        api.create(pa, storage=1)
    assert e.value.code == NONFINITE and "NaN" in e.value.message


# ------------------------------------------------------------------ 6. refusals

def expect(code, fn, *a, **kw):
    with pytest.raises(_capi.GLRMError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, e.value.message)
    if code == UNSUPPORTED:
        assert "f32" in e.value.message, e.value.message
    return e.value.message


def test_refusals_name_the_mode_and_leave_the_handle_usable():
    pa, X0, Y0 = small_problem(12, 20, 5, [3, 9], seed=3, reg=(S.REG_QUAD, 0, 0.3))
    pa, X0, Y0 = make_representable(pa, X0, Y0)
    api = _capi.hip_api()
    m, n, k = pa.m, pa.n, pa.k
    # at create
    expect(INVALID, api.create, pa, storage=2)
    expect(INVALID, api.create, pa, storage=-1)
    expect(UNSUPPORTED, api.create, pa, storage=1, sum_order=1)
    expect(UNSUPPORTED, api.create, pa, storage=1, tiled=2)
    expect(UNSUPPORTED, api.create, pa, storage=1, quad_gram=1)
    expect(UNSUPPORTED, api.create, pa, storage=1, defer=True)
    expect(UNSUPPORTED, api.multi_create, pa, 1, storage=1)
    expect(INVALID, api.multi_create, pa, 1, storage=2)
    expect(UNSUPPORTED, api.scale_columns, pa, _capi.SCALE_EQUILIBRATE, storage=1)
    A = np.ascontiguousarray(np.random.default_rng(0).standard_normal((m, n)))
    dense = _capi.ProblemArrays(m, n, k, None, None, None, None, None, None, pa.losses, pa.rx, pa.ry, dense_A=A, dense_ld=n, dense_colmajor=0)
    expect(UNSUPPORTED, api.create, dense, storage=1)

    def with_(**kw):
        q = _capi.ProblemArrays(m, n, k, pa.rowptr, pa.colidx, pa.rowvals, pa.colptr, pa.rowidx, pa.colvals, pa.losses, pa.rx, pa.ry)
        for key, v in kw.items():
            setattr(q, key, v)
        return q
    wrapped = np.array([(S.REG_QUAD, 1, 0.3)], dtype=_capi.REG_DTYPE)      # lastentry1(QuadReg)
    vector = np.array([(5, 0, 1.0)], dtype=_capi.REG_DTYPE)               # QuadConstraint
    expect(UNSUPPORTED, api.create, with_(rx=wrapped), storage=1)
    expect(UNSUPPORTED, api.create, with_(ry=vector), storage=1)
    mnl = np.array([L.MultinomialLoss(4).descriptor()], dtype=_capi.LOSS_DTYPE)
    levels = with_(losses=mnl, rowvals=np.ones_like(pa.rowvals), colvals=np.ones_like(pa.colvals))
    expect(UNSUPPORTED, api.create, levels, storage=1)

    # on a handle
    h0 = api.create(pa)
    h = api.create(pa, storage=1)
    try:
        assert api.storage(h0) == 0 and api.storage(h) == 1
        before = api.objective(h, X0, Y0)
        api.reset_stepsizes(h, 1.0)
        expect(UNSUPPORTED, api.set_regularizers, h, wrapped, pa.ry)
        expect(UNSUPPORTED, api.set_regularizers, h, pa.rx, vector)
        expect(UNSUPPORTED, api.step_x_range, h, 0, m, 0.01)
        expect(UNSUPPORTED, api.step_y_arrival, h, 0.01, [(0, m, 0)])
        expect(UNSUPPORTED, api.gradstep_x, h, 0.1)
        expect(UNSUPPORTED, api.gradstep_y, h, 0.1)
        expect(UNSUPPORTED, api.fit_sparse, h, L.SparseProxGradParams(max_iter=2), X0.copy(order="F"), Y0.copy(order="F"))
        expect(UNSUPPORTED, api.subset, h, np.ones(len(pa.colidx), np.uint8), np.ones(len(pa.rowidx), np.uint8), 1)
        expect(UNSUPPORTED, api.init_svd, h, X0.copy(order="F"), Y0.copy(order="F"))
        dom = np.zeros(n, dtype=_capi.DOMAIN_DTYPE)
        expect(UNSUPPORTED, api.impute, h, X0, Y0, dom, m, n)
        expect(UNSUPPORTED, api.error_metric, h, X0, Y0, dom)
        expect(UNSUPPORTED, api.init_kmeanspp, h, np.asfortranarray(Y0.copy()), 0, np.full(k - 1, 0.5))
        # none of them touched the handle: the factors are where objective() left them, and the half-steps run
        Xg, Yg = np.zeros_like(X0), np.zeros_like(Y0)
        api.get_factors(h, Xg, Yg)
        assert np.array_equal(Xg, X0) and np.array_equal(Yg, Y0)
        assert api.objective(h, X0, Y0) == before
        api.set_regularizers(h, np.array([(S.REG_QUAD, 0, 0.5)], dtype=_capi.REG_DTYPE), np.array([(S.REG_NONNEG, 0, 1.0)], dtype=_capi.REG_DTYPE))
        api.step_x(h, 0.01)
        api.step_y(h, 0.01)
        api.get_factors(h, Xg, Yg)
        assert S.is_f32(Xg) and S.is_f32(Yg) and Yg.min() >= 0 and not np.array_equal(Xg, X0)
    finally:
        api.destroy(h)
        api.destroy(h0)


# ------------------------------------------------------------------ 7. leaks

def test_create_and_destroy_release_the_device_memory():
    import torch
    pa, X0, Y0 = nnmf_problem()
    api = _capi.hip_api()

    def cycle():
        h = api.create(pa, storage=1)
        try:
            api.set_factors(h, X0, Y0)
            api.reset_stepsizes(h, 1.0)
            api.step_x(h, 0.01)
            api.step_y(h, 0.01)
            X, Y = np.zeros_like(X0), np.zeros_like(Y0)
            api.get_factors(h, X, Y)
            api.objective(h, X, Y)
        finally:
            api.destroy(h)

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    cycle()
    cycle()
    levels = [free_bytes()]
    for _ in range(2):       # two windows of ten: a leak loses memory in both, a one-off growth of a runtime pool in one
        for _ in range(10):
            cycle()
        levels.append(free_bytes())
    lost = [levels[i] - levels[i + 1] for i in range(2)]
    assert min(lost) < 4 << 20, f"device memory lost per window of 10 create / destroy cycles (MiB): {[round(x / 2**20, 2) for x in lost]}"


# ------------------------------------------------------------------ 8. the Python mirror

def test_fit_with_storage_f32_through_the_python_layer():
    rng = np.random.default_rng(4)
    m, n, k = 120, 80, 6
    A = rng.standard_normal((m, k)) @ rng.standard_normal((k, n)) + 0.1 * rng.standard_normal((m, n))
    obs = np.nonzero(rng.random((m, n)) < 0.4)
    g = L.GLRM(A, L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.1), k, obs=obs, X=rng.standard_normal((k, m)), Y=rng.standard_normal((k, n)))
    api = _capi.hip_api()
    try:
        _, _, ch = L.fit_b(g, L.HipProxGradParams(storage="f32", max_iter=15), verbose=False)
        h = g._handle_cache[1]
        assert api.storage(h) == _capi.STORAGE_F32
        assert g.X.dtype == np.float64 and g.Y.dtype == np.float64 and S.is_f32(g.X) and S.is_f32(g.Y)
        assert ch.objective[-1] < ch.objective[0]
        first = h.value
        _, _, ch2 = L.fit_b(g, L.HipProxGradParams(storage="f32", max_iter=5), verbose=False)   # warm start on the same handle
        assert g._handle_cache[1].value == first and api.storage(g._handle_cache[1]) == _capi.STORAGE_F32
        assert ch2.objective[-1] <= ch2.objective[0] < ch.objective[0]
        _, _, ch3 = L.fit_b(g, L.HipProxGradParams(storage="f64", max_iter=5), verbose=False)   # another storage: a handle of its own
        assert api.storage(g._handle_cache[1]) == _capi.STORAGE_F64
        assert ch3.objective[-1] <= ch3.objective[0] and not (S.is_f32(g.X) and S.is_f32(g.Y))
        # a fully observed model is handed over as lists, not as dense_A; a model the mode refuses raises
        gd = L.GLRM(A, L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), k)
        try:
            L.fit_b(gd, L.HipProxGradParams(storage="f32", max_iter=3), verbose=False)
            assert api.storage(gd._handle_cache[1]) == 1 and api.kernel_stats(gd._handle_cache[1])["tiled"] == 0 and S.is_f32(gd.X)
        finally:
            gd.close()
        gv = L.GLRM(A, L.QuadLoss(), L.QuadConstraint(2.0), L.ZeroReg(), k, obs=obs)
        try:
            with pytest.raises(_capi.GLRMError) as e:
                L.fit_b(gv, L.HipProxGradParams(storage="f32", max_iter=3), verbose=False)
            assert e.value.code == UNSUPPORTED and "f32" in e.value.message
        finally:
            gv.close()
    finally:
        g.close()
