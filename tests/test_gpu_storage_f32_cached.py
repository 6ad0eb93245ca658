"""-m gpu: glrm_options.storage = 1 on the cached row sweep (csrc/glrm_cached.hpp, csrc/glrm_cached_f32.hip) --
a row's opposing vectors fetched once per half-step and held in registers as floats, every sum in fp64 in the order of the fp64 kernels.

Every case forces the family with GLRM_HIP_CACHED=1 on a `storage=1, tiled=1` handle: no committed shape is large enough for the auto
rule.  The half-steps are held to the lane-by-lane host reference bit for bit (tests/storage_f32_cached_ref.py, pinned to the CPU oracle
by tests/test_storage_f32_cached.py); the persistent kernel to the one-row-per-workgroup kernel; the loss kinds the reference does not
model to the float gather sweep, which adds a short row on one wave instead of two."""
import functools

import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import storage_f32_cached_ref as SC
import storage_f32_ref as S
from lowrankmodels.jl_amd import _capi
from test_gpu_storage_f32 import Bound, expect, f32r, make_representable
from test_gpu_sum_order import engine_and_oracle_in_its_order, problem as synth_problem
from test_sum_order import small_problem

pytestmark = pytest.mark.gpu

UNSUPPORTED = _capi.ERR_UNSUPPORTED
CACHED = 64
N = 131

#: name -> (k, G, R, regularizer, row lengths, rows): the three problems of the bit-for-bit test
PROBLEMS = {
    "k64-quadreg-maxt7": (64, 8, 8, (S.REG_QUAD, 0, 0.1), SC.LENS_K64, 4 * len(SC.LENS_K64)),
    "k64-nonneg-maxt4": (64, 8, 8, (S.REG_NONNEG, 0, 1.0), SC.LENS_K64_SHORT, len(SC.LENS_K64_SHORT)),
    "k20-zeroreg-g4": (20, 4, 8, (S.REG_ZERO, 0, 1.0), SC.LENS_K20, 3 * len(SC.LENS_K20)),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(problem, start, two iterations of the host reference): computed once, shared by the cases, never written to."""
    k, G, R, reg, lens, m = PROBLEMS[name]
    pa, X0, Y0 = small_problem(m, N, k, lens, seed=k + len(lens), reg=reg)
    pa, X0, Y0 = make_representable(pa, X0, Y0, nonneg=reg[0] == S.REG_NONNEG)
    want = SC.trajectory(pa, X0, Y0, G, R, reg, 2, min_stepsize=0.01)
    for a in (X0, Y0):
        a.setflags(write=False)
    return pa, X0, Y0, want


def family_handle(monkeypatch, pa, persist=None, **kw):
    monkeypatch.setenv("GLRM_HIP_CACHED", "1")
    if persist is not None:
        monkeypatch.setenv("GLRM_HIP_CACHED_PERSIST", str(persist))
    return Bound(pa, 1, tiled=1, **kw)


# ------------------------------------------------------------------ 1. the family runs and says so

@pytest.mark.parametrize("k,G,maxlen", [(64, 8, 104), (20, 4, 208), (32, 4, 208)])
def test_the_family_runs_on_a_float_handle_and_reports_it(monkeypatch, k, G, maxlen):
    pa, X0, Y0 = small_problem(24, N, k, [0, 1, 9, 40, maxlen, maxlen + 1], seed=k, reg=(S.REG_QUAD, 0, 0.1))
    pa, X0, Y0 = make_representable(pa, X0, Y0)
    monkeypatch.setenv("GLRM_HIP_CACHED_REGS", "0")     # ignored for float storage: there is no float LDS variant
    monkeypatch.setenv("GLRM_HIP_CACHED_WAVES", "4")    # ignored as well
    b = family_handle(monkeypatch, pa)
    try:
        api, h = b.api, b.h
        assert api.storage(h) == _capi.STORAGE_F32
        assert api.kernel_stats(h)["tiled"] & CACHED, api.kernel_stats(h)["tiled"]
        assert api.kernel_stats(h)["tiled"] == CACHED      # tiled_* and blocked_* stay 0
        o = api.sum_order(h, 0).asdict()
        assert (o["family_name"], o["lanes"], o["comps"], o["cached_waves"], o["cached_maxlen"]) == ("strided", G, 8, 2, maxlen), o
        assert api.sum_order(h, 1).asdict()["cached_maxlen"] == -1
        api.set_factors(h, X0, Y0)
        api.reset_stepsizes(h, 1.0)
        api.step_x(h, 0.01)
        X1, _ = b.factors()
        assert S.is_f32(X1) and not np.array_equal(X1, X0)
        assert api.kernel_stats(h)["accepts_x"] > 0
    finally:
        b.close()
    # switched off, and without the variable on a tiled = 1 handle: the float gather sweeps, reported as before
    for setting in ("0", None):
        if setting is None:
            monkeypatch.delenv("GLRM_HIP_CACHED")
        else:
            monkeypatch.setenv("GLRM_HIP_CACHED", setting)
        b = Bound(pa, 1, tiled=1)
        try:
            assert b.api.kernel_stats(b.h)["tiled"] == 0 and b.api.sum_order(b.h, 0).asdict()["cached_maxlen"] == -1
        finally:
            b.close()


# ------------------------------------------------------------------ 2. bit for bit against the host reference

@pytest.mark.parametrize("persist", [1, 0], ids=["persistent", "row-per-workgroup"])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_half_steps_equal_the_host_reference_bit_for_bit(monkeypatch, name, persist):
    """X after every step_x, Y after every step_y, the trial totals and the bound dObjCol, over two iterations."""
    k, G, R, reg, lens, m = PROBLEMS[name]
    pa, X0, Y0, want = reference(name)
    b = family_handle(monkeypatch, pa, persist)
    api, h = b.api, b.h
    try:
        o = api.sum_order(h, 0).asdict()
        assert api.kernel_stats(h)["tiled"] == CACHED and (o["cached_waves"], o["cached_maxlen"]) == (2, SC.cached_maxlen(G))
        assert max(lens) > o["cached_maxlen"]            # the listed form: long rows beside the cached ones
        api.set_factors(h, X0, Y0)
        api.reset_stepsizes(h, 1.0)
        for it, (X1, Y2, objcol, tx, ty, _) in enumerate(want):
            api.step_x(h, 0.01)
            Xg, Yg = b.factors()
            bad = np.nonzero((Xg != X1).any(axis=0))[0]
            assert bad.size == 0, (it, "rows", bad[:8], "lengths", np.diff(pa.rowptr)[bad[:8]], np.abs(Xg - X1).max())
            assert np.array_equal(Yg, want[it - 1][1] if it else Y0)
            assert api.kernel_stats(h)["trials_x"] == tx
            api.step_y(h, 0.01)
            Xg, Yg = b.factors()
            assert np.array_equal(Yg, Y2), (it, np.abs(Yg - Y2).max())
            assert np.array_equal(Xg, X1)
            assert S.is_f32(Xg) and S.is_f32(Yg)
            st = api.kernel_stats(h)
            assert (st["trials_x"], st["trials_y"]) == (tx, ty)
            assert np.array_equal(b.objcol(), objcol)
        # the bound float buffer: leading dimension ld, and the padding beyond k is still exactly zero
        dX = b.dX.cpu().numpy().reshape(pa.m, b.ld)
        assert np.array_equal(dX[:, :k].astype(np.float64), want[-1][0].T) and not dX[:, k:].any()
        dY = b.dY.cpu().numpy().reshape(pa.n, b.ld)
        assert not dY[:, k:].any()
    finally:
        b.close()


# ------------------------------------------------------------------ 3. persistent walk against the one-row-per-workgroup kernel

POOL = [0, 1, 7, 8, 9, 16, 17, 63, 64, 65, 100, 104]
LONG = [105, 208, 300, 150] * 5


@functools.lru_cache(maxsize=None)
def walk_problem(m_short, n_long=20, n=257):
    lens = [POOL[e % len(POOL)] for e in range(m_short)] + LONG[:n_long]
    pa, X0, Y0 = small_problem(len(lens), n, 64, lens, seed=m_short, reg=(S.REG_NONNEG, 0, 1.0))
    return make_representable(pa, X0, Y0, nonneg=True)


def run_fit(monkeypatch, pa, X0, Y0, persist, iters, **prm_kw):
    prm = L.ProxGradParams(max_iter=iters, abs_tol=-1e300, rel_tol=-1e300, **prm_kw)
    monkeypatch.setenv("GLRM_HIP_CACHED", "1")
    monkeypatch.setenv("GLRM_HIP_CACHED_PERSIST", str(persist))
    api = _capi.hip_api()
    h = api.create(pa, storage=1, tiled=1)
    try:
        assert api.kernel_stats(h)["tiled"] == CACHED
        X, Y = X0.copy(order="F"), Y0.copy(order="F")
        obj, _ = api.fit(h, prm, X, Y)
        st = api.kernel_stats(h)
    finally:
        api.destroy(h)
    return X, Y, np.array(obj), {key: st[key] for key in ("trials_x", "accepts_x", "trials_y", "accepts_y")}


def both_kernels_agree(monkeypatch, pa, X0, Y0, iters, **prm_kw):
    Xp, Yp, op, sp = run_fit(monkeypatch, pa, X0, Y0, 1, iters, **prm_kw)
    Xw, Yw, ow, sw = run_fit(monkeypatch, pa, X0, Y0, 0, iters, **prm_kw)
    assert np.array_equal(Xp, Xw), np.abs(Xp - Xw).max()
    assert np.array_equal(Yp, Yw), np.abs(Yp - Yw).max()
    assert np.array_equal(op, ow), (op, ow)
    assert sp == sw, (sp, sw)
    assert S.is_f32(Xp) and S.is_f32(Yp)
    return sp


@pytest.mark.parametrize("case", ["stepsize-1", "stepsize-1e3", "rows-give-up"])
def test_persistent_walk_equals_one_row_per_workgroup(monkeypatch, case):
    """12 301 cached rows and twenty long ones: the resident grid of 128-thread workgroups is at most 16 per CU x 256 CUs = 4 096, so every
    workgroup walks at least three rows and the last round is ragged.  Three iterations."""
    pa, X0, Y0 = walk_problem(12301)
    m = pa.m
    if case == "stepsize-1":
        st = both_kernels_agree(monkeypatch, pa, X0, Y0, 3)
        assert st["accepts_x"] > 0
    elif case == "stepsize-1e3":
        st = both_kernels_agree(monkeypatch, pa, X0, Y0, 3, stepsize=1e3, min_stepsize=0.01)
        print("stepsize 1e3:", st)
        assert st["trials_x"] > 3 * st["accepts_x"] > 0          # several rejections per row
    else:
        st = both_kernels_agree(monkeypatch, pa, X0, Y0, 3, stepsize=1e3, min_stepsize=0.5)
        print("stepsize 1e3, min_stepsize 0.5:", st)
        assert st["accepts_x"] < 3 * m                           # row half-steps that ended without an accepted trial


@pytest.mark.parametrize("m", [1, 127])
def test_persistent_walk_without_a_next_row(monkeypatch, m):
    """Fewer rows than resident workgroups: no next row for any workgroup (m = 1: a single row, and it is a cached one)."""
    if m == 1:
        pa, X0, Y0 = make_representable(*small_problem(1, N, 64, [100], seed=1, reg=(S.REG_NONNEG, 0, 1.0)), nonneg=True)
    else:
        pa, X0, Y0 = walk_problem(m, n_long=2, n=N)
    st = both_kernels_agree(monkeypatch, pa, X0, Y0, 2)
    assert st["accepts_x"] > 0


# ------------------------------------------------------------------ 4. every scalar loss kind, against the float gather sweep

def kinds_problem(model, m=600, n=N, k=64, seed=9):
    """Rows of 1 ... 104 observations; columns cycle through the scalar loss kinds (or all carry one HuberLoss); float-representable."""
    rng = np.random.default_rng(seed)
    kinds = [L.QuadLoss(0.8), L.L1Loss(0.6), L.HuberLoss(1.1, crossover=0.7), L.QuantileLoss(0.9, quantile=0.3), L.PeriodicLoss(2.5, 0.8),
             L.PoissonLoss(20), L.OrdinalHingeLoss(1, 5, 0.9), L.LogisticLoss(0.7), L.WeightedHingeLoss(1.2, case_weight_ratio=2.0)]
    if model == "eight-kinds-no-trig":
        kinds = [lo for lo in kinds if not isinstance(lo, L.PeriodicLoss)]
    objs = [L.HuberLoss(1.1, crossover=0.7)] * n if model == "one-huber" else [kinds[f % len(kinds)] for f in range(n)]
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
    rows = [np.sort(rng.choice(n, 1 + e % 104, replace=False)) for e in range(m)]
    I = np.repeat(np.arange(m), [len(r) for r in rows])
    J = np.concatenate(rows)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    order = np.lexsort((I, J))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(J, minlength=n))]).astype(np.int64)
    losses = np.array([lo.descriptor() for lo in (objs[:1] if model == "one-huber" else objs)], dtype=_capi.LOSS_DTYPE)
    r = np.array([(S.REG_QUAD, 0, 0.2)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, J.astype(np.int32), A[I, J], colptr, I[order].astype(np.int32), A[I, J][order], losses, r, r)
    return pa, f32r(0.1 * rng.standard_normal((k, m))), f32r(0.1 * rng.standard_normal((k, n)))


@pytest.mark.parametrize("model", ["nine-kinds", "eight-kinds-no-trig", "one-huber"])
def test_every_scalar_loss_kind_against_the_float_gather_sweep(monkeypatch, model):
    """One step_x from the same start on a handle with the family (a row on two waves) and on a tiled = 1 handle without the variable (the
    float gather sweep: the row on one wave).  The two orders differ, so an entry may differ by a last float bit where a component sits on
    a rounding boundary, and a line search can in principle fall the other way: at most 1 % of the rows may hold an entry further than
    one float ulp from the other handle's, and in the remaining rows every entry is within that ulp."""
    pa, X0, Y0 = kinds_problem(model)
    fam = family_handle(monkeypatch, pa)
    monkeypatch.delenv("GLRM_HIP_CACHED")
    plain = Bound(pa, 1, tiled=1)
    try:
        api = fam.api
        assert api.kernel_stats(fam.h)["tiled"] == CACHED and api.kernel_stats(plain.h)["tiled"] == 0
        out = []
        for b in (fam, plain):
            api.set_factors(b.h, X0, Y0)
            api.reset_stepsizes(b.h, 1.0)
            api.step_x(b.h, 0.01)
            out.append(b.factors()[0])
            assert api.kernel_stats(b.h)["accepts_x"] > 0.9 * pa.m
        Xf, Xp = out
        assert not np.array_equal(Xf, X0)
        ulp = np.spacing(np.maximum(np.abs(Xf), np.abs(Xp)).astype(np.float32)).astype(np.float64)
        within = np.abs(Xf - Xp) <= ulp
        bad = ~within.all(axis=0)
        print(f"{model}: rows with an entry beyond one float ulp: {int(bad.sum())} of {pa.m}; entries that differ at all: "
              f"{int((Xf != Xp).sum())} of {Xf.size}; trials {api.kernel_stats(fam.h)['trials_x']} / {api.kernel_stats(plain.h)['trials_x']}")
        assert bad.mean() <= 0.01, int(bad.sum())
        assert within[:, ~bad].all()
    finally:
        fam.close()
        plain.close()


# ------------------------------------------------------------------ 5. the Python layer

def test_fit_through_the_python_layer_and_an_fp64_fit_afterwards(monkeypatch):
    """3 000 x 400 NNMF, rank 32, 12 % observed: rows average 48 observations, all of them cached rows."""
    monkeypatch.setenv("GLRM_HIP_CACHED", "1")
    rng = np.random.default_rng(12)
    m, n, k = 3000, 400, 32
    A = np.abs(rng.standard_normal((m, 6))) @ np.abs(rng.standard_normal((6, n))) + 0.05 * np.abs(rng.standard_normal((m, n)))
    obs = np.nonzero(rng.random((m, n)) < 0.12)
    g = L.GLRM(A, L.QuadLoss(), L.NonNegConstraint(), L.NonNegConstraint(), k, obs=obs, X=np.abs(rng.standard_normal((k, m))) / 4,
               Y=np.abs(rng.standard_normal((k, n))) / 4)
    api = _capi.hip_api()
    try:
        prm = L.HipProxGradParams(storage="f32", tiled=1, max_iter=12, abs_tol=-1e300, rel_tol=-1e300)
        _, _, ch = L.fit_b(g, prm, verbose=False)
        h = g._handle_cache[1]
        assert api.storage(h) == _capi.STORAGE_F32 and api.kernel_stats(h)["tiled"] & CACHED
        obj = list(ch.objective)
        assert len(obj) == 13 and all(obj[i + 1] <= obj[i] for i in range(1, 12)), obj
        assert S.is_f32(g.X) and S.is_f32(g.Y) and g.X.min() >= 0 and g.Y.min() >= 0
        first = h.value
        _, _, ch2 = L.fit_b(g, L.HipProxGradParams(storage="f32", tiled=1, max_iter=3), verbose=False)   # warm start on the same handle
        assert g._handle_cache[1].value == first and api.kernel_stats(g._handle_cache[1])["tiled"] & CACHED
        assert ch2.objective[-1] <= ch2.objective[0] <= obj[-1]
        # an fp64 handle on the family in the same process still lands on its oracle bit for bit (its resident grid is its own)
        pa, X0, Y0 = synth_problem(3000, 400, 32, 50, (3, 0, 1.0), value_model=1)
        o = engine_and_oracle_in_its_order(pa, X0, Y0, 4, CACHED, ("strided", "strided"), tiled=1)
        assert o[0].cached_maxlen == 208 and o[0].cached_waves == 2
    finally:
        g.close()


# ------------------------------------------------------------------ 6. trajectory against the fp64 oracle

#: max_i |J32_i - J64_i| / J64_i over the 50 iterations below with the family on, measured once on the MI355X
TRAJECTORY_MEASURED = 8.713e-06


def test_trajectory_stays_near_the_fp64_oracle(monkeypatch):
    """The sibling's recipe (tests/test_gpu_storage_f32.py): QuadLoss, QuadReg(0.1), 2 000 x 500, k = 32, 50 observations per row, 50
    iterations; the float handle with the family on against the fp64 CPU oracle in reference order.  The bound is 4 x the measured value:
    the margin for one line-search decision falling the other way."""
    import oracle as O
    monkeypatch.setenv("GLRM_HIP_CACHED", "1")
    rowptr, colidx, rowvals, colptr, rowidx, colvals, X0, Y0 = O.synth_cpu(2000, 500, 32, 50)
    losses = np.array([(0, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    r = np.array([(S.REG_QUAD, 0, 0.1)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(2000, 500, 32, rowptr, colidx, rowvals, colptr, rowidx, colvals, losses, r, r)
    X0, Y0 = np.asfortranarray(0.3 * X0), np.asfortranarray(0.3 * Y0)
    prm = L.ProxGradParams(max_iter=50, abs_tol=-1e300, rel_tol=-1e300)
    api, oapi = _capi.hip_api(), O.oracle_api()
    h = api.create(pa, storage=1, tiled=1)
    try:
        assert api.kernel_stats(h)["tiled"] == CACHED
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
    print(f"storage f32 on the cached row sweep vs fp64 oracle, max relative objective deviation over 50 iterations: {dev:.3e}")
    assert dev <= 4 * TRAJECTORY_MEASURED, (dev, TRAJECTORY_MEASURED)


# ------------------------------------------------------------------ 7. what stays refused stays refused; leaks

def test_refusals_on_a_handle_with_the_family(monkeypatch):
    pa, X0, Y0 = small_problem(12, N, 64, [3, 9, 50, 120], seed=3, reg=(S.REG_QUAD, 0, 0.3))
    pa, X0, Y0 = make_representable(pa, X0, Y0)
    m, n = pa.m, pa.n
    b = family_handle(monkeypatch, pa)
    api, h = b.api, b.h
    try:
        assert api.kernel_stats(h)["tiled"] == CACHED
        api.set_factors(h, X0, Y0)
        api.reset_stepsizes(h, 1.0)
        wrapped = np.array([(S.REG_QUAD, 1, 0.3)], dtype=_capi.REG_DTYPE)      # lastentry1(QuadReg)
        vector = np.array([(5, 0, 1.0)], dtype=_capi.REG_DTYPE)               # QuadConstraint
        expect(UNSUPPORTED, api.fit_sparse, h, L.SparseProxGradParams(max_iter=2), X0.copy(order="F"), Y0.copy(order="F"))
        expect(UNSUPPORTED, api.gradstep_x, h, 0.1)
        expect(UNSUPPORTED, api.step_x_range, h, 0, m, 0.01)
        expect(UNSUPPORTED, api.set_regularizers, h, vector, pa.ry)
        expect(UNSUPPORTED, api.set_regularizers, h, wrapped, pa.ry)
        expect(UNSUPPORTED, api.subset, h, np.ones(len(pa.colidx), np.uint8), np.ones(len(pa.rowidx), np.uint8), 1)
        expect(UNSUPPORTED, api.impute, h, X0, Y0, np.zeros(n, dtype=_capi.DOMAIN_DTYPE), m, n)
        # none of them touched the handle, and the half-steps still run on the family
        Xg, Yg = b.factors()
        assert np.array_equal(Xg, X0) and np.array_equal(Yg, Y0)
        api.step_x(h, 0.01)
        api.step_y(h, 0.01)
        Xg, Yg = b.factors()
        assert S.is_f32(Xg) and S.is_f32(Yg) and not np.array_equal(Xg, X0) and api.kernel_stats(h)["tiled"] == CACHED
    finally:
        b.close()


def test_create_and_destroy_release_the_device_memory(monkeypatch):
    import torch
    monkeypatch.setenv("GLRM_HIP_CACHED", "1")
    pa, X0, Y0 = walk_problem(127, n_long=2, n=N)
    api = _capi.hip_api()

    def cycle():
        h = api.create(pa, storage=1, tiled=1)
        try:
            assert api.kernel_stats(h)["tiled"] == CACHED
            api.set_factors(h, X0, Y0)
            api.reset_stepsizes(h, 1.0)
            api.step_x(h, 0.01)
            api.step_y(h, 0.01)
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
