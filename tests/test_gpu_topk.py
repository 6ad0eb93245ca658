"""-m gpu: the top-k extension (include/glrm_hip_topk.h) and L.precision_at_k against the numpy restatement of
src/cross_validate.jl:243-304 (tests/precision_ref.py).  Every equality is exact -- q by its bits, counts and hits as integers -- because
every input is chosen so that numpy can state u_ij = the ascending fma chain without an fma: k = 1 (one rounded product), factors that
are small multiples of 1/2 or powers of two (every product and sum exact), or the engine's own chain read back through glrm_hip_impute.

The selection tests run under three settings of the engine's two launch knobs (KNOBS): the defaults; one workgroup walking every tile and
no early finish (eight counting passes); three workgroups and an early finish that only triggers below 300 entries (so it happens after
a different number of counting passes than by default).  q, n_gt and n_eq must not notice.

`train_time` of the driver is a wall clock: it is the one returned array that two runs cannot share, and is checked for its shape and for
being finite and non-decreasing instead (the history's clock accumulates over the path)."""
import ctypes as C

import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import precision_ref as R
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.losses import pack_losses
from lowrankmodels.jl_amd.regularizers import pack_regs

pytestmark = pytest.mark.gpu

KNOBS = [(None, None), ("0", "1"), ("300", "3")]   # (GLRM_HIP_TOPK_FINISH, GLRM_HIP_TOPK_GRID)


def hip():
    return _capi.hip_api()


@pytest.fixture(params=KNOBS, ids=["default", "no-finish-grid1", "finish300-grid3"])
def knobs(request, monkeypatch):
    finish, grid = request.param
    for name, v in (("GLRM_HIP_TOPK_FINISH", finish), ("GLRM_HIP_TOPK_GRID", grid)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    return request.param


def list_model(m, n, k, **kw):
    """A list model with max(m, n) observations, one at least in every row and column: the selection never reads the lists."""
    t = np.arange(max(m, n))
    return L.GLRM(np.ones((m, n)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), k, obs=(t % m, t % n), **kw)


class Handle:
    def __init__(self, pa, **opts):
        self.api = hip()
        self.h = self.api.create(pa, **opts)

    def __enter__(self):
        return self.api, self.h

    def __exit__(self, *exc):
        self.api.destroy(self.h)


def check_select(X, Y, ranks, XY=None, **opts):
    """q, n_gt, n_eq of every rank against the sorted restatement; returns the restatement."""
    X, Y = np.asfortranarray(X, dtype=np.float64), np.asfortranarray(Y, dtype=np.float64)
    (k, m), n = X.shape, Y.shape[1]
    ref = R.Sorted(R.xy_chain(X, Y) if XY is None else XY)
    with Handle(list_model(m, n, k).problem_arrays(), **opts) as (api, h):
        api.set_factors(h, X, Y)
        for r in ranks:
            q, gt, eq = api.xy_select(h, None, None, int(r))
            rq, rgt, req = ref.select(int(r))
            print("rank", int(r), "q", q, "n_gt", gt, "n_eq", eq, "passes", api.xy_select_info())
            assert R.same_bits(q, rq) and (gt, eq) == (rgt, req), (int(r), q, rq, gt, rgt, eq, req)
            assert gt < r <= gt + eq
    return ref


def half_ints(rng, shape, r=4):
    return rng.integers(-2 * r, 2 * r + 1, shape) / 2.0     # multiples of 1/2 in [-r, r]


# ================================================================== select

def test_select_generic_doubles(knobs):
    """k = 1, standard normal factors: u is one rounded product.  Every digit of the key and both signs."""
    rng = np.random.default_rng(1)
    m, n = 37, 53
    X, Y = rng.standard_normal((1, m)), rng.standard_normal((1, n))
    ranks = [1, 2, m * n // 2, m * n - 1, m * n] + rng.integers(1, m * n + 1, 20).tolist()
    check_select(X, Y, ranks)


@pytest.mark.parametrize("k", [5, 70])
def test_select_exact_factors_with_ties(k, knobs):
    """k below and above one 16-component trip (70 = 4 trips + 6), 130 x 67 = two row tiles, neither a multiple of the tile.  Factors that
    are multiples of 1/2 in [-4, 4]: every u is a multiple of 1/4 below 2^53, exact in any order (tests/test_gpu_impute.py:67), and there
    are thousands of ties: ranks at the first, an inner and the last position of tie groups pin n_gt and n_eq."""
    rng = np.random.default_rng(2 + k)
    m, n = 130, 67
    X, Y = half_ints(rng, (k, m)), half_ints(rng, (k, n))
    XY = R.xy_chain(X, Y)
    assert np.array_equal(XY, X.T @ Y)
    ref = R.Sorted(XY)
    ranks = [1, m * n]
    for probe in (m * n // 2, m * n // 7, 3 * m * n // 4):
        _, gt, eq = ref.select(probe)
        assert eq >= 3
        ranks += [gt + 1, gt + 1 + eq // 2, gt + eq]
    assert len(np.unique(ref.desc)) < m * n // 4
    check_select(X, Y, ranks, XY=XY)


def test_select_keys_that_differ_only_in_the_low_digits(knobs):
    """x_i = (1, i), y_j = (1, j 2^-52): u = 1 + i j 2^-52 in [1, 2), exact; the leading passes see one bucket."""
    m = n = 64
    X = np.vstack([np.ones(m), np.arange(m, dtype=np.float64)])
    Y = np.vstack([np.ones(n), np.arange(n, dtype=np.float64) * 2.0 ** -52])
    XY = R.xy_chain(X, Y)
    assert XY.min() == 1.0 and XY.max() < 2.0 and np.array_equal(XY, 1.0 + np.outer(X[1], Y[1]))
    rng = np.random.default_rng(3)
    check_select(X, Y, [1, 2, 64, 2048, m * n - 1, m * n] + rng.integers(1, m * n + 1, 10).tolist(), XY=XY)


def test_select_keys_that_differ_only_in_the_high_digits(knobs):
    """k = 1, x_i = +-2^a_i, y_j = 2^b_j, exponents spread over +-300: the mantissa is zero everywhere."""
    rng = np.random.default_rng(4)
    m, n = 40, 33
    X = (np.where(rng.random(m) < 0.5, -1.0, 1.0) * 2.0 ** rng.integers(-300, 301, m))[None, :]
    Y = (2.0 ** rng.integers(-300, 301, n))[None, :]
    assert np.all(np.isfinite(X)) and np.all(X != 0) and np.all(Y > 0)
    check_select(X, Y, [1, 2, m * n // 2, m * n - 1, m * n] + rng.integers(1, m * n + 1, 10).tolist())


def test_select_non_finite_values(knobs):
    """+Inf, -Inf and exactly one NaN (Inf * 0): NaN is greatest, then +Inf; -Inf is last."""
    X = np.array([[1.0, -1.0, np.inf, 2.0, 3.0, 0.5]])
    Y = np.array([[np.inf, 1.0, 0.0, 2.0, -1.0, 4.0]])
    XY = R.xy_chain(X, Y)
    assert np.isnan(XY).sum() == 1 and np.isposinf(XY).sum() >= 2 and np.isneginf(XY).sum() >= 2
    ref = check_select(X, Y, range(1, 37), XY=XY)
    assert np.isnan(ref.select(1)[0]) and ref.select(2)[0] == np.inf and ref.select(36)[0] == -np.inf
    with Handle(list_model(6, 6, 1).problem_arrays()) as (api, h):
        q1, q2, q36 = (api.xy_select(h, X, Y, r) for r in (1, 2, 36))
    assert np.isnan(q1[0]) and q1[1:] == (0, 1) and q2[0] == np.inf and q2[1] == 1 and q36[0] == -np.inf and q36[1] + q36[2] == 36


def test_select_against_the_engines_own_chain(knobs):
    """Random normal factors at k = 7: glrm_hip_impute of a QuadLoss / RealDomain model returns the engine's own u matrix (the chain of
    dots()); the selection must return the entries of that matrix, which pins `the same chain` without numpy needing an fma."""
    rng = np.random.default_rng(5)
    m, n, k = 90, 41, 7
    X, Y = rng.standard_normal((k, m)), rng.standard_normal((k, n))
    g = L.GLRM(np.zeros((m, n)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), k, X=X, Y=Y)
    U = L.impute(g, engine=hip())
    g.close()
    assert U.shape == (m, n) and np.allclose(U, X.T @ Y, rtol=1e-12, atol=1e-12)
    check_select(X, Y, [1, m * n] + rng.integers(1, m * n + 1, 8).tolist(), XY=U)


def test_the_early_finish_and_the_pass_count_are_what_the_knobs_say(monkeypatch):
    rng = np.random.default_rng(6)
    X, Y = rng.standard_normal((1, 200)), rng.standard_normal((1, 150))
    out = {}
    with Handle(list_model(200, 150, 1).problem_arrays()) as (api, h):
        for finish in (None, "0", "300"):
            if finish is None:
                monkeypatch.delenv("GLRM_HIP_TOPK_FINISH", raising=False)
            else:
                monkeypatch.setenv("GLRM_HIP_TOPK_FINISH", finish)
            out[finish] = (api.xy_select(h, X, Y, 12345), api.xy_select_info())
    print(out)
    assert out[None][0] == out["0"][0] == out["300"][0]
    assert out["0"][1] == (8, 0)                                    # all eight digits counted, nothing sorted
    assert out[None][1][0] == 2 and out[None][1][1] > 300           # one counting pass, then the bucket is written out and sorted
    assert 2 < out["300"][1][0] <= 8 and 0 < out["300"][1][1] <= 300


def test_select_argument_forms_and_refusals():
    rng = np.random.default_rng(7)
    api = hip()
    g = L.GLRM(rng.standard_normal((64, 48)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 16)
    X, Y = np.asfortranarray(rng.standard_normal((16, 64))), np.asfortranarray(rng.standard_normal((16, 48)))
    ptr, idx = np.zeros(65, dtype=np.int64), np.zeros(0, dtype=np.int32)

    with Handle(g.problem_arrays()) as (_, h):
        with pytest.raises(_capi.GLRMError) as ei:                   # no factors on the device yet
            api.xy_select(h, None, None, 1)
        assert ei.value.code == _capi.ERR_INVALID
        host = api.xy_select(h, X, Y, 1000)
        api.set_factors(h, X, Y)
        assert api.xy_select(h, None, None, 1000) == host             # the NULL-factor form
        for rank in (0, 64 * 48 + 1, -5):
            with pytest.raises(_capi.GLRMError) as ei:
                api.xy_select(h, X, Y, rank)
            assert ei.value.code == _capi.ERR_INVALID and "BoundsError" in ei.value.message
        with pytest.raises(ValueError):
            api.xy_select(h, X, None, 1)
        q = C.c_double(0.0)                                          # the library itself refuses one NULL factor
        assert api._f["xy_select"](h, X.ctypes.data, None, 1, C.byref(q), None, None) == _capi.ERR_INVALID
        assert api._f["xy_select"](h, None, Y.ctypes.data, 1, C.byref(q), None, None) == _capi.ERR_INVALID
        assert api._f["xy_select"](h, X.ctypes.data, Y.ctypes.data, 1000, C.byref(q), None, None) == 0 and q.value == host[0]   # n_gt, n_eq may be NULL

    def refused(h, code):
        try:
            for call in (lambda: api.xy_select(h, X, Y, 1), lambda: api.precision_scan(h, X, Y, 0.0, ptr, idx, 5)):
                with pytest.raises(_capi.GLRMError) as ei:
                    call()
                assert ei.value.code == code, ei.value
        finally:
            api.destroy(h)

    refused(api.create(g.problem_arrays(dense=True)), _capi.ERR_UNSUPPORTED)
    refused(api.create(g.problem_arrays(), storage=_capi.STORAGE_F32), _capi.ERR_UNSUPPORTED)
    refused(api.create(g.problem_arrays(rows=(0, 32))), _capi.ERR_INVALID)
    refused(api.create(g.problem_arrays(), defer=True), _capi.ERR_INVALID)
    gm = L.GLRM(np.ones((8, 2)), [L.QuadLoss(), L.MultinomialLoss(3)], L.ZeroReg(), L.ZeroReg(), 2)
    with Handle(gm.problem_arrays()) as (_, h):
        with pytest.raises(_capi.GLRMError) as ei:
            api.xy_select(h, np.zeros((2, 8), order="F"), np.zeros((2, 4), order="F"), 1)
        assert ei.value.code == _capi.ERR_UNSUPPORTED and "multi-dimensional loss" in ei.value.message


# ================================================================== scan

class ScanProblem:
    """Raw train and test lists (a model built from a matrix cannot list a column twice): rows with duplicates, empty rows (every ninth
    train row, every seventh test row), and test entries that are also train entries."""

    def __init__(self, m, n, k, seed):
        rng = np.random.default_rng(seed)
        self.m, self.n, self.k = m, n, k
        self.X, self.Y = np.asfortranarray(half_ints(rng, (k, m))), np.asfortranarray(half_ints(rng, (k, n)))
        self.XY = R.xy_chain(self.X, self.Y)
        assert np.array_equal(self.XY, self.X.T @ self.Y)
        self.train = [np.zeros(0, np.int64) if i % 9 == 4 else rng.integers(0, n, rng.integers(1, n // 2)) for i in range(m)]
        self.test = []
        for i in range(m):
            own = np.zeros(0, np.int64) if i % 7 == 3 else rng.integers(0, n, rng.integers(1, 7))
            shared = self.train[i][:2] if i % 3 == 0 else np.zeros(0, np.int64)     # in test AND in train: a true positive
            self.test.append(np.concatenate([own, shared, own[:1]]).astype(np.int64))
        assert any(len(set(r.tolist())) < len(r) for r in self.train) and any(len(set(r.tolist())) < len(r) for r in self.test)
        self.ntrain = sum(len(r) for r in self.train)
        self.test_ptr = np.concatenate([[0], np.cumsum([len(r) for r in self.test])]).astype(np.int64)
        self.test_idx = np.concatenate(self.test).astype(np.int32)

    def arrays(self):
        rowptr = np.concatenate([[0], np.cumsum([len(r) for r in self.train])]).astype(np.int64)
        colidx = np.concatenate(self.train).astype(np.int32)
        I = np.repeat(np.arange(self.m, dtype=np.int64), np.diff(rowptr))
        pc = np.argsort(colidx, kind="stable")
        colptr = np.concatenate([[0], np.cumsum(np.bincount(colidx, minlength=self.n))]).astype(np.int64)
        vals = np.ones(len(colidx))
        return _capi.ProblemArrays(self.m, self.n, self.k, rowptr, np.ascontiguousarray(colidx), vals, colptr,
                                   np.ascontiguousarray(I[pc].astype(np.int32)), np.ones(len(colidx)),
                                   pack_losses([L.QuadLoss()] * self.n), pack_regs([L.ZeroReg()]), pack_regs([L.ZeroReg()]))

    def compare(self, api, h, q, kprec, block_rows):
        ref = R.scan(self.XY, q, self.train, self.test, kprec)
        tp, fp, hits, rows = api.precision_scan(h, None, None, q, self.test_ptr, self.test_idx, kprec, block_rows=block_rows)
        got = (tp, fp, list(zip(hits[0].tolist(), hits[1].tolist(), hits[2].tolist())), rows)
        assert got == ref, (kprec, block_rows, got, ref)
        counts = api.precision_scan(h, None, None, q, self.test_ptr, self.test_idx, kprec, block_rows=block_rows, want_hits=False)
        assert counts == (tp, fp, None, rows)                         # the hit arrays are optional
        return ref


def test_scan_small_every_stop_and_every_block_size():
    p = ScanProblem(45, 30, 3, seed=8)
    with Handle(p.arrays()) as (api, h):
        q, gt, eq = api.xy_select(h, p.X, p.Y, p.ntrain)              # q from the select, as the driver takes it
        assert (q, gt, eq) == R.Sorted(p.XY).select(p.ntrain)
        everything = R.scan(p.XY, q, p.train, p.test, 10 ** 9)
        hits = everything[2]
        assert everything[0] > 3 and everything[1] > 3 and everything[3] == 45
        ignored = sum(1 for i in range(45) for j in range(30) if p.XY[i, j] >= q and j in set(p.train[i].tolist()) and j not in set(p.test[i].tolist()))
        assert ignored > 3                                            # flagged, in train only: skipped without counting
        at_block_end = next(t + 1 for t, (i, _, _) in enumerate(hits) if i % 7 == 6 and (t + 1 == len(hits) or hits[t + 1][0] != i))
        mid_row = next(t + 1 for t, (i, _, _) in enumerate(hits) if t + 1 < len(hits) and hits[t + 1][0] == i)
        for kprec in (0, -3, 1, 10, mid_row, at_block_end, len(hits), len(hits) + 5):
            for block_rows in (0, 1, 7, 45, 1000):
                ref = p.compare(api, h, q, kprec, block_rows)
                if kprec == at_block_end:
                    assert ref[3] % 7 == 0                            # the stop is exactly at the last row of a 7-row block
                if kprec > len(hits):
                    assert ref[3] == 45                               # never stops
        for block_rows in (0, 7):
            assert api.precision_scan(h, None, None, np.nan, p.test_ptr, p.test_idx, 10, block_rows=block_rows)[:2] == (0, 0)
            p.compare(api, h, -np.inf, 10 ** 6, block_rows)           # every entry is flagged: the whole classification
            p.compare(api, h, np.inf, 10, block_rows)                 # nothing is


def test_scan_across_tiles_and_wave_chunks():
    """150 x 200: two row tiles and two column tiles of the flag kernel, four 64-column chunks per row of the classifying wave."""
    p = ScanProblem(150, 200, 5, seed=9)
    with Handle(p.arrays()) as (api, h):
        q = api.xy_select(h, p.X, p.Y, p.ntrain)[0]
        nhits = len(R.scan(p.XY, q, p.train, p.test, 10 ** 9)[2])
        assert nhits > 200
        for kprec in (25, nhits - 1, nhits + 1):
            for block_rows in (0, 64, 129):
                p.compare(api, h, q, kprec, block_rows)


def test_scan_refuses_malformed_test_lists():
    p = ScanProblem(45, 30, 3, seed=8)
    with Handle(p.arrays()) as (api, h):
        api.set_factors(h, p.X, p.Y)
        bad_ptr = p.test_ptr.copy()
        bad_ptr[5] = bad_ptr[6] + 1
        bad_idx = p.test_idx.copy()
        bad_idx[3] = 30
        for ptr, idx in ((bad_ptr, p.test_idx), (p.test_ptr, bad_idx), (p.test_ptr + 1, p.test_idx)):
            with pytest.raises(_capi.GLRMError) as ei:
                api.precision_scan(h, None, None, 0.0, ptr, idx, 5)
            assert ei.value.code == _capi.ERR_INVALID


# ================================================================== the driver

def censored_example(m, n, seed):
    """examples/precision_at_k.jl:6-19, shrunk: Bernoulli samples of a rank-one matrix, only the ones observed; 20 % held out."""
    rng = np.random.default_rng(seed)
    A = rng.random((m, 1)) @ rng.random((1, n))
    B = (rng.random((m, n)) >= A).astype(np.int64)
    train_of, train_oe, test_of = [[] for _ in range(m)], [[] for _ in range(n)], [[] for _ in range(m)]
    for i in range(m):
        for j in range(n):
            if B[i, j] == 1:
                if rng.random() < 0.2:
                    test_of[i].append(j)
                else:
                    train_of[i].append(j)
                    train_oe[j].append(i)

    def model():
        return L.GLRM(B, [L.QuadLoss() for _ in range(n)], L.QuadReg(.1), L.QuadReg(.1), 1, observed_features=train_of,
                      observed_examples=train_oe, rng=np.random.default_rng(seed + 1))
    return model, test_of


def test_precision_at_k_equals_the_restatement():
    m = n = 40
    model, test_of = censored_example(m, n, seed=10)
    params = L.Params(1, max_iter=20, abs_tol=1e-5, min_stepsize=0.01)
    reg_params = [10.0, 0.1, 1e-3]
    g = model()
    got = L.precision_at_k(g, test_of, params=params, reg_params=reg_params, verbose=False, kprec=10, rng=np.random.default_rng(77), engine=hip())
    assert [r.scale for r in list(g.rx)[:2] + list(g.ry)[:2]] == [1e-3] * 4      # set to reg_param, not multiplied
    g.close()
    g = model()
    ref = R.precision_at_k(g, test_of, params, reg_params, 10, np.random.default_rng(77), hip())
    g.close()
    names = ("train_error", "test_error", "prec_at_k", "train_time", "reg_params", "solution")
    for name, a, b in zip(names, got, ref):
        print(name, np.asarray(a).tolist(), np.asarray(b).tolist())
    for name, a, b in zip(names, got, ref):
        if name == "train_time":
            assert a.shape == b.shape == (3,) and np.all(np.isfinite(a)) and np.all(np.diff(a) >= 0) and a[0] > 0
        else:
            assert R.same_bits(a, b), name                           # NaN positions included
    assert np.all((got[2] >= 0) & (got[2] <= 1) | np.isnan(got[2]))


# ================================================================== determinism

def test_two_calls_and_handles_of_different_families_agree():
    p = ScanProblem(150, 200, 5, seed=11)
    outs = []
    for opts in ({}, {}, {"tiled": 1}, {"tiled": 2}):
        with Handle(p.arrays(), **opts) as (api, h):
            sel = [api.xy_select(h, p.X, p.Y, r) for r in (1, p.ntrain, 150 * 200)]
            sel2 = [api.xy_select(h, p.X, p.Y, r) for r in (1, p.ntrain, 150 * 200)]
            assert all(R.same_bits(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(sel, sel2))
            tp, fp, hits, rows = api.precision_scan(h, None, None, sel[1][0], p.test_ptr, p.test_idx, 40)
            outs.append(([(np.float64(q).view(np.uint64), gt, eq) for q, gt, eq in sel], tp, fp, [x.tolist() for x in hits], rows))
    assert all(o == outs[0] for o in outs[1:])
