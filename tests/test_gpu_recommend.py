"""-m gpu: glrm_hip_row_topk (include/glrm_hip_recommend.h; csrc/glrm_recommend.hip) and L.recommend against the numpy restatement
(tests/recommend_ref.py).  Every comparison is exact -- columns and counts as integers, values by their bits -- because every input is
one of the devices of tests/test_gpu_topk.py: k = 1 (u is one rounded product), factors that are multiples of 1/2 in [-4, 4] (every
product and sum exact), or the engine's own u read back through L.impute.

Every case runs with col_splits in SPLITS (the engine's choice, one span, three spans, more spans than there are tiles) and every one
must return the same arrays: the order is strict, so the answer cannot depend on how the columns are cut."""
import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import precision_ref as R
import recommend_ref as RR
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.losses import pack_losses
from lowrankmodels.jl_amd.regularizers import pack_regs
from test_gpu_leaks import free_bytes
from test_gpu_topk import Handle, half_ints, hip, list_model

pytestmark = pytest.mark.gpu

SPLITS = [0, 1, 3, 1000]
TILE = 128


def list_arrays(m, n, k, lists):
    """ProblemArrays from raw row lists (a model built from a matrix cannot list a column twice), like ScanProblem.arrays."""
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    colidx = (np.concatenate([np.asarray(r, dtype=np.int64) for r in lists]) if rowptr[-1] else np.zeros(0)).astype(np.int32)
    I = np.repeat(np.arange(m, dtype=np.int64), np.diff(rowptr))
    pc = np.argsort(colidx, kind="stable")
    colptr = np.concatenate([[0], np.cumsum(np.bincount(colidx, minlength=n))]).astype(np.int64)
    return _capi.ProblemArrays(m, n, k, rowptr, np.ascontiguousarray(colidx), np.ones(len(colidx)), colptr,
                               np.ascontiguousarray(I[pc].astype(np.int32)), np.ones(len(colidx)),
                               pack_losses([L.QuadLoss()] * n), pack_regs([L.ZeroReg()]), pack_regs([L.ZeroReg()]))


def random_lists(rng, m, n, most=40):
    """0 .. most columns per row, drawn with replacement (duplicates), in no order; the first row's list is empty."""
    lists = [rng.integers(0, n, rng.integers(0, most + 1)) for _ in range(m)]
    lists[0] = np.zeros(0, dtype=np.int64)
    lists[1] = np.concatenate([lists[1], lists[1][:3], [n - 1, n - 1]])
    assert any(len(set(r.tolist())) < len(r) for r in lists)
    return lists


def check(api, h, X, Y, XY, kpers, lists=None, rows=None, excludes=(0, 1)):
    """Every kper x exclude x col_splits against the restatement; with ``lists`` None the handle's lists are not compared (exclude = 0)."""
    X, Y = np.asfortranarray(X, dtype=np.float64), np.asfortranarray(Y, dtype=np.float64)
    tiles = -(-XY.shape[1] // TILE)
    for kper in kpers:
        for exclude in excludes if lists is not None else (0,):
            ref = RR.row_topk(XY, rows, kper, lists if exclude else None)
            for s in SPLITS:
                got = api.row_topk(h, X, Y, rows, kper, exclude=exclude, col_splits=s)
                info = api.row_topk_info()
                bad = np.flatnonzero((got[0] != ref[0]).any(axis=1) | (got[2] != ref[2]))
                print("kper", kper, "exclude", exclude, "col_splits", s, info, "rows that differ", bad[:5].tolist())
                assert RR.same(got, ref), (kper, exclude, s, bad[:5].tolist(), got[0][bad[:2]].tolist(), ref[0][bad[:2]].tolist())
                if s:
                    assert info["col_splits"] == min(s, tiles)
                assert info["row_blocks"] == 1 and 0 <= info["candidates_merged"] <= info["col_splits"] * kper * len(ref[2])


def test_generic_doubles():
    """k = 1, standard normal factors.  130 rows = two bands, the second of 2 rows; 300 columns = three tiles, the last of 44."""
    rng = np.random.default_rng(21)
    m, n = 130, 300
    X, Y = rng.standard_normal((1, m)), rng.standard_normal((1, n))
    lists = random_lists(rng, m, n)
    with Handle(list_arrays(m, n, 1, lists)) as (api, h):
        check(api, h, X, Y, R.xy_chain(X, Y), (1, 10, 128), lists)


@pytest.mark.parametrize("k", [5, 70])
def test_exact_factors_with_ties(k):
    """k below and above one 16-component staging trip, factors that are multiples of 1/2 (in [-1, 1]: at k = 70 a wider range spreads
    the 47 candidates of a row over too many values to tie): every u is exact in any order and there are thousands of ties, so the column
    rule decides who is kept: some row has at least 3 candidates equal to its kper-th, not all of them kept."""
    rng = np.random.default_rng(22 + k)
    m, n, kper = 130, 67, 10
    X, Y = half_ints(rng, (k, m), r=1), half_ints(rng, (k, n), r=1)
    XY = R.xy_chain(X, Y)
    assert np.array_equal(XY, X.T @ Y)
    mask = rng.random((m, n)) < 0.3
    lists = [np.flatnonzero(mask[i]) for i in range(m)]
    cols, vals, count = RR.row_topk(XY, None, kper, lists)
    decided = 0
    for i in range(m):
        cand = XY[i, ~mask[i]]
        tied = int((cand == vals[i, kper - 1]).sum())
        kept = int((vals[i] == vals[i, kper - 1]).sum())
        decided += tied >= 3 and kept < tied
    assert decided >= 1
    with Handle(list_arrays(m, n, k, lists)) as (api, h):
        check(api, h, X, Y, XY, (kper, 128), lists)


def test_generic_doubles_against_the_engines_own_chain():
    """Random normal factors at k = 7: L.impute of a QuadLoss / RealDomain model returns the engine's own u matrix."""
    rng = np.random.default_rng(23)
    m, n, k = 40, 150, 7
    X, Y = rng.standard_normal((k, m)), rng.standard_normal((k, n))
    g = L.GLRM(np.zeros((m, n)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), k, X=X, Y=Y)
    U = L.impute(g, engine=hip())
    g.close()
    assert U.shape == (m, n) and np.allclose(U, X.T @ Y, rtol=1e-12, atol=1e-12)
    lists = random_lists(rng, m, n)
    with Handle(list_arrays(m, n, k, lists)) as (api, h):
        check(api, h, X, Y, U, (10,), lists)


@pytest.mark.parametrize("order", ["ascending", "descending", "equal"])
def test_adversarial_orders(order):
    """k = 1, x = 1.  y_j = j: scores ascending in j, every entry of every tile passes the threshold, the staging area overflows and a
    tile drains in rounds.  y_j = -j: nothing passes after the first tile.  y = 1: all scores equal, the answer is the kper lowest
    columns that are not left out.  129 rows (a second band of one row), 700 columns (six tiles, the last of 60)."""
    rng = np.random.default_rng(24)
    m, n = 129, 700
    j = np.arange(n, dtype=np.float64)
    X, Y = np.ones((1, m)), {"ascending": j, "descending": -j, "equal": np.ones(n)}[order][None, :]
    lists = random_lists(rng, m, n)
    lists[2] = np.arange(5)                                          # the five lowest columns: the `equal` answer starts at column 5
    lists[3] = np.arange(n - 5, n)                                   # the five highest
    XY = R.xy_chain(X, Y)
    with Handle(list_arrays(m, n, 1, lists)) as (api, h):
        check(api, h, X, Y, XY, (10, 128), lists)
        if order == "equal":
            cols = api.row_topk(h, X, Y, [2, 0], 10)[0]
            assert cols.tolist() == [list(range(5, 15)), list(range(10))]


def test_short_and_empty_rows():
    rng = np.random.default_rng(25)
    m, n, kper = 6, 200, 10
    X, Y = rng.standard_normal((1, m)), rng.standard_normal((1, n))
    lists = [rng.permutation(n),                                     # every column: count 0, all padding
             rng.permutation(n)[3:],                                 # all but 3: count 3 < kper
             np.zeros(0, dtype=np.int64),                            # empty
             np.full(50, 17),                                        # one column, repeated
             np.concatenate([np.arange(n), np.arange(n)]),           # every column twice
             rng.integers(0, n, 30)]
    XY = R.xy_chain(X, Y)
    ref = RR.row_topk(XY, None, kper, lists)
    assert ref[2].tolist() == [0, 3, 10, 10, 0, 10] and (ref[0][0] == -1).all() and (ref[0][1, 3:] == -1).all() and 17 not in ref[0][3]
    assert (ref[1].view(np.uint64)[0] == 0x7FF8000000000000).all()
    with Handle(list_arrays(m, n, 1, lists)) as (api, h):
        check(api, h, X, Y, XY, (kper, 128), lists)


def test_non_finite_values_and_signed_zeros():
    """The 6 x 6 example of test_select_non_finite_values: NaN ranks first, then +Inf; -Inf is last.  And a row whose products underflow
    to +0.0 and -0.0 (the restatement's matrix is written out: numpy's unfused x y + 0.0 loses the sign the fma keeps)."""
    X = np.array([[1.0, -1.0, np.inf, 2.0, 3.0, 0.5]])
    Y = np.array([[np.inf, 1.0, 0.0, 2.0, -1.0, 4.0]])
    XY = R.xy_chain(X, Y)
    assert np.isnan(XY).sum() == 1 and np.isnan(XY[2, 2])
    with Handle(list_model(6, 6, 1).problem_arrays()) as (api, h):
        check(api, h, X, Y, XY, (1, 6, 7))
        cols, vals, count = api.row_topk(h, X, Y, None, 6, exclude=False)
    assert cols[2, 0] == 2 and vals.view(np.uint64)[2, 0] == 0x7FF8000000000000            # the NaN first, as THE quiet NaN
    assert vals[2, 1] == np.inf and vals[2, 5] == -np.inf and vals[0, 0] == np.inf and vals[1, 5] == -np.inf and count.tolist() == [6] * 6
    x, y = np.array([[1e-200, -1e-200]]), np.array([[1e-200, -1e-200, 0.0, 1.0, -1.0]])
    Z = np.array([[0.0, -0.0, 0.0, 1e-200, -1e-200], [-0.0, 0.0, 0.0, -1e-200, 1e-200]])  # fma(x, y, +0.0): -0.0 only by underflow
    ref = RR.row_topk(Z, None, 5)
    assert ref[0].tolist() == [[3, 0, 2, 1, 4], [4, 1, 2, 0, 3]]                           # +0.0 above -0.0, equal zeros by column
    with Handle(list_model(2, 5, 1).problem_arrays()) as (api, h):
        check(api, h, x, y, Z, (5, 2))


def test_query_lists():
    rng = np.random.default_rng(26)
    m, n, kper = 140, 131, 10
    X, Y = np.asfortranarray(rng.standard_normal((1, m))), np.asfortranarray(rng.standard_normal((1, n)))
    lists = random_lists(rng, m, n)
    XY = R.xy_chain(X, Y)
    with Handle(list_arrays(m, n, 1, lists)) as (api, h):
        everything = api.row_topk(h, X, Y, None, kper)
        assert RR.same(everything, api.row_topk(h, X, Y, np.arange(m), kper))            # in place against gathered
        assert RR.same(everything, RR.row_topk(XY, None, kper, lists))
        api.set_factors(h, X, Y)
        assert RR.same(everything, api.row_topk(h, None, None, np.arange(m), kper))      # the NULL-factor form
        queries = np.concatenate([rng.permutation(m), [139, 0, 139, 7, 7]])               # unordered, with repeats, 145 > one band
        check(api, h, X, Y, XY, (kper,), lists, rows=queries)
        check(api, h, X, Y, XY, (kper,), lists, rows=[77])                               # a single row
        cols, vals, count = api.row_topk(h, X, Y, np.zeros(0, dtype=np.int64), kper)     # n_rows = 0
        assert cols.shape == vals.shape == (0, kper) and count.shape == (0,)
        with pytest.raises(ValueError):
            api.row_topk(h, None, None, None, kper)                                      # rows=None needs X for m


def test_refusals():
    rng = np.random.default_rng(27)
    api = hip()
    g = L.GLRM(rng.standard_normal((64, 48)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 16)                  # (k = 16: eligible for the dense hand-over)
    X, Y = np.asfortranarray(rng.standard_normal((16, 64))), np.asfortranarray(rng.standard_normal((16, 48)))

    def refused(call, code, word):
        with pytest.raises(_capi.GLRMError) as ei:
            call()
        assert ei.value.code == code and word in ei.value.message, ei.value

    with Handle(g.problem_arrays()) as (_, h):
        refused(lambda: api.row_topk(h, None, None, [0], 5), _capi.ERR_INVALID, "no factors")
        good = api.row_topk(h, X, Y, [3, 5], 5)
        refused(lambda: api.row_topk(h, X, Y, [3, -1], 5), _capi.ERR_INVALID, "rows[1] = -1")
        refused(lambda: api.row_topk(h, X, Y, [64], 5), _capi.ERR_INVALID, "rows[0] = 64")
        refused(lambda: api.row_topk(h, X, Y, [0], 0), _capi.ERR_INVALID, "kper")
        refused(lambda: api.row_topk(h, X, Y, [0], 129), _capi.ERR_UNSUPPORTED, "GLRM_ROW_TOPK_MAX = 128")
        refused(lambda: api.row_topk(h, X, Y, [0], 5, exclude=2), _capi.ERR_INVALID, "exclude")
        refused(lambda: api.row_topk(h, X, Y, [0], 5, col_splits=-1), _capi.ERR_INVALID, "col_splits")
        fn = api._f["row_topk"]
        rows, cols, vals = np.array([3, 5], dtype=np.int64), np.full((2, 5), -7, dtype=np.int32), np.full((2, 5), -7.0)
        assert fn(h, X.ctypes.data, Y.ctypes.data, rows.ctypes.data, 2, 5, 1, 0, None, vals.ctypes.data, None) == _capi.ERR_INVALID
        assert "out_cols" in api.last_error()
        assert fn(h, X.ctypes.data, None, rows.ctypes.data, 2, 5, 1, 0, cols.ctypes.data, vals.ctypes.data, None) == _capi.ERR_INVALID
        assert fn(h, X.ctypes.data, Y.ctypes.data, rows.ctypes.data, -1, 5, 1, 0, cols.ctypes.data, vals.ctypes.data, None) == _capi.ERR_INVALID
        assert "n_rows" in api.last_error()
        assert fn(h, X.ctypes.data, Y.ctypes.data, None, 2, 5, 1, 0, cols.ctypes.data, vals.ctypes.data, None) == _capi.ERR_INVALID   # rows NULL: n_rows must be m
        assert (cols == -7).all() and (vals == -7.0).all()                                # a refusal touches nothing
        assert fn(h, X.ctypes.data, Y.ctypes.data, rows.ctypes.data, 2, 5, 1, 0, cols.ctypes.data, vals.ctypes.data, None) == 0       # out_count may be NULL
        assert np.array_equal(cols, good[0]) and R.same_bits(vals, good[1])

    def handle_refused(h, code, word=""):
        try:
            refused(lambda: api.row_topk(h, X, Y, [0], 5), code, word)
        finally:
            api.destroy(h)

    handle_refused(api.create(g.problem_arrays(dense=True)), _capi.ERR_UNSUPPORTED, "dense_A")
    handle_refused(api.create(g.problem_arrays(), storage=_capi.STORAGE_F32), _capi.ERR_UNSUPPORTED)
    handle_refused(api.create(g.problem_arrays(rows=(0, 32))), _capi.ERR_INVALID, "single-shard")
    handle_refused(api.create(g.problem_arrays(), defer=True), _capi.ERR_INVALID)
    g.close()
    gm = L.GLRM(np.ones((8, 2)), [L.QuadLoss(), L.MultinomialLoss(3)], L.ZeroReg(), L.ZeroReg(), 2)
    with Handle(gm.problem_arrays()) as (_, h):
        refused(lambda: api.row_topk(h, np.zeros((2, 8), order="F"), np.zeros((2, 4), order="F"), [0], 1), _capi.ERR_UNSUPPORTED, "multi-dimensional loss")
    gm.close()


def test_the_driver():
    rng = np.random.default_rng(28)
    m, n, k = 60, 40, 3
    A = rng.standard_normal((m, k)) @ rng.standard_normal((k, n))
    I, J = np.nonzero(rng.random((m, n)) < 0.4)
    g = L.GLRM(A, L.QuadLoss(), L.QuadReg(.1), L.QuadReg(.1), k, obs=(I, J), rng=np.random.default_rng(29))
    L.fit_b(g, L.Params(1, max_iter=10, abs_tol=1e-5, min_stepsize=0.01), verbose=False, engine=hip())
    U = L.impute(g, engine=hip())
    seen = [np.asarray(r, dtype=np.int64) for r in g.observed_features]
    assert sum(len(r) for r in seen) == len(I)
    cols, scores = L.recommend(g, k=5)
    ref = RR.row_topk(U, None, 5, seen)
    assert np.array_equal(cols, ref[0]) and cols.dtype == np.int32 and R.same_bits(scores, ref[1])
    for i in range(m):
        assert not set(cols[i].tolist()) & set(seen[i].tolist())                          # nothing a row has observed comes back
    cols_all, scores_all = L.recommend(g, k=5, exclude_observed=False)
    ref_all = RR.row_topk(U, None, 5)
    assert np.array_equal(cols_all, ref_all[0]) and R.same_bits(scores_all, ref_all[1]) and not np.array_equal(cols_all, cols)
    some = [59, 0, 0, 31]
    c2, s2 = L.recommend(g, some, 5, X=g.X.copy(), Y=g.Y.copy())                           # passed factors against the model's own
    assert np.array_equal(c2, cols[some]) and R.same_bits(s2, scores[some])
    c3, s3 = L.recommend(g, k=45)                                                         # more than there are columns: padding
    assert c3.shape == (m, 45) and (c3[:, 40:] == -1).all() and np.isnan(s3[:, 40:]).all()
    assert all((c3[i] >= 0).sum() == n - len(set(seen[i].tolist())) for i in range(m))
    with pytest.raises(_capi.GLRMError) as ei:
        L.recommend(g, [m], 5)
    assert ei.value.code == _capi.ERR_INVALID
    g.close()


def test_no_device_memory_leak():
    """20 calls leave device memory where it was.  A call's scratch is well above 1 MiB here (2000 queries x 128 kept x 12 B x 2), so a
    call that kept it would lose tens of MiB; a one-off step of the runtime's own pools is not a leak (tests/test_gpu_leaks.py), so the
    better of two windows of 10 calls is held to 4 MiB."""
    rng = np.random.default_rng(30)
    m, n = 2000, 300
    X, Y = np.asfortranarray(rng.standard_normal((1, m))), np.asfortranarray(rng.standard_normal((1, n)))
    with Handle(list_arrays(m, n, 1, random_lists(rng, m, n))) as (api, h):
        rows = rng.permutation(m)
        first = api.row_topk(h, X, Y, rows, 128)
        api.row_topk(h, X, Y, rows, 128)
        levels = [free_bytes()]
        for _ in range(2):
            for _ in range(10):
                out = api.row_topk(h, X, Y, rows, 128)
            levels.append(free_bytes())
        assert RR.same(out, first)
        lost = [levels[i] - levels[i + 1] for i in range(2)]
        assert min(lost) < 4 << 20, f"device memory lost per window of 10 calls (MiB): {[round(x / 2**20, 1) for x in lost]}"
