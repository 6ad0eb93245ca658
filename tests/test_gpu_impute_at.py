"""-m gpu: glrm_hip_impute_at (include/glrm_hip_impute_at.h; csrc/glrm_impute_at.hip) and L.impute_at / L.error_metric_at.

Every comparison is bit for bit (NaNs by their bits).  The reference is glrm_hip_impute's full matrix on the same handle and the same
factors; behind it stands the Python mirror (L.impute_entry / L.error_metric_entry) on inputs whose dot products are exact (multiples
of 1/2, tests/test_gpu_impute.py).  Every case runs with block_entries in BLOCKS (the engine's choice, one entry per block, a quarter of
a workgroup, more than there are entries) and every one must return the same arrays."""
import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import precision_ref as R
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.domains import pack_domains
from test_gpu_impute import EXACT, UNSUPPORTED_PAIRS, factors, table_model, trans_model
from test_gpu_leaks import free_bytes
from test_gpu_topk import Handle, hip

pytestmark = pytest.mark.gpu

BLOCKS = [0, 1, 64, 1000]
M, N = 130, 70
KS = [5, 20, 32, 64]          # kp 8 / 32 / 32 / 64: two padded layouts, two unpadded
PS = [0, 1, 63, 64, 65, 257, 1000]
# the nine scalar loss kinds of tests/test_gpu_storage_f32_cached.py::kinds_problem (which draws rows of up to 104 observations and so
# cannot be built with 70 columns), cycling over the columns
NINE = [L.QuadLoss(0.8), L.L1Loss(0.6), L.HuberLoss(1.1, crossover=0.7), L.QuantileLoss(0.9, quantile=0.3), L.PeriodicLoss(2.5, 0.8),
        L.PoissonLoss(20), L.OrdinalHingeLoss(1, 5, 0.9), L.LogisticLoss(0.7), L.WeightedHingeLoss(1.2, case_weight_ratio=2.0)]


def scalar_model(model, k):
    """(problem arrays, X, Y, packed domains) of the m = 130, n = 70 models: QuadLoss / RealDomain, or the nine kinds with their default domains."""
    rng = np.random.default_rng(1000 + k)
    losses = [L.QuadLoss()] * N if model == "quad" else [NINE[f % len(NINE)] for f in range(N)]
    X, Y = np.asfortranarray(rng.standard_normal((k, M))), np.asfortranarray(rng.standard_normal((k, N)))
    g = L.GLRM(np.ones((M, N)), losses if model != "quad" else L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), k, X=X, Y=Y)
    pa = g.problem_arrays()
    g.close()
    return pa, X, Y, pack_domains([L.default_domain(l) for l in losses])


def draw_pairs(rng, P, m, n):
    """P pairs with repeats, in no order; the four corners are among them for P >= 4."""
    rows, cols = rng.integers(0, m, P), rng.integers(0, n, P)
    if P >= 4:
        at = rng.choice(P, 4, replace=False)
        rows[at], cols[at] = [0, m - 1, 0, m - 1], [0, n - 1, n - 1, 0]
    if P >= 64:
        rows[7], cols[7] = rows[3], cols[3]                           # a repeat for certain
    return rows.astype(np.int64), cols.astype(np.int32)


def mirror(pairs, losses, U, rows, cols):
    """L.impute_entry at the pairs; U = the exact X'Y over the d vectors of Y."""
    spans = L.get_yidxs(losses)
    out = np.empty(len(rows))
    for t, (i, j) in enumerate(zip(rows, cols)):
        y0, y1 = spans[j]
        out[t] = float(L.impute_entry(pairs[j][0], losses[j], U[i, y0:y1] if losses[j].embedding_dim > 1 else float(U[i, y0])))
    return out


# ================================================================== 1. pairs, scalar models

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("model", ["quad", "nine-kinds"])
def test_pairs_scalar_models(model, k):
    pa, X, Y, doms = scalar_model(model, k)
    rng = np.random.default_rng(k)
    with Handle(pa) as (api, h):
        assert api.factor_ld(h) == {5: 8, 20: 32, 32: 32, 64: 64}[k]
        Ahat = api.impute(h, X, Y, doms, M, N)
        for P in PS:
            rows, cols = draw_pairs(rng, P, M, N)
            want = Ahat[rows, cols]
            for b in BLOCKS:
                got = api.impute_at(h, X, Y, doms, M, N, rows, cols, block_entries=b)
                info = api.impute_at_info()
                bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
                print(model, "k", k, "P", P, "block_entries", b, info, "entries that differ", bad[:5].tolist())
                assert R.same_bits(got, want), (P, b, bad[:5].tolist(), got[bad[:3]], want[bad[:3]])
                assert info["entries_fast"] == P and info["entries_general"] == 0
                assert info["blocks"] == (0 if P == 0 else -(-P // b) if b else 1)


# ================================================================== 2. pairs, the rule table

def every_entry_shuffled(rng, m, n):
    t = rng.permutation(m * n)
    return (t % m).astype(np.int64), (t // m).astype(np.int32)


@pytest.mark.parametrize("m,k", [(129, 5), (130, 33)])
def test_rule_table_every_entry_in_a_shuffled_order(m, k):
    """The (domain, loss) pairs of tests/test_gpu_impute.py whose rules are comparisons, rounding and IEEE division, scalar columns and
    columns of embedding dimension 2 .. 32 side by side: every entry once, shuffled, against the full matrix AND against the mirror."""
    g, X, Y, doms = table_model(EXACT, m, k, seed=100 + m)
    pa, n, losses = g.problem_arrays(), len(EXACT), list(g.losses)
    g.close()
    rows, cols = every_entry_shuffled(np.random.default_rng(m), m, n)
    U = R.xy_chain(X, Y)
    assert np.array_equal(U, X.T @ Y)                                 # exact in any order
    want_mirror = mirror(EXACT, losses, U, rows, cols)
    n_general = int(sum(l.embedding_dim > 1 for l in losses)) * m
    assert 0 < n_general < m * n
    with Handle(pa) as (api, h):
        Ahat = api.impute(h, X, Y, doms, m, n)
        for b in [0, 1000, 4097]:
            got = api.impute_at(h, X, Y, doms, m, n, rows, cols, block_entries=b)
            info = api.impute_at_info()
            print("m", m, "k", k, "block_entries", b, info)
            bad = np.flatnonzero(got.view(np.uint64) != Ahat[rows, cols].view(np.uint64))
            assert bad.size == 0, [(EXACT[cols[t]], int(rows[t]), got[t], Ahat[rows[t], cols[t]]) for t in bad[:5]]
            assert info["entries_general"] == n_general and info["entries_fast"] == m * n - n_general      # both paths in one call
        # The mirror rounds with Python's round(), which returns an int: where the engine's rint gives -0.0 (u = -1/4, -1/2) the mirror
        # has +0.0 and no way to say otherwise.  Both sides therefore have +0.0 added (-0.0 + 0.0 = +0.0, every other value and every
        # NaN keeps its bits); the sign of such a zero IS held above, against the full matrix.
        a, b = got + 0.0, want_mirror + 0.0
        assert np.signbit(got[got == 0]).any() and not np.signbit(want_mirror[want_mirror == 0]).any()
        bad = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))
        assert bad.size == 0, [(EXACT[cols[t]], int(rows[t]), got[t], want_mirror[t]) for t in bad[:5]]


def test_rule_table_with_transcendentals_equals_the_full_matrix():
    """The rules that decide through exp / log / cos: the same device function on the same u, so the same bits as the full matrix."""
    g, X, Y, doms = trans_model()
    pa, (m, n) = g.problem_arrays(), (g.m, g.n)
    g.close()
    rows, cols = every_entry_shuffled(np.random.default_rng(3), m, n)
    with Handle(pa) as (api, h):
        Ahat = api.impute(h, X, Y, doms, m, n)
        for b in [0, 777]:
            got = api.impute_at(h, X, Y, doms, m, n, rows, cols, block_entries=b)
            info = api.impute_at_info()
            assert R.same_bits(got, Ahat[rows, cols]), b
            assert info["entries_general"] > 0 and info["entries_fast"] > 0


# ================================================================== 3. slabs

SLAB_ROWS, SLAB_COLS = [0, 129, 64, 64], [69, 0, 5]


def check_slabs(api, h, X, Y, doms, m, n, cols):
    Ahat = api.impute(h, X, Y, doms, m, n)
    for b in BLOCKS + [37]:                                           # 37: a block ends inside a slab's row of 4 / column of 130
        got = api.impute_at(h, X, Y, doms, m, n, rows=SLAB_ROWS, block_entries=b)
        assert got.shape == (4, n) and got.flags.f_contiguous and R.same_bits(got, Ahat[SLAB_ROWS, :]), ("rows", b)
        assert api.impute_at_info()["blocks"] == (-(-4 * n // b) if b else 1)
        got = api.impute_at(h, X, Y, doms, m, n, cols=cols, block_entries=b)
        assert got.shape == (m, len(cols)) and got.flags.f_contiguous and R.same_bits(got, Ahat[:, cols]), ("cols", b)
        assert api.impute_at_info()["blocks"] == (-(-m * len(cols) // b) if b else 1)


@pytest.mark.parametrize("model,k", [("quad", 5), ("quad", 64), ("nine-kinds", 20), ("nine-kinds", 32)])
def test_slabs_scalar_models(model, k):
    pa, X, Y, doms = scalar_model(model, k)
    with Handle(pa) as (api, h):
        check_slabs(api, h, X, Y, doms, M, N, SLAB_COLS)
        assert api.impute_at_info()["entries_general"] == 0
        empty = api.impute_at(h, X, Y, doms, M, N, rows=[])
        assert empty.shape == (0, N)


def test_slabs_rule_table():
    g, X, Y, doms = table_model(EXACT, M, 5, seed=230)
    pa, n = g.problem_arrays(), len(EXACT)
    g.close()
    with Handle(pa) as (api, h):
        check_slabs(api, h, X, Y, doms, M, n, [n - 1, 0, 5])
        api.impute_at(h, X, Y, doms, M, n, rows=SLAB_ROWS)
        info = api.impute_at_info()
        assert info["entries_general"] > 0 and info["entries_fast"] > 0


# ================================================================== 4. errors

def sum_like_the_device(v):
    """glrm_hip_sum's fixed order on a vector: thread s of 65536 adds the elements s, s + 65536, .. ascending, then two tree sums."""
    v = np.asarray(v, dtype=np.float64)
    pad = np.zeros(-(-max(len(v), 1) // 65536) * 65536)
    pad[:len(v)] = v
    acc = np.zeros(65536)
    for row in pad.reshape(-1, 65536):
        acc = acc + row
    for _ in range(2):                                                # 256 blocks of 256, then the 256 partials
        acc = acc.reshape(-1, 256).copy()
        s = 128
        while s:
            acc[:, :s] += acc[:, s:2 * s]
            s //= 2
        acc = acc[:, 0]
    return float(acc[0])


def test_errors_on_integer_data_are_exact():
    """Integer A, X and Y (k = 2), QuadLoss / RealDomain; column lengths around the 256-entry workgroup (255, 256, 257), a long column, a
    single entry and none.  Pairs = the model's own observations in column-view order, truth = their values: every term is an integer."""
    m, k, lens = 4096, 2, [255, 256, 257, 1000, 1, 0]
    rng = np.random.default_rng(4096)
    A = rng.integers(-9, 10, (m, len(lens))).astype(np.float64)
    X, Y = np.asfortranarray(rng.integers(-3, 4, (k, m)).astype(np.float64)), np.asfortranarray(rng.integers(-3, 4, (k, len(lens))).astype(np.float64))
    I = np.concatenate([np.sort(rng.choice(m, n_f, replace=False)) for n_f in lens])
    J = np.repeat(np.arange(len(lens)), lens)
    g = L.GLRM(A, L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), k, obs=(I, J), X=X, Y=Y)
    pa = g.problem_arrays()
    g.close()
    assert np.array_equal(pa.rowidx, I) and np.array_equal(pa.colvals, A[I, J])            # column-view order
    doms = pack_domains([L.RealDomain()] * len(lens))
    terms = [L.error_metric_entry(L.RealDomain(), L.QuadLoss(), float(X[:, i] @ Y[:, j]), A[i, j]) for i, j in zip(I, J)]
    want = sum(int(t) for t in terms)
    assert all(t == int(t) for t in terms) and 0 < want < 2 ** 53
    with Handle(pa) as (api, h):
        assert api.error_metric(h, X, Y, doms, False) == want
        for b in BLOCKS:
            out, err, total = api.impute_at(h, X, Y, doms, m, len(lens), I, J, truth=pa.colvals, block_entries=b)
            assert np.array_equal(err, np.array(terms)) and total == want, b
            assert R.same_bits(out, R.xy_chain(X, Y)[I, J])
        out2, err2, total2 = api.impute_at(h, X, Y, doms, m, len(lens), I, J, truth=pa.colvals, want_err=False)     # err may be NULL
        assert err2 is None and total2 == want
        out3, err3, total3 = api.impute_at(h, X, Y, doms, m, len(lens), I, J, truth=pa.colvals, want_total=False)   # and so may err_total
        assert total3 is None and np.array_equal(err3, np.array(terms))
        _, err0, total0 = api.impute_at(h, X, Y, doms, m, len(lens), I[:0], J[:0], truth=np.zeros(0))               # no entries: 0.0
        assert err0.shape == (0,) and total0 == 0.0 and np.signbit(total0) == False


def test_errors_periodic_bool_and_categorical_are_exact():
    """The columns of test_error_metric_periodic_bool_and_categorical_are_exact: squared distances on the circle in multiples of 1/16 and
    misclassification counts, entry by entry against the mirror."""
    T = 2.5
    B = L.BoolDomain()
    pairs = [(L.PeriodicDomain(T), L.QuadLoss()), (L.PeriodicDomain(T), L.PeriodicLoss(T)), (B, L.LogisticLoss()), (B, L.QuadLoss()),
             (L.CategoricalDomain(4), L.MultinomialLoss(4)), (L.CategoricalDomain(3), L.OvALoss(3, bin_loss=L.HingeLoss()))]
    m, k = 200, 2
    rng = np.random.default_rng(25)
    losses = [l for _, l in pairs]
    X, Y = factors(rng, m, k, L.embedding_dim(losses))
    A = np.stack([rng.choice([0.0, -T, T, 2 * T, -2 * T, -1.0, 1.25, 3.75, -0.25], m), rng.integers(-12, 13, m) / 4.0, rng.integers(0, 2, m),
                  rng.integers(0, 2, m), rng.integers(1, 5, m), rng.integers(1, 4, m)], axis=1).astype(np.float64)
    I, J = np.nonzero(rng.random(A.shape) < 0.7)
    order = np.lexsort((I, J))
    I, J = I[order], J[order]
    g = L.GLRM(A, losses, L.ZeroReg(), L.ZeroReg(), k, obs=(I, J), X=X, Y=Y)
    pa, doms = g.problem_arrays(), pack_domains([D for D, _ in pairs])
    g.close()
    U = R.xy_chain(X, Y)
    spans = L.get_yidxs(losses)
    terms = np.array([L.error_metric_entry(pairs[j][0], losses[j], U[i, spans[j][0]:spans[j][1]] if losses[j].embedding_dim > 1 else float(U[i, spans[j][0]]), A[i, j])
                      for i, j in zip(I, J)])
    want = float(np.sum(terms))
    assert all(t * 16 == int(t * 16) for t in terms) and want > 0
    with Handle(pa) as (api, h):
        assert api.error_metric(h, X, Y, doms, False) == want
        for b in BLOCKS:
            out, err, total = api.impute_at(h, X, Y, doms, m, len(pairs), I, J, truth=A[I, J], block_entries=b)
            assert R.same_bits(err, terms) and total == want, b
        info = api.impute_at_info()
        assert info["entries_general"] == int((J >= 4).sum()) > 0


def test_err_total_is_the_ordered_device_sum_whatever_the_blocks():
    """Standard normal factors and truth, 200000 pairs (three rounds of the 65536 accumulators and a part of a fourth): the total is
    glrm_hip_sum's fixed order over the whole err vector, to the bit, for every way of blocking."""
    pa, X, Y, doms = scalar_model("quad", 20)
    rng = np.random.default_rng(77)
    P = 200000
    rows, cols, truth = rng.integers(0, M, P), rng.integers(0, N, P), rng.standard_normal(P)
    with Handle(pa) as (api, h):
        totals = []
        for b in [0, 65536, 65543, 1000]:
            out, err, total = api.impute_at(h, X, Y, doms, M, N, rows, cols, truth=truth, block_entries=b)
            totals.append(total)
            assert R.same_bits(err, (out - truth) * (out - truth))
        assert len({np.float64(t).view(np.uint64) for t in totals}) == 1, totals
        assert np.float64(totals[0]).view(np.uint64) == np.float64(sum_like_the_device(err)).view(np.uint64)


# ================================================================== 5. factors

def test_resident_factors_and_recommend_scores():
    pa, X, Y, doms = scalar_model("quad", 20)
    rng = np.random.default_rng(5)
    rows, cols = draw_pairs(rng, 300, M, N)
    with Handle(pa) as (api, h):
        passed = api.impute_at(h, X, Y, doms, M, N, rows, cols)
        api.set_factors(h, X, Y)
        assert R.same_bits(api.impute_at(h, None, None, doms, M, N, rows, cols), passed)      # the NULL-factor form
        assert R.same_bits(api.impute_at(h, None, None, doms, M, N, rows=SLAB_ROWS), api.impute_at(h, X, Y, doms, M, N, rows=SLAB_ROWS))
        fn = api._f["impute_at"]
        out = np.full(300, -7.0)
        for Xp, Yp in ((X.ctypes.data, None), (None, Y.ctypes.data)):
            assert fn(h, Xp, Yp, doms.ctypes.data, rows.ctypes.data, 300, cols.ctypes.data, 300, 0, None, 0, out.ctypes.data, None, None) == _capi.ERR_INVALID
            assert "both" in api.last_error() and (out == -7.0).all()
        tc, tv, _ = api.row_topk(h, X, Y, None, 5, exclude=False)                            # recommend's scores are these entries
        assert R.same_bits(api.impute_at(h, X, Y, doms, M, N, np.repeat(np.arange(M), 5), tc.reshape(-1)), tv.reshape(-1))
    with Handle(pa) as (api, h):                                                              # a fresh handle has no factors yet
        with pytest.raises(_capi.GLRMError) as ei:
            api.impute_at(h, None, None, doms, M, N, rows, cols)
        assert ei.value.code == _capi.ERR_INVALID and "no factors" in ei.value.message


# ================================================================== 6. refusals

def test_refusals_touch_nothing():
    pa, X, Y, doms = scalar_model("quad", 5)
    api = hip()
    rows, cols, truth = np.array([3, 5, 129], dtype=np.int64), np.array([0, 69, 7], dtype=np.int32), np.zeros(3)
    out, err, tot = np.full(3 * N, -7.0), np.full(3 * N, -7.0), np.full(1, -7.0)
    p = lambda a: None if a is None else a.ctypes.data                                       # noqa: E731

    def refused(h, code, word, *, X=X, Y=Y, d=doms, r=rows, nr=3, c=cols, nc=3, mode=0, t=truth, b=0, o=out, e=err, s=tot):
        rc = api._f["impute_at"](h, p(X), p(Y), p(d), p(r), nr, p(c), nc, mode, p(t), b, p(o), p(e), None if s is None else s.ctypes.data_as(_capi.C.POINTER(_capi.C.c_double)))
        assert rc == code and word in api.last_error(), (rc, api.last_error())
        assert (out == -7.0).all() and (err == -7.0).all() and (tot == -7.0).all()           # a refusal touches nothing

    with Handle(pa) as (_, h):
        I = _capi.ERR_INVALID
        refused(h, I, "rows[1] = 130", r=np.array([3, 130, 0], dtype=np.int64))
        refused(h, I, "rows[0] = -1", r=np.array([-1, 0, 0], dtype=np.int64))
        refused(h, I, "cols[2] = 70", c=np.array([0, 0, 70], dtype=np.int32))
        refused(h, I, "cols[0] = -1", c=np.array([-1, 0, 0], dtype=np.int32))
        refused(h, I, "rows[0] = 130", r=np.array([130, 0, 0], dtype=np.int64), c=None, nc=0, mode=1, t=None, e=None, s=None)
        refused(h, I, "cols[1] = 70", c=np.array([0, 70, 0], dtype=np.int32), r=None, nr=0, mode=2, t=None, e=None, s=None)
        refused(h, I, "negative", nr=-1, nc=-1)
        refused(h, I, "n_rows 3 == n_cols 2", nc=2)                                          # counts that do not fit the mode
        refused(h, I, "row slab", mode=1)
        refused(h, I, "row slab", mode=1, c=None, nc=1)
        refused(h, I, "column slab", mode=2)
        refused(h, I, "NULL", r=None)
        refused(h, I, "mode 3", mode=3)
        refused(h, I, "mode -1", mode=-1)
        refused(h, I, "out is NULL", o=None)
        refused(h, I, "domains is NULL", d=None)
        refused(h, I, "need truth", t=None, s=None)
        refused(h, I, "need truth", t=None, e=None)
        refused(h, I, "block_entries -1", b=-1)
        for field, value in (("kind", 6), ("kind", -1), ("reserved", 1)):
            d = doms.copy()
            d[N // 2][field] = value
            refused(h, I, "domain descriptor 35 is invalid", d=d)
        refused(h, I, "both", Y=None)
        refused(None, I, "NULL handle")
        rc = api._f["impute_at"](h, p(X), p(Y), p(doms), p(rows), 3, p(cols), 3, 0, p(truth), 0, p(out), None, None)   # err and err_total may be NULL
        assert rc == 0 and R.same_bits(out[:3], api.impute(h, X, Y, doms, M, N)[rows, cols]) and (out[3:] == -7.0).all()
        out[:] = -7.0

    g = L.GLRM(np.ones((64, 48)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 16)                 # (k = 16: eligible for the dense hand-over)
    Xg, Yg, dg = np.zeros((16, 64), order="F"), np.zeros((16, 48), order="F"), pack_domains([L.RealDomain()] * 48)
    r2, c2 = np.array([3, 5, 63], dtype=np.int64), np.array([0, 47, 7], dtype=np.int32)
    for make, code, word in ((lambda: api.create(g.problem_arrays(dense=True)), _capi.ERR_UNSUPPORTED, "dense_A"),
                             (lambda: api.create(g.problem_arrays(), storage=_capi.STORAGE_F32), _capi.ERR_UNSUPPORTED, "storage = f32"),
                             (lambda: api.create(g.problem_arrays(rows=(0, 32))), _capi.ERR_INVALID, "single-shard"),
                             (lambda: api.create(g.problem_arrays(), defer=True), _capi.ERR_INVALID, "glrm_hip_finalize")):
        hh = make()
        try:
            refused(hh, code, word, X=Xg, Y=Yg, d=dg, r=r2, c=c2)
        finally:
            api.destroy(hh)
    g.close()


@pytest.mark.parametrize("name,D,loss", UNSUPPORTED_PAIRS, ids=[u[0] for u in UNSUPPORTED_PAIRS])
def test_an_unsupported_column_is_refused_only_where_it_is_queried(name, D, loss):
    pairs = [(L.RealDomain(), L.QuadLoss()), (L.CategoricalDomain(3), L.OvALoss(3)), (D, loss), (L.OrdinalDomain(1, 7), L.HuberLoss())]
    g, X, Y, doms = table_model(pairs, 130, 3, seed=5)
    pa, losses = g.problem_arrays(), list(g.losses)
    g.close()
    U = R.xy_chain(X, Y)
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 130, 400).astype(np.int64)
    cols = rng.choice([0, 1, 3], 400).astype(np.int32)
    with Handle(pa) as (api, h):
        with pytest.raises(_capi.GLRMError) as ei:
            api.impute(h, X, Y, doms, 130, 4)                                                # the full matrix computes every column
        assert ei.value.code == _capi.ERR_UNSUPPORTED
        got = api.impute_at(h, X, Y, doms, 130, 4, rows, cols)                               # nobody asks for column 2
        assert R.same_bits(got, mirror(pairs, losses, U, rows, cols))
        slab = api.impute_at(h, X, Y, doms, 130, 4, cols=[3, 0, 1])
        ii, jj = np.tile(np.arange(130), 3), np.repeat([3, 0, 1], 130)
        assert R.same_bits(slab.reshape(-1, order="F"), mirror(pairs, losses, U, ii, jj))
        out = np.full(400 * 4, -7.0)
        fn = api._f["impute_at"]
        touching = cols.copy()
        touching[399] = 2
        only = np.array([1, 2], dtype=np.int32)
        for args in ((rows.ctypes.data, 400, touching.ctypes.data, 400, 0),                  # one pair in the column
                     (rows.ctypes.data, 400, None, 0, 1),                                    # whole rows cross it
                     (None, 0, only.ctypes.data, 2, 2)):                                     # the column itself
            assert fn(h, X.ctypes.data, Y.ctypes.data, doms.ctypes.data, *args, None, 0, out.ctypes.data, None, None) == _capi.ERR_UNSUPPORTED
            assert "column 2 is queried" in api.last_error() and (out == -7.0).all()
        assert R.same_bits(api.impute_at(h, X, Y, doms, 130, 4, rows, cols), got)            # the handle serves the next call


# ================================================================== the driver

def test_the_driver():
    rng = np.random.default_rng(28)
    m, n, k = 60, 40, 3
    A = rng.standard_normal((m, k)) @ rng.standard_normal((k, n))
    I, J = np.nonzero(rng.random((m, n)) < 0.4)
    g = L.GLRM(A, L.QuadLoss(), L.QuadReg(.1), L.QuadReg(.1), k, obs=(I, J), rng=np.random.default_rng(29))
    L.fit_b(g, L.Params(1, max_iter=10, abs_tol=1e-5, min_stepsize=0.01), verbose=False, engine=hip())
    U = L.impute(g, engine=hip())
    held = ~np.isin(np.arange(m * n), I * n + J)
    hi, hj = np.nonzero(held.reshape(m, n))
    assert R.same_bits(L.impute_at(g, hi, hj), U[hi, hj])
    assert R.same_bits(L.impute_at(g, rows=[59, 0, 0]), U[[59, 0, 0], :]) and R.same_bits(L.impute_at(g, cols=[39, 1]), U[:, [39, 1]])
    err, total = L.error_metric_at(g, hi, hj, A[hi, hj])
    assert R.same_bits(err, (U[hi, hj] - A[hi, hj]) ** 2) and total == pytest.approx(float(np.sum(err)), rel=1e-12)
    assert R.same_bits(L.impute_at(g, hi, hj, X=g.X.copy(), Y=g.Y.copy(), domains=[L.RealDomain()] * n), U[hi, hj])
    gb = L.GLRM(A > 0, L.LogisticLoss(), L.ZeroReg(), L.ZeroReg(), k, X=g.X.copy(), Y=g.Y.copy())
    got = L.impute_at(gb, hi, hj)                                                            # Bool columns come back as 1.0 / 0.0
    assert got.dtype == np.float64 and set(np.unique(got)) <= {0.0, 1.0} and np.array_equal(got, (U[hi, hj] >= 0).astype(float))
    gb.close()
    with pytest.raises(ValueError, match="impute"):
        L.impute_at(g)
    with pytest.raises(_capi.GLRMError) as ei:
        L.impute_at(g, [m], [0])
    assert ei.value.code == _capi.ERR_INVALID
    g.close()


# ================================================================== 7. leaks

def test_no_device_memory_leak():
    """20 calls leave device memory where it was.  A call's scratch is tens of MiB here (10^6 pairs x 36 B), so a call that kept it would
    lose hundreds of MiB; the better of two windows of 10 calls is held to 4 MiB, as for row_topk (tests/test_gpu_recommend.py)."""
    pa, X, Y, doms = scalar_model("quad", 20)
    rng = np.random.default_rng(30)
    P = 1000000
    rows, cols, truth = rng.integers(0, M, P), rng.integers(0, N, P), rng.standard_normal(P)
    with Handle(pa) as (api, h):
        first = api.impute_at(h, X, Y, doms, M, N, rows, cols, truth=truth)
        api.impute_at(h, X, Y, doms, M, N, rows, cols, truth=truth)
        levels = [free_bytes()]
        for _ in range(2):
            for _ in range(10):
                last = api.impute_at(h, X, Y, doms, M, N, rows, cols, truth=truth)
            levels.append(free_bytes())
        assert R.same_bits(last[0], first[0]) and R.same_bits(last[1], first[1]) and last[2] == first[2]
        lost = [levels[i] - levels[i + 1] for i in range(2)]
        assert min(lost) < 4 << 20, f"device memory lost per window of 10 calls (MiB): {[round(x / 2**20, 1) for x in lost]}"
