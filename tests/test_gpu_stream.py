"""-m gpu: glrm_hip_stream_rows / glrm_hip_stream_info (include/glrm_hip_stream.h; csrc/glrm_stream.hip, csrc/glrm_stream.hpp) and the
drivers over them.

The contract is bit for bit: the header fixes every operation and its order, tests/stream_ref.py restates it in numpy (and
tests/test_stream.py holds that restatement to a derived backward-error bound and to a literal transcription of the reference's loop), and
every comparison below is ``tobytes`` equality -- X, Y, the query results, and the objective wherever a row was solved (a kept row's
objective is NaN on both sides).  The status of every row is compared as well.

first = 16 everywhere.  The three patterns are those of tests/test_stream.py, which asserts that the first two have levels at least 4 rows
wide and that the third is one chain: every k runs both launch shapes.  The ragged pattern has rows of 0, 1, 33 and 65 observations (on
either side of ALS_CHUNK = 32 and of two chunks), rows that name a column twice, and ZeroReg rows shorter than k, which are kept.
"""
import functools

import numpy as np
import pytest

import stream_ref as S
import lowrankmodels.jl_amd as L
from lowrankmodels.jl_amd import _capi

pytestmark = pytest.mark.gpu
FIRST = 16
STEP = 0.05
PATTERNS = ((160, 64, 3, 1), (200, 256, 4, 1), (96, 24, 24, 1))     # m, n, observations per row, seed
KS = (1, 8, 17, 32, 33, 64)
COUNTERS = ("trials_x", "trials_y", "accepts_x", "accepts_y", "launches_x", "launches_y")


def hip():
    return _capi.hip_api()


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def pattern_problem(case, k, sy=0.3):
    m, n, q, seed = PATTERNS[case]
    lists = S.pattern(m, n, q, seed)
    g, X0, Y0 = S.model(lists, n, k, seed=10 * case + k, sy=sy)
    return (g.problem_arrays(),) + frozen(X0, Y0) + (lists,)


@functools.lru_cache(maxsize=None)
def ragged_problem(k=8, sy=0.3):
    """59 rows over 80 columns: lengths from {0, 1, 33, 65} and a few others, six rows that name a column twice (one of them 40 times:
    more than a staging chunk), per-row scales from {0, 0.1, 2.5}: ZeroReg rows shorter than k are kept."""
    rng = np.random.default_rng(4242)
    m, n = 59, 80
    lens = rng.choice([0, 1, 5, 12, 33, 65], size=m)
    lens[FIRST:FIRST + 4] = [0, 1, 33, 65]
    lists = [rng.choice(n, l, replace=False) for l in lens]
    for i in (FIRST + 5, FIRST + 9, FIRST + 10, FIRST + 20, FIRST + 30):
        l = lists[i] if len(lists[i]) else np.array([3])
        lists[i] = np.concatenate([l, l[:2], l[:1]])                              # a column three times, another twice
    lists[FIRST + 12] = np.concatenate([rng.choice(n, 30, replace=False), np.full(40, 7)])
    g, X0, Y0 = S.model(lists, n, k, seed=99, rx_scales=(0.0, 0.1, 2.5), sy=sy)
    return (g.problem_arrays(),) + frozen(X0, Y0) + (lists,)


def neighbour_queries(lists, n, seed=5):
    """per row: a column the row before writes, one the row after writes, two random ones"""
    rng = np.random.default_rng(seed)
    m = len(lists)
    out = [np.zeros(0, dtype=np.int64)] * m
    for i in range(FIRST, m):
        near = [l[:1] for l in (lists[i - 1], lists[min(i + 1, m - 1)]) if len(l)]
        out[i] = np.concatenate(near + [rng.choice(n, 2)]).astype(np.int64)
    return S.csr(out)


@functools.lru_cache(maxsize=None)
def reference(kind, case, k, interval, queries=False, sy=0.3):
    pa, X0, Y0, lists = pattern_problem(case, k, sy) if kind == "pattern" else ragged_problem(k, sy)
    qptr, qcol = neighbour_queries(lists, pa.n) if queries else (None, None)
    out = S.stream_rows(pa, X0, Y0, FIRST, STEP, interval, qptr, qcol)
    frozen(*(v for v in out.values() if v is not None))
    return out


def factors(api, h, pa):
    X, Y = np.zeros((pa.k, pa.m), order="F"), np.zeros((pa.k, pa.n), order="F")
    api.get_factors(h, X, Y)
    return X, Y


def on_device(pa, X0, Y0, interval, sequential=False, qptr=None, qcol=None, calls=1, first=FIRST, step=STEP):
    api = hip()
    h = api.create(pa)
    try:
        api.set_factors(h, X0, Y0)
        for _ in range(calls):
            obj, qout = api.stream_rows(h, pa.m, first, step, interval, sequential=sequential, qptr=qptr, qcol=qcol)
        info = api.stream_info(h, rows=pa.m - first)
        X, Y = factors(api, h, pa)
        stats = api.kernel_stats(h)
    finally:
        api.destroy(h)
    return dict(X=X, Y=Y, objective=obj, qout=qout, status=info["status"], info=info, stats=stats)


def same_bits(got, ref, what=""):
    bad = np.flatnonzero(got["status"] != ref["status"])
    assert bad.size == 0, (what, "status of rows", bad[:10] + FIRST, got["status"][bad[:10]], ref["status"][bad[:10]])
    bad = np.flatnonzero(np.any(got["X"] != ref["X"], axis=0))
    assert bad.size == 0, (what, "rows of X", bad[:10])
    bad = np.flatnonzero(np.any(got["Y"] != ref["Y"], axis=0))
    assert bad.size == 0, (what, "columns of Y", bad[:10])
    assert got["X"].tobytes() == np.asfortranarray(ref["X"]).tobytes() and got["Y"].tobytes() == np.asfortranarray(ref["Y"]).tobytes()
    solved = ref["status"] == S.SOLVED
    assert got["objective"][solved].tobytes() == ref["objective"][solved].tobytes(), what
    assert np.all(np.isnan(got["objective"][~solved])) and np.all(np.isnan(ref["objective"][~solved]))
    if ref["qout"] is not None:
        bad = np.flatnonzero(got["qout"] != ref["qout"])
        assert bad.size == 0 and got["qout"].tobytes() == ref["qout"].tobytes(), (what, "queries", bad[:10])
    assert all(got["stats"][c] == 0 for c in COUNTERS), got["stats"]              # glrm_kernel_stats is not touched
    assert {c: got["info"][c] for c in ("solved", "kept_short", "kept_pivot")} == S.A_.counts(ref["status"])


@pytest.mark.parametrize("case", range(3))
@pytest.mark.parametrize("k", KS)
def test_the_three_patterns_equal_the_restatement_bit_for_bit(k, case):
    pa, X0, Y0, lists = pattern_problem(case, k)
    ref = reference("pattern", case, k, 10)
    got = on_device(pa, X0, Y0, 10)
    same_bits(got, ref, (k, case))
    assert np.all(ref["status"] == S.SOLVED) and got["X"][:, :FIRST].tobytes() == np.asfortranarray(X0[:, :FIRST]).tobytes()
    ptr, idx = S.csr(lists)
    want = S.plan(pa.m, pa.n, FIRST, ptr, idx)
    assert {c: got["info"][c] for c in ("nlevels", "nlaunches", "max_width")} == {c: want[c] for c in ("nlevels", "nlaunches", "max_width")}
    if case < 2:
        assert got["info"]["max_width"] >= 4                                      # wide levels ran
    else:
        assert got["info"]["nlaunches"] == 1 and got["info"]["nlevels"] == pa.m - FIRST   # one chain ran


@pytest.mark.parametrize("interval", (1, 3, 10))
@pytest.mark.parametrize("k", (8, 33))
def test_ragged_rows_dup_rows_and_kept_rows_at_three_intervals(k, interval):
    """m = 59 is a multiple of none of the intervals; rows of 0, 1, 33 and 65 observations; dup rows; ZeroReg rows shorter than k."""
    pa, X0, Y0, lists = ragged_problem(k)
    ref = reference("ragged", 0, k, interval)
    got = on_device(pa, X0, Y0, interval)
    same_bits(got, ref, (k, interval))
    c = S.A_.counts(ref["status"])
    assert c["kept_short"] > 0 and c["solved"] > 0
    kept = ref["status"] != S.SOLVED
    assert got["X"][:, FIRST:][:, kept].tobytes() == np.asfortranarray(X0[:, FIRST:][:, kept]).tobytes()   # a kept row keeps every bit
    ptr, idx = S.csr(lists)
    assert S.plan(pa.m, pa.n, FIRST, ptr, idx)["dup_rows"] == 6


def test_sy_zero_divides_nothing():
    pa, X0, Y0, lists = ragged_problem(8, 0.0)
    ref = reference("ragged", 0, 8, 3, sy=0.0)
    same_bits(on_device(pa, X0, Y0, 3), ref)
    pa2, X2, Y2, lists2 = pattern_problem(1, 8, 0.0)                              # 256 columns, 4 per row: some are never written
    got = on_device(pa2, X2, Y2, 3)
    same_bits(got, reference("pattern", 1, 8, 3, sy=0.0))
    untouched = np.setdiff1d(np.arange(pa2.n), np.concatenate(lists2[FIRST:]))
    assert untouched.size > 0 and got["Y"][:, untouched].tobytes() == np.asfortranarray(Y2[:, untouched]).tobytes()


@pytest.mark.parametrize("case", range(3))
def test_sequential_gives_the_same_bits_through_the_other_launch_shape(case):
    pa, X0, Y0, lists = pattern_problem(case, 17)
    ref = reference("pattern", case, 17, 3)
    par, seq = on_device(pa, X0, Y0, 3), on_device(pa, X0, Y0, 3, sequential=True)
    same_bits(par, ref, "level by level")
    same_bits(seq, ref, "sequential")
    assert (seq["info"]["nlaunches"], seq["info"]["max_width"], seq["info"]["nlevels"]) == (1, 1, pa.m - FIRST)
    if case < 2:
        assert par["info"]["max_width"] >= 4 and par["info"]["nlaunches"] > 1     # neither path can stand in for the other
    else:
        assert par["info"]["nlaunches"] == 1
    pa, X0, Y0, _ = ragged_problem(8)
    same_bits(on_device(pa, X0, Y0, 3, sequential=True), reference("ragged", 0, 8, 3), "ragged, sequential")


@pytest.mark.parametrize("kind,case,k", [("pattern", 0, 8), ("pattern", 1, 33), ("pattern", 2, 8), ("ragged", 0, 8)])
def test_queries_on_columns_a_neighbouring_row_writes(kind, case, k):
    pa, X0, Y0, lists = pattern_problem(case, k) if kind == "pattern" else ragged_problem(k)
    qptr, qcol = neighbour_queries(lists, pa.n)
    ref = reference(kind, case, k, 3, queries=True)
    got = on_device(pa, X0, Y0, 3, qptr=qptr, qcol=qcol)
    same_bits(got, ref, (kind, case, k))
    assert len(got["qout"]) == qptr[-1] > 0 and np.all(np.isfinite(got["qout"]))
    want = S.plan(pa.m, pa.n, FIRST, *S.csr(lists), qptr, qcol)
    assert got["info"]["nlevels"] == want["nlevels"] and got["info"]["max_width"] == want["max_width"]
    plain = reference(kind, case, k, 3)                                           # a reader writes nothing
    assert got["X"].tobytes() == np.asfortranarray(plain["X"]).tobytes() and got["Y"].tobytes() == np.asfortranarray(plain["Y"]).tobytes()
    same_bits(on_device(pa, X0, Y0, 3, sequential=True, qptr=qptr, qcol=qcol), ref, "sequential")


def test_what_the_header_lists_as_not_written_is_not_written():
    import torch
    pa, X0, Y0, _ = pattern_problem(0, 17)
    api = hip()
    h = api.create(pa)
    try:
        ld = api.factor_ld(h)
        dX, dY = torch.zeros(ld * pa.m, dtype=torch.float64, device="cuda"), torch.zeros(ld * pa.n, dtype=torch.float64, device="cuda")
        oc, orow = torch.full((pa.n,), 7.5, dtype=torch.float64, device="cuda"), torch.full((pa.m,), -3.25, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        api.bind_buffers(h, dX.data_ptr(), dY.data_ptr(), oc.data_ptr(), orow.data_ptr())
        api.set_factors(h, X0, Y0)
        api.synchronize(h)
        rawX0, rawY0 = dX.cpu().numpy().reshape(pa.m, ld).copy(), dY.cpu().numpy().reshape(pa.n, ld).copy()
        api.stream_rows(h, pa.m, FIRST, STEP, 3)
        rawX, rawY = dX.cpu().numpy().reshape(pa.m, ld), dY.cpu().numpy().reshape(pa.n, ld)
        assert ld == 32
        assert rawX[:, 17:].tobytes() == rawX0[:, 17:].tobytes() and rawY[:, 17:].tobytes() == rawY0[:, 17:].tobytes()   # components k .. ld-1
        assert rawX[:FIRST].tobytes() == rawX0[:FIRST].tobytes()                                                          # rows below first
        assert np.all(oc.cpu().numpy() == 7.5) and np.all(orow.cpu().numpy() == -3.25)                                    # obj_by_col / obj_by_row
        ref = reference("pattern", 0, 17, 3)
        assert np.asfortranarray(rawX[:, :17].T).tobytes() == np.asfortranarray(ref["X"]).tobytes()
        assert np.asfortranarray(rawY[:, :17].T).tobytes() == np.asfortranarray(ref["Y"]).tobytes()
        assert all(api.kernel_stats(h)[c] == 0 for c in COUNTERS)
    finally:
        api.destroy(h)


def test_a_half_step_after_a_streaming_call_is_a_fresh_handles():
    """the step sizes, the counters and the objective vectors are untouched: step_x and step_y after the pass leave the bits a fresh handle
    with the same factors leaves"""
    pa, X0, Y0, _ = pattern_problem(1, 8)
    api = hip()

    def steps(h):
        api.step_x(h, 0.01)
        api.step_y(h, 0.01)
        return factors(api, h, pa) + (api.kernel_stats(h),)
    h = api.create(pa)
    try:
        api.set_factors(h, X0, Y0)
        api.reset_stepsizes(h, 1.0)
        api.stream_rows(h, pa.m, FIRST, STEP, 3)
        X1, Y1 = factors(api, h, pa)
        Xa, Ya, sa = steps(h)
    finally:
        api.destroy(h)
    h = api.create(pa)
    try:
        api.set_factors(h, X1, Y1)
        api.reset_stepsizes(h, 1.0)
        Xb, Yb, sb = steps(h)
    finally:
        api.destroy(h)
    assert Xa.tobytes() == Xb.tobytes() and Ya.tobytes() == Yb.tobytes() and not np.array_equal(Xa, X1)
    assert all(sa[c] == sb[c] for c in COUNTERS), (sa, sb)


def test_two_calls_on_one_handle_are_two_fresh_handles():
    """epoch is zeroed by every call"""
    pa, X0, Y0, _ = pattern_problem(1, 8)
    ref = reference("pattern", 1, 8, 3)
    again = S.stream_rows(pa, ref["X"], ref["Y"], FIRST, STEP, 3)
    got = on_device(pa, X0, Y0, 3, calls=2)
    same_bits(got, again, "second call")
    assert not np.array_equal(again["Y"], ref["Y"])


def test_the_drivers_run_on_the_device():
    T0 = FIRST
    lists = S.pattern(60, 20, 6, 8)
    g = S.model(lists, 20, 3, seed=8, rx_scales=(0.1, 0.5))[0]
    p = L.StreamingParams(T0, stepsize=STEP, Y_update_interval=3)
    init = L.keep_rows(g, T0)
    L.init_svd_(init)
    init.close()
    X, Y, ch = L.streaming_fit(g, p, verbose=False)
    try:
        X0 = np.asfortranarray(g.X.copy())
        X0[:, :T0] = init.X
        ref = S.stream_rows(g.problem_arrays(), X0, init.Y, T0, STEP, 3)
        assert g.X.tobytes() == np.asfortranarray(ref["X"]).tobytes() and g.Y.tobytes() == np.asfortranarray(ref["Y"]).tobytes()
        assert np.array(ch.objective).tobytes() == ref["objective"].tobytes() and ch.times == []
        assert g._stream_info["solved"] == g.m - T0 and g._stream_info["plan_ms"] >= 0.0
    finally:
        g.close()
    g2 = S.model(lists, 20, 3, seed=8, rx_scales=(0.1, 0.5))[0]
    rows, cols = np.array([59, 20, 20, 33]), np.array([0, 19, 3, 7])
    vals = L.streaming_impute_at(g2, rows, cols, p)
    g2.close()
    qptr = np.zeros(61, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=60), out=qptr[1:])
    order = np.argsort(rows, kind="stable")
    want = S.stream_rows(g.problem_arrays(), X0, init.Y, T0, STEP, 3, qptr, cols[order].astype(np.int32))["qout"]
    assert vals[order].tobytes() == want.tobytes()


# ------------------------------------------------------------------ refusals

def refused(call, code, *words):
    with pytest.raises(_capi.GLRMError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, ei.value.message)
    for w in words:
        assert w in ei.value.message, (w, ei.value.message)
    return ei.value.message


def test_refusals_name_what_was_found_and_leave_the_factors_alone():
    from lowrankmodels.jl_amd.stream import check_model
    api = hip()
    rng = np.random.default_rng(5)
    m, n = 24, 18
    A = rng.standard_normal((m, n))
    obs = np.nonzero(rng.random((m, n)) < 0.6)
    q = L.QuadReg(0.1)
    HDR = "include/glrm_hip_stream.h"

    def model(losses=None, rx=q, ry=q, k=4, **kw):
        return L.GLRM(A, L.QuadLoss() if losses is None else losses, rx, ry, k, obs=obs, rng=np.random.default_rng(1), **kw)

    def on_handle(g, body, vec=False, **create_kw):
        from lowrankmodels.jl_amd.fit import install_regularizers
        h = api.create(g.problem_arrays(), **create_kw)
        try:
            if vec:
                install_regularizers(api, h, g)
            X, Y = np.asfortranarray(g.X), np.asfortranarray(g.Y)
            if create_kw.get("storage"):
                X, Y = (np.asfortranarray(F.astype(np.float32).astype(np.float64)) for F in (X, Y))
            api.set_factors(h, X, Y)
            body(h)
            X1, Y1 = np.zeros_like(X), np.zeros_like(Y)
            api.get_factors(h, X1, Y1)
            assert X1.tobytes() == X.tobytes() and Y1.tobytes() == Y.tobytes()          # nothing written
        finally:
            api.destroy(h)

    def run(h, first=4, step=0.1, interval=2, **kw):
        return api.stream_rows(h, m, first, step, interval, **kw)

    def arguments(h):
        refused(lambda: api.stream_info(h), _capi.ERR_INVALID, "has not run")
        refused(lambda: run(h, first=0), _capi.ERR_INVALID, "first must be in 1 .. m = 24", "got 0")
        refused(lambda: run(h, first=m + 1), _capi.ERR_INVALID, "first must be in 1 .. m = 24", "got 25")
        refused(lambda: run(h, interval=0), _capi.ERR_INVALID, "interval must be at least 1")
        for step in (0.0, -1.0, np.inf, np.nan):
            refused(lambda: run(h, step=step), _capi.ERR_INVALID, "stepsize must be finite and > 0")
        qptr = np.zeros(m + 1, dtype=np.int64)
        qptr[5:] = 1
        refused(lambda: run(h, qptr=qptr, qcol=np.array([n], dtype=np.int32)), _capi.ERR_INVALID, f"column {n}", "outside 0 .. 17")
        refused(lambda: run(h, qptr=qptr, qcol=np.array([-1], dtype=np.int32)), _capi.ERR_INVALID, "column -1")
        fn = api._stream("stream_rows")                                                  # half-given query pointers, at the boundary itself
        out = np.zeros(1)
        for args in ((qptr.ctypes.data, None, None), (None, np.zeros(1, dtype=np.int32).ctypes.data, None), (None, None, out.ctypes.data),
                     (qptr.ctypes.data, np.zeros(1, dtype=np.int32).ctypes.data, None)):
            assert fn(h, 4, 0.1, 2, 0, *args, None) == _capi.ERR_INVALID and "go together" in api.last_error()
        refused(lambda: api.stream_info(h), _capi.ERR_INVALID, "has not run")            # none of these was a run
    on_handle(model(), arguments)
    refused(lambda: api.stream_rows(None, m, 4, 0.1, 2), _capi.ERR_INVALID, "NULL handle")
    refused(lambda: api.stream_info(None), _capi.ERR_INVALID, "NULL handle")
    g = model()
    h = api.create(g.problem_arrays(), defer=True)
    try:
        refused(lambda: run(h), _capi.ERR_INVALID, "glrm_hip_finalize")
    finally:
        api.destroy(h)
    h = api.create(g.problem_arrays())
    try:
        refused(lambda: run(h), _capi.ERR_INVALID, "no factors on the device yet")
    finally:
        api.destroy(h)

    # the model: the engine's words are the host's (lowrankmodels.jl_amd/stream.py: check_model)
    def same_words(g, *words, **kw):
        def body(h):
            msg = refused(lambda: run(h), _capi.ERR_UNSUPPORTED, HDR, *words)
            with pytest.raises(_capi.GLRMError) as ei:
                check_model(g)
            assert msg == ei.value.message, (msg, ei.value.message)
        on_handle(g, body, **kw)
    same_words(model(losses=L.HuberLoss()), "column 0 has loss kind 2", "needs QuadLoss")
    same_words(model(losses=[L.QuadLoss()] * 7 + [L.L1Loss()] + [L.QuadLoss()] * 10), "column 7 has loss kind 1")
    same_words(model(losses=L.QuadLoss(2.0)), "column 0 is QuadLoss with scale 2", "exactly 1")
    same_words(model(losses=[L.QuadLoss()] * 7 + [L.QuadLoss(0.5)] + [L.QuadLoss()] * 10), "column 7 is QuadLoss with scale 0.5")
    same_words(model(rx=L.NonNegConstraint()), "rx[0] has regularizer kind 3, wrap 0")
    same_words(model(ry=[q] * 5 + [L.OneReg(0.3)] + [q] * 12), "ry[5] has regularizer kind 2")
    same_words(model(rx=L.QuadReg(-0.5)), "rx[0] is QuadReg with scale -0.5")
    same_words(model(ry=[q] * 5 + [L.QuadReg(0.3)] + [q] * 12), "ry[5] has scale 0.3 and ry[0] has 0.1", "equal scales")
    same_words(model(ry=[q] * 5 + [L.ZeroReg()] + [q] * 12), "ry[5] has scale 0 and ry[0] has 0.1")
    same_words(model(k=65), "rank k = 65 is above GLRM_STREAM_MAX_K = 64")
    same_words(model(offset=True), "rx[0] has regularizer kind 1, wrap 1")
    # ZeroReg is taken as scale 0: a ZeroReg / QuadReg(0) mix on the columns has equal scales and runs
    g = model(ry=[L.ZeroReg()] * 5 + [L.QuadReg(0.0)] + [L.ZeroReg()] * 12)
    h = api.create(g.problem_arrays())
    try:
        api.set_factors(h, np.asfortranarray(g.X), np.asfortranarray(g.Y))
        run(h)
        assert api.stream_info(h)["solved"] == m - 4
    finally:
        api.destroy(h)
    # a regularizer that carries a vector
    gv = model()
    gv.ry = _capi.TrackedList(L.fixed_latent_features(r, gv.Y[:2, j]) for j, r in enumerate(gv.ry))
    on_handle(gv, lambda h: refused(lambda: run(h), _capi.ERR_UNSUPPORTED, HDR), vec=True)

    # the handle
    on_handle(model(), lambda h: refused(lambda: run(h), _capi.ERR_UNSUPPORTED, HDR, "storage = f32"), storage=1)
    full = L.GLRM(A, L.QuadLoss(), q, q, 12, rng=np.random.default_rng(1))
    assert full.dense_eligible()
    h = api.create(full.problem_arrays(dense=True))
    try:
        api.set_factors(h, np.asfortranarray(full.X), np.asfortranarray(full.Y))
        refused(lambda: run(h), _capi.ERR_UNSUPPORTED, HDR, "dense_A")
    finally:
        api.destroy(h)
    g = model()
    h = api.create(g.problem_arrays(rows=(0, m // 2)), defer=True)
    try:
        api.finalize(h, api.signature(h))
        api.set_factors(h, np.asfortranarray(g.X), np.asfortranarray(g.Y))
        refused(lambda: run(h), _capi.ERR_UNSUPPORTED, HDR, "this one is a shard", f"rows [0, {m // 2}) of {m}")
    finally:
        api.destroy(h)
