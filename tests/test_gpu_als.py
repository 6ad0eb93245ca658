"""-m gpu: glrm_hip_als_solve / glrm_hip_als_info (include/glrm_hip_als.h; csrc/glrm_als.hip, csrc/glrm_als.hpp) and the drivers over them.

The contract is bit for bit: the header fixes every operation and its order, tests/als_ref.py restates it in numpy (and tests/test_als.py
holds that restatement to a derived backward-error bound), and every comparison below is ``tobytes`` equality -- the same operations in
the same order, so there is no allowance.  The status of every segment is compared as well, and the three counts are asserted one by one,
so nothing passes by keeping everything.

Problems follow the recipe of tests/test_gpu_transform.py::from_lengths: N = 257 opposing vectors, lists in ascending index order (the
order every family then holds), seeded.  Segment lengths {0, 1, k-1, k, k+1, 63, 64, 65, 100, 300}, every one present: 65 is two full
staging chunks of the kernel (ALS_CHUNK = 32, csrc/glrm_als.hpp) plus one observation, 300 > N repeats opposing indices.  One segment
repeats ONE index k + 3 times: rank 1, a failed pivot where k > 1.  Per-segment penalty scales from {0, 0.1, 2.5}, per-column loss scales
from {0.5, 1, 3}.  m = 300 segments of at most 300 observations keep the numpy side at about a second per case.
"""
import functools
import os
import re

import numpy as np
import pytest

import als_ref as R
import lowrankmodels.jl_amd as L
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.als import check_model

pytestmark = pytest.mark.gpu
N = 257
CHUNK = 32                      # ALS_CHUNK, the kernel's staging chunk
KS = (1, 5, 20, 32, 64)
GAMMAS = (0.0, 0.1, 2.5)
SCALES = (0.5, 1.0, 3.0)
EPS = 2.0 ** -52


def hip():
    return _capi.hip_api()


def test_the_chunk_named_here_is_the_kernels():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "lowrankmodels.jl_amd", "csrc", "glrm_als.hpp")).read()
    assert int(re.search(r"constexpr int ALS_CHUNK = (\d+);", txt).group(1)) == CHUNK


def pool(k):
    return sorted({0, 1, k - 1, k, k + 1, 63, 64, 65, 100, 300, 2 * CHUNK + 1})


@functools.lru_cache(maxsize=None)
def problem(k, side, nseg=300, long_one=0):
    """Seeded, built once per shape and shared (nothing writes to it).  The SOLVED side has ``nseg`` segments with the lengths above over N
    opposing vectors; side 1 is the same recipe with rows and columns exchanged.  -> (ProblemArrays, X0, Y0, segment lengths)"""
    rng = np.random.default_rng(9000 + 10 * k + side)
    lens = rng.choice(pool(k), size=nseg)
    lens[: len(pool(k))] = pool(k)
    rank1 = len(pool(k))                                             # this segment repeats one index
    lens[rank1] = k + 3
    if long_one:
        lens[rank1 + 1] = long_one
    S, O_ = [], []
    for s, l in enumerate(lens):
        o = rng.permutation(N)[: min(l, N)]
        if l > N:
            o = np.concatenate([o, rng.integers(0, N, l - N)])
        if s == rank1:
            o = np.full(l, 17)
        S.append(np.full(l, s)); O_.append(np.sort(o))
    S, O_ = np.concatenate(S).astype(np.int64), np.concatenate(O_).astype(np.int64)
    own0, opp0 = rng.standard_normal((k, nseg)), rng.standard_normal((k, N))
    seg_regs = [L.QuadReg(g) if g > 0 else L.ZeroReg() for g in rng.choice(GAMMAS, size=nseg)]
    seg_regs[rank1] = L.ZeroReg()
    if side == 0:
        m, n, I, J, X0, Y0 = nseg, N, S, O_, own0, opp0
        rx, ry = seg_regs, L.QuadReg(0.1)
    else:
        m, n, I, J, X0, Y0 = N, nseg, O_, S, opp0, own0
        rx, ry = L.QuadReg(0.1), seg_regs
    A = X0.T @ Y0 + 0.1 * rng.standard_normal((m, n))
    losses = [L.QuadLoss(s) for s in rng.choice(SCALES, size=n)]
    g = L.GLRM(A, losses, rx, ry, k, obs=(I, J), X=X0, Y=Y0)
    X0, Y0 = np.asfortranarray(X0), np.asfortranarray(Y0)
    for a in (X0, Y0):
        a.setflags(write=False)
    return g.problem_arrays(), X0, Y0, lens


@functools.lru_cache(maxsize=None)
def reference(k, side, long_one=0):
    pa, X0, Y0, lens = problem(k, side, long_one=long_one)
    new, status = R.solve_side(pa, side, X0, Y0)
    new = np.asfortranarray(new)
    new.setflags(write=False)
    status.setflags(write=False)
    return new, status


def factors(api, h, pa):
    X, Y = np.zeros((pa.k, pa.m), order="F"), np.zeros((pa.k, pa.n), order="F")
    api.get_factors(h, X, Y)
    return X, Y


def solve_on_device(pa, X0, Y0, side, **create_kw):
    """als_solve(h, side) from (X0, Y0), then ONE further half-step of the side (stored state) -> dict"""
    api = hip()
    h = api.create(pa, **create_kw)
    try:
        api.set_factors(h, X0, Y0)
        api.reset_stepsizes(h, 1.0)
        api.als_solve(h, side)
        nseg = pa.m if side == 0 else pa.n
        info = api.als_info(h, side, nseg=nseg)
        X, Y = factors(api, h, pa)
        st = api.kernel_stats(h)
        (api.step_x if side == 0 else api.step_y)(h, 0.01)
        X2, Y2 = factors(api, h, pa)
        st2 = api.kernel_stats(h)
    finally:
        api.destroy(h)
    return dict(X=X, Y=Y, info=info, stats=st, X2=X2, Y2=Y2, stats2=st2)


def fresh_step(pa, X, Y, side, **create_kw):
    """The same further half-step on a fresh handle given the same factors."""
    api = hip()
    h = api.create(pa, **create_kw)
    try:
        api.set_factors(h, X, Y)
        api.reset_stepsizes(h, 1.0)
        (api.step_x if side == 0 else api.step_y)(h, 0.01)
        X2, Y2 = factors(api, h, pa)
        st2 = api.kernel_stats(h)
    finally:
        api.destroy(h)
    return X2, Y2, st2


COUNTERS = ("trials_x", "trials_y", "accepts_x", "accepts_y", "launches_x", "launches_y")


def check_side(k, side, long_one=0):
    pa, X0, Y0, lens = problem(k, side, long_one=long_one)
    ref, status = reference(k, side, long_one)
    got = solve_on_device(pa, X0, Y0, side)
    own, opp, own0, opp0 = (got["X"], got["Y"], X0, Y0) if side == 0 else (got["Y"], got["X"], Y0, X0)
    bad = np.flatnonzero(np.any(own != ref, axis=0) | (got["info"]["status"] != status))
    assert bad.size == 0, ("segments", bad[:12], "lengths", lens[bad[:12]], "status", got["info"]["status"][bad[:12]], status[bad[:12]])
    assert own.tobytes() == ref.tobytes()
    assert opp.tobytes() == opp0.tobytes()                           # the opposing factor is not written
    want = R.counts(status)
    nseg = len(lens)
    assert {c: got["info"][c] for c in want} == want and sum(want.values()) == nseg, (got["info"], want)
    gam = R.gammas(pa.rx if side == 0 else pa.ry, nseg)
    assert want["kept_short"] == int(np.sum((gam == 0) & (lens < k))) and want["solved"] > 0
    assert want["kept_pivot"] == (1 if k > 1 else 0) and want["kept_short"] > 0
    kept = status != R.SOLVED
    assert own[:, kept].tobytes() == np.asfortranarray(own0[:, kept]).tobytes()    # every bit of a kept point
    assert np.all(own[:, (status == R.SOLVED) & (lens == 0)] == 0.0)               # empty, penalised: exactly 0
    # the step sizes, the counters and the objective vectors: untouched by the solve -- one further half-step on this handle is the
    # half-step of a fresh handle given the same factors
    assert all(got["stats"][c] == 0 for c in COUNTERS), got["stats"]
    X2, Y2, st2 = fresh_step(pa, got["X"], got["Y"], side)
    assert got["X2"].tobytes() == X2.tobytes() and got["Y2"].tobytes() == Y2.tobytes()
    assert all(got["stats2"][c] == st2[c] for c in COUNTERS), (got["stats2"], st2)
    return got


@pytest.mark.parametrize("k", KS)
def test_rows_equal_the_restatement_bit_for_bit(k):
    check_side(k, 0)


@pytest.mark.parametrize("k", KS)
def test_columns_equal_the_restatement_bit_for_bit(k):
    """One column of 5 000 observations among the short ones: the same kernel, one workgroup."""
    check_side(k, 1, long_one=5000)


def test_the_padding_of_a_rank_20_factor_stays_zero():
    import torch
    pa, X0, Y0, lens = problem(20, 0)
    api = hip()
    h = api.create(pa)
    try:
        ld = api.factor_ld(h)
        dX, dY = torch.zeros(ld * pa.m, dtype=torch.float64, device="cuda"), torch.zeros(ld * pa.n, dtype=torch.float64, device="cuda")
        oc, orow = torch.zeros(pa.n, dtype=torch.float64, device="cuda"), torch.zeros(pa.m, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        api.bind_buffers(h, dX.data_ptr(), dY.data_ptr(), oc.data_ptr(), orow.data_ptr())
        api.set_factors(h, X0, Y0)
        api.als_solve(h, 0)
        api.synchronize(h)
        raw = dX.cpu().numpy().reshape(pa.m, ld)
        assert ld == 32 and not raw[:, 20:].any()
        assert np.asfortranarray(raw[:, :20].T).tobytes() == reference(20, 0)[0].tobytes()
    finally:
        api.destroy(h)


@pytest.mark.parametrize("tiled", [1, 2])
def test_the_family_of_the_handle_changes_no_bit(tiled):
    """tiled = 1: gather sweeps only; tiled = 2: the LDS-tiled sweeps wherever the lists allow (they do: ascending lists are in tile order,
    so the private copy such a handle may hold has the caller's order).  The solve reads the lists the handle holds and nothing of a family."""
    pa, X0, Y0, lens = problem(32, 0)
    got = solve_on_device(pa, X0, Y0, 0, tiled=tiled)
    assert got["X"].tobytes() == reference(32, 0)[0].tobytes()
    assert np.array_equal(got["info"]["status"], reference(32, 0)[1])


@functools.lru_cache(maxsize=None)
def chained_model():
    rng = np.random.default_rng(77)
    k, m = 20, 80
    lens = rng.choice([25, 40, 63, 64, 65, 100], size=m)
    I = np.concatenate([np.full(l, i) for i, l in enumerate(lens)]).astype(np.int64)
    J = np.concatenate([np.sort(rng.permutation(N)[:l]) for l in lens]).astype(np.int64)
    X0, Y0 = rng.standard_normal((k, m)), rng.standard_normal((k, N))
    A = (rng.standard_normal((m, 3)) @ rng.standard_normal((3, N))) + 0.05 * rng.standard_normal((m, N))
    losses = [L.QuadLoss(s) for s in rng.choice(SCALES, size=N)]
    ry = [L.QuadReg(g) if g > 0 else L.ZeroReg() for g in rng.choice(GAMMAS, size=N)]
    return A, losses, ry, k, (I, J), X0, Y0


def test_three_chained_iterations_equal_the_restatement_through_both_doors():
    A, losses, ry, k, obs, X0, Y0 = chained_model()
    g = L.GLRM(A, losses, L.QuadReg(0.1), ry, k, obs=obs, X=X0, Y=Y0)
    pa = g.problem_arrays()
    Xr, Yr = np.asfortranarray(X0), np.asfortranarray(Y0)
    infos = []
    for _ in range(3):
        Xr, sx = R.solve_side(pa, 0, Xr, Yr)
        Yr, sy = R.solve_side(pa, 1, Xr, Yr)
        infos = [R.counts(sx), R.counts(sy)]
    assert infos[1]["kept_short"] > 0 and infos[1]["solved"] > 0       # columns of fewer than k observations under ZeroReg are kept
    # the raw entry points
    api = hip()
    h = api.create(pa)
    try:
        api.set_factors(h, np.asfortranarray(X0), np.asfortranarray(Y0))
        for _ in range(3):
            api.als_solve(h, 0)
            api.als_solve(h, 1)
        X, Y = factors(api, h, pa)
        assert [api.als_info(h, 0), api.als_info(h, 1)] == infos
    finally:
        api.destroy(h)
    assert X.tobytes() == np.asfortranarray(Xr).tobytes() and Y.tobytes() == np.asfortranarray(Yr).tobytes()
    # fit(glrm, AlsParams(max_iter=3))
    Xt, Yf, ch = L.fit(g, L.AlsParams(max_iter=3), verbose=False)
    try:
        assert np.asfortranarray(Xt.T).tobytes() == np.asfortranarray(Xr).tobytes() and np.asfortranarray(Yf).tobytes() == np.asfortranarray(Yr).tobytes()
        obj = np.array(ch.objective)
        nnz = len(obs[0])
        print("objective history:", obj)
        assert len(obj) == 4 and np.all(obj[1:] <= obj[:-1] * (1 + nnz * EPS)), obj    # an exact half-step cannot raise the full objective
        assert g._als_info == {0: infos[0], 1: infos[1]}
        assert obj[-1] == pytest.approx(L.objective(g, Xr, Yr), rel=1e-12)             # the FULL objective, row penalties included
    finally:
        g.close()


def test_transform_exact_is_one_solve_of_the_new_rows_and_reproduces_a_noiseless_model():
    """inverse_transform of the exact embedding against the noiseless A_new = X_t' Y, entry by entry, to the bound that follows from the
    backward-error bound of tests/test_als.py: with M = Y Y' (ZeroReg, unit scales, every column observed) and r the residual bound of the
    row's solve (als_ref's formula at the computed x), |Y' x - a| <= |Y' M^-1| r + (|P| + I) d + e, where P = Y' M^-1 Y, d = (k + 1) 2^-52
    |x_t|' |Y| is the rounding of the product that made A_new (so A_new is not exactly of rank 3) and e = (k + 1) 2^-52 |x|' |Y| the rounding
    of inverse_transform's own product.  Evaluated in np.longdouble."""
    rng = np.random.default_rng(31)
    k, n, m_new = 3, 40, 12
    Y = rng.standard_normal((k, n))
    fitted = L.GLRM(rng.standard_normal((6, k)) @ Y, L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), k, X=rng.standard_normal((k, 6)), Y=Y)
    Xt = rng.standard_normal((k, m_new))
    A_new = Xt.T @ Y
    X0 = rng.standard_normal((k, m_new))
    Xn, ch = L.transform(fitted, A_new, exact=True, X0=X0)
    new = L.GLRM(A_new, L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), k, X=X0, Y=Y)
    pa = new.problem_arrays()
    api = hip()
    h = api.create(pa)
    try:
        api.set_factors(h, np.asfortranarray(X0), np.asfortranarray(Y))
        api.als_solve(h, 0)
        assert api.als_info(h, 0) == dict(solved=m_new, kept_short=0, kept_pivot=0)
        X1 = factors(api, h, pa)[0]
    finally:
        api.destroy(h)
    assert Xn.tobytes() == X1.tobytes() == np.asfortranarray(R.solve_side(pa, 0, np.asfortranarray(X0), np.asfortranarray(Y))[0]).tobytes()
    assert len(ch.objective) == 2 and ch.objective[1] < ch.objective[0]
    ld = np.longdouble
    Yl = Y.astype(ld)
    Minv = np.linalg.inv((Yl @ Yl.T).astype(np.float64)).astype(ld)   # k = 3, well conditioned: the inverse only weights the bound
    YtMinv = np.abs(Yl.T @ Minv)
    P = np.abs(Yl.T @ Minv @ Yl)
    rec = L.inverse_transform(fitted, Xn)
    worst = 0.0
    for i in range(m_new):
        x = Xn[:, i].astype(ld)
        assert R.residual_ratio(Y.T, A_new[i], np.ones(n), 0.0, Xn[:, i]) <= 1.0
        Gabs = np.abs(Yl) @ np.abs(Yl.T)
        babs = np.abs(Yl) @ np.abs(A_new[i].astype(ld))
        r = ld((n + 3 * k + 2) * EPS) * (k * (Gabs @ np.abs(x)) + babs)
        d = ld((k + 1) * EPS) * (np.abs(Xt[:, i].astype(ld)) @ np.abs(Yl))
        e = ld((k + 1) * EPS) * (np.abs(x) @ np.abs(Yl))
        bound = YtMinv @ r + (P + np.eye(n)) @ d + e
        err = np.abs(rec[i].astype(ld) - A_new[i].astype(ld))
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (i, float(np.max(err / bound)))
    print(f"inverse_transform: worst error / bound = {worst:.3g}")


# ------------------------------------------------------------------ refusals

def refused(call, code, *words):
    with pytest.raises(_capi.GLRMError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, ei.value.message)
    for w in words:
        assert w in ei.value.message, (w, ei.value.message)
    return ei.value.message


def host_words(g, sides):
    with pytest.raises(_capi.GLRMError) as ei:
        check_model(g, sides)
    return ei.value.message


def test_refusals_name_what_was_found_and_leave_the_factors_alone():
    api = hip()
    rng = np.random.default_rng(5)
    m, n = 24, 18
    A = rng.standard_normal((m, n))
    obs = np.nonzero(rng.random((m, n)) < 0.6)
    q = L.QuadReg(0.1)
    HDR = "include/glrm_hip_als.h"

    def model(losses=None, rx=q, ry=q, k=4, **kw):
        return L.GLRM(A, L.QuadLoss() if losses is None else losses, rx, ry, k, obs=obs, rng=np.random.default_rng(1), **kw)

    def on_handle(g, body, vec=False, **create_kw):
        from lowrankmodels.jl_amd.fit import install_regularizers
        pa = g.problem_arrays()
        h = api.create(pa, **create_kw)
        try:
            if vec:
                install_regularizers(api, h, g)
            X, Y = np.asfortranarray(g.X), np.asfortranarray(g.Y)
            if create_kw.get("storage"):                                                 # a float handle holds float-representable factors
                X, Y = (np.asfortranarray(F.astype(np.float32).astype(np.float64)) for F in (X, Y))
            api.set_factors(h, X, Y)
            body(h)
            X1, Y1 = np.zeros_like(X), np.zeros_like(Y)
            api.get_factors(h, X1, Y1)
            assert X1.tobytes() == X.tobytes() and Y1.tobytes() == Y.tobytes()          # nothing written
        finally:
            api.destroy(h)

    # arguments and order of calls
    def arguments(h):
        refused(lambda: api.als_solve(h, 2), _capi.ERR_INVALID, "side must be 0", "got 2")
        refused(lambda: api.als_solve(h, -1), _capi.ERR_INVALID, "side")
        refused(lambda: api.als_info(h, 0), _capi.ERR_INVALID, "has not run on side 0")
        refused(lambda: api.als_info(h, 3), _capi.ERR_INVALID, "side")
    on_handle(model(), arguments)
    refused(lambda: api.als_solve(None, 0), _capi.ERR_INVALID, "NULL handle")
    g = model()
    h = api.create(g.problem_arrays(), defer=True)
    try:
        refused(lambda: api.als_solve(h, 0), _capi.ERR_INVALID, "glrm_hip_finalize")
        refused(lambda: api.als_info(h, 0), _capi.ERR_INVALID, "glrm_hip_finalize")
    finally:
        api.destroy(h)
    h = api.create(g.problem_arrays())
    try:
        refused(lambda: api.als_solve(h, 0), _capi.ERR_INVALID, "no factors on the device yet")
    finally:
        api.destroy(h)

    # the model: the engine's words are the host's (lowrankmodels.jl_amd/als.py: check_model)
    def same_words(g, side, *words, sides=None, **kw):
        def body(h):
            msg = refused(lambda: api.als_solve(h, side), _capi.ERR_UNSUPPORTED, HDR, *words)
            assert msg == host_words(g, (side,) if sides is None else sides), (msg, host_words(g, (side,)))
        on_handle(g, body, **kw)
    same_words(model(losses=L.HuberLoss()), 0, "column 0 has loss kind 2", "needs QuadLoss")
    same_words(model(losses=[L.QuadLoss()] * 7 + [L.L1Loss()] + [L.QuadLoss()] * 10), 1, "column 7 has loss kind 1")
    same_words(model(rx=L.NonNegConstraint()), 0, "rx[0] has regularizer kind 3, wrap 0")
    same_words(model(ry=[q] * 5 + [L.OneReg(0.3)] + [q] * 12), 1, "ry[5] has regularizer kind 2")
    same_words(model(rx=L.QuadReg(-0.5)), 0, "rx[0] is QuadReg with scale -0.5")
    same_words(model(k=65), 0, "rank k = 65 is above GLRM_ALS_MAX_K = 64")
    same_words(model(offset=True), 0, "rx[0] has regularizer kind 1, wrap 1")
    same_words(model(rx=L.QuadConstraint(2.0)), 0, "rx[0] has regularizer kind 5")
    same_words(model(ry=L.lastentry_unpenalized(L.QuadReg(0.1))), 0, "general sweeps")   # the other side's wrapper: the handle is on the general sweeps
    # the other side's regularizer is not looked at
    on_handle(model(rx=L.NonNegConstraint()), lambda h: refused(lambda: api.als_solve(h, 0), _capi.ERR_UNSUPPORTED, "rx[0]"))
    g = model(rx=L.NonNegConstraint())
    h = api.create(g.problem_arrays())
    try:
        api.set_factors(h, np.asfortranarray(g.X), np.asfortranarray(g.Y))
        api.als_solve(h, 1)                                                              # columns: ry is a QuadReg
        assert api.als_info(h, 1)["solved"] == n
    finally:
        api.destroy(h)
    # a regularizer that carries a vector
    gv = model()
    gv.ry = _capi.TrackedList(L.fixed_latent_features(r, gv.Y[:2, j]) for j, r in enumerate(gv.ry))
    on_handle(gv, lambda h: refused(lambda: api.als_solve(h, 1), _capi.ERR_UNSUPPORTED, HDR, "ry[0]"), vec=True)
    refused(lambda: check_model(gv), _capi.ERR_UNSUPPORTED, HDR, "ry[0]")

    # the handle
    on_handle(model(), lambda h: refused(lambda: api.als_solve(h, 0), _capi.ERR_UNSUPPORTED, HDR, "storage = f32"), storage=1)
    full = L.GLRM(A, L.QuadLoss(), q, q, 12, rng=np.random.default_rng(1))
    assert full.dense_eligible()
    h = api.create(full.problem_arrays(dense=True))
    try:
        api.set_factors(h, np.asfortranarray(full.X), np.asfortranarray(full.Y))
        refused(lambda: api.als_solve(h, 0), _capi.ERR_UNSUPPORTED, HDR, "dense_A")
    finally:
        api.destroy(h)
    g = model()
    h = api.create(g.problem_arrays(rows=(0, m // 2)), defer=True)
    try:
        api.finalize(h, api.signature(h))
        api.set_factors(h, np.asfortranarray(g.X), np.asfortranarray(g.Y))
        refused(lambda: api.als_solve(h, 0), _capi.ERR_UNSUPPORTED, HDR, "this one is a shard", f"rows [0, {m // 2}) of {m}")
    finally:
        api.destroy(h)
