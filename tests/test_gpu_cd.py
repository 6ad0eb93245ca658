"""-m gpu: glrm_hip_cd_solve / glrm_hip_cd_info (include/glrm_hip_cd.h; csrc/glrm_cd.hip, csrc/glrm_cd.hpp) and the driver over them.

The contract is bit for bit: the header fixes every operation and its order, tests/cd_ref.py restates it in numpy (and tests/test_cd.py
holds that restatement to brute force), and every comparison below is ``tobytes`` equality -- the same operations in the same order, so
there is no allowance.  The status bits and the sweeps run of every segment are compared as well, and the counts are asserted one by one
against properties of the reference, so nothing passes by keeping everything.

Problems follow the recipe of tests/test_gpu_als.py: N = 257 opposing vectors, lists in ascending index order, seeded; 300 segments with
lengths from {0, 1, k-1, k, k+1, 63, 64, 65, 100, 300}, every one present; one segment repeats ONE index k + 3 times (rank 1); one segment
hits only the opposing vector whose component 2 is 0.0 (k > 2: G_22 = 0, a skipped coordinate); columns get one list of 5 000
observations.  Per-segment regularizers from ZeroReg, QuadReg, OneReg and NonNegConstraint with scales from {0.1, 2.5}, per-column loss
scales from {0.5, 1, 3}.  The start is standard normal, so every NonNegConstraint segment is projected first.
"""
import functools

import numpy as np
import pytest

import cd_ref as R
import lowrankmodels.jl_amd as L
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.cd import check_model

pytestmark = pytest.mark.gpu
N = 257
ZERO_VEC, RANK1_VEC = 19, 17    # the opposing vector with component 2 equal to 0.0; the one the rank-1 segment repeats
KS = (1, 5, 20, 32, 64)
SWEEPS = (1, 3)
REG_SCALES = (0.1, 2.5)
SCALES = (0.5, 1.0, 3.0)


def hip():
    return _capi.hip_api()


def pool(k):
    return sorted({0, 1, k - 1, k, k + 1, 63, 64, 65, 100, 300})


def draw_reg(rng):
    kind, scale = int(rng.integers(0, 4)), float(rng.choice(REG_SCALES))
    return (L.ZeroReg(), L.QuadReg(scale), L.OneReg(scale), L.NonNegConstraint())[kind]


@functools.lru_cache(maxsize=None)
def problem(k, side, nseg=300, long_one=0, seed=0):
    """Seeded, built once per shape and shared (nothing writes to it).  The SOLVED side has ``nseg`` segments with the lengths above over N
    opposing vectors; side 1 is the same recipe with rows and columns exchanged.  -> (ProblemArrays, X0, Y0, segment lengths, the index
    of the segment on the zero-component vector)"""
    rng = np.random.default_rng(9500 + 1000 * seed + 10 * k + side)
    lens = rng.choice(pool(k), size=nseg)
    lens[: len(pool(k))] = pool(k)
    rank1 = len(pool(k))                                             # this segment repeats one index
    zero_seg = rank1 + 1                                             # this one sees only the zero-component vector
    lens[rank1] = lens[zero_seg] = k + 3
    if long_one:
        lens[zero_seg + 1] = long_one
    S, O_ = [], []
    for s, l in enumerate(lens):
        o = rng.permutation(N)[: min(l, N)]
        if l > N:
            o = np.concatenate([o, rng.integers(0, N, l - N)])
        if s == rank1:
            o = np.full(l, RANK1_VEC)
        if s == zero_seg:
            o = np.full(l, ZERO_VEC)
        S.append(np.full(l, s)); O_.append(np.sort(o))
    S, O_ = np.concatenate(S).astype(np.int64), np.concatenate(O_).astype(np.int64)
    own0, opp0 = rng.standard_normal((k, nseg)), rng.standard_normal((k, N))
    if k > 2:
        opp0[2, ZERO_VEC] = 0.0
    seg_regs = [draw_reg(rng) for _ in range(nseg)]
    seg_regs[zero_seg] = L.NonNegConstraint() if side == 0 else L.OneReg(2.5)
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
    return g.problem_arrays(), X0, Y0, lens, zero_seg


@functools.lru_cache(maxsize=None)
def references(k, side, long_one=0, seed=0, sweeps_list=SWEEPS):
    """{sweeps: (factor, status, sweeps_run)} of the restatement, each segment's Gram matrix formed once; computed once and left unchanged."""
    pa, X0, Y0, lens, _ = problem(k, side, long_one=long_one, seed=seed)
    res = R.solve_side_each(pa, side, X0, Y0, sweeps_list)
    out = {}
    for sw, (new, status, run) in res.items():
        new = np.asfortranarray(new)
        for a in (new, status, run):
            a.setflags(write=False)
        out[sw] = (new, status, run)
    return out


def factors(api, h, pa):
    X, Y = np.zeros((pa.k, pa.m), order="F"), np.zeros((pa.k, pa.n), order="F")
    api.get_factors(h, X, Y)
    return X, Y


def solve_on_device(pa, X0, Y0, side, sweeps_list, **create_kw):
    """For every sweep count, on ONE handle: cd_solve(h, side, sweeps) from (X0, Y0); after the last one ONE further half-step of the side
    (stored state) -> {sweeps: dict}, dict of the further step"""
    api = hip()
    h = api.create(pa, **create_kw)
    out = {}
    try:
        nseg = pa.m if side == 0 else pa.n
        for sw in sweeps_list:
            api.set_factors(h, X0, Y0)
            api.reset_stepsizes(h, 1.0)
            api.cd_solve(h, side, sw)
            info = api.cd_info(h, side, nseg=nseg)
            X, Y = factors(api, h, pa)
            out[sw] = dict(X=X, Y=Y, info=info, stats=api.kernel_stats(h))
        (api.step_x if side == 0 else api.step_y)(h, 0.01)
        X2, Y2 = factors(api, h, pa)
        further = dict(X2=X2, Y2=Y2, stats2=api.kernel_stats(h))
    finally:
        api.destroy(h)
    return out, further


def fresh_step(pa, X, Y, side):
    """The same further half-step on a fresh handle given the same factors."""
    api = hip()
    h = api.create(pa)
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
    pa, X0, Y0, lens, zero_seg = problem(k, side, long_one=long_one)
    refs = references(k, side, long_one)
    got_all, further = solve_on_device(pa, X0, Y0, side, SWEEPS)
    nseg = len(lens)
    kind, scale = R.kinds_and_scales(pa.rx if side == 0 else pa.ry, nseg)
    for sw in SWEEPS:
        ref, status, run = refs[sw]
        got = got_all[sw]
        own, opp, opp0 = (got["X"], got["Y"], Y0) if side == 0 else (got["Y"], got["X"], X0)
        info = got["info"]
        bad = np.flatnonzero(np.any(own != ref, axis=0) | (info["status"] != status) | (info["sweeps_run"] != run))
        assert bad.size == 0, (sw, "segments", bad[:12], "lengths", lens[bad[:12]], "kinds", kind[bad[:12]], "status", info["status"][bad[:12]], status[bad[:12]],
                               "sweeps", info["sweeps_run"][bad[:12]], run[bad[:12]])
        assert own.tobytes() == ref.tobytes()
        assert info["status"].tobytes() == status.tobytes() and info["sweeps_run"].tobytes() == run.tobytes()
        assert opp.tobytes() == opp0.tobytes()                       # the opposing factor is not written
        # the counts, one by one, and what the REFERENCE must show for them to mean something
        want = R.counts(status, run)
        assert info["converged"] == want["converged"] and info["skipped"] == want["skipped"] and info["sweeps_total"] == want["sweeps_total"], (info, want)
        assert want["skipped"] > 0 and nseg <= want["sweeps_total"] <= sw * nseg and np.all(run >= 1)
        empty_kept = (lens == 0) & np.isin(kind, (R.ZERO, R.NONNEG))
        assert empty_kept.any() and np.all(status[empty_kept] & R.SKIPPED)
        if k > 2:
            assert status[zero_seg] & R.SKIPPED
        if sw > 1:
            assert want["sweeps_total"] < sw * nseg and want["converged"] > 0      # some segment stopped early
        assert np.any(ref != (X0 if side == 0 else Y0)[:, :nseg])
        nn = kind == R.NONNEG
        assert nn.any() and np.all(own[:, nn] >= 0) and np.any((X0 if side == 0 else Y0)[:, nn] < 0)
        assert np.all(own[:, (lens == 0) & np.isin(kind, (R.QUAD, R.ONE))] == 0.0)   # empty, penalised: exactly 0
        assert all(got["stats"][c] == 0 for c in COUNTERS), got["stats"]
    # the step sizes, the counters and the objective vectors: untouched by the solves -- one further half-step on this handle is the
    # half-step of a fresh handle given the same factors
    last = got_all[SWEEPS[-1]]
    X2, Y2, st2 = fresh_step(pa, last["X"], last["Y"], side)
    assert further["X2"].tobytes() == X2.tobytes() and further["Y2"].tobytes() == Y2.tobytes()
    assert all(further["stats2"][c] == st2[c] for c in COUNTERS), (further["stats2"], st2)


@pytest.mark.parametrize("k", KS)
def test_rows_equal_the_restatement_bit_for_bit(k):
    check_side(k, 0)


@pytest.mark.parametrize("k", KS)
def test_columns_equal_the_restatement_bit_for_bit(k):
    """One column of 5 000 observations among the short ones: the same kernel, one workgroup."""
    check_side(k, 1, long_one=5000)


EARLY = dict(k=5, side=0, seed=0, sweeps_list=(64,))


def test_a_segment_that_stops_changing_leaves_early_and_one_that_cycles_does_not():
    """k = 5, 64 sweeps.  The restatement alone shows both on this seed (asserted first): segments that carry CONVERGED after fewer than 64
    sweeps, and segments that run all 64 (a singular G under ZeroReg creeps along its null space; others cycle in the last bit)."""
    pa, X0, Y0, lens, _ = problem(EARLY["k"], EARLY["side"], seed=EARLY["seed"])
    ref, status, run = references(**EARLY)[64]
    early = (status & R.CONVERGED != 0) & (run < 64)
    late = (status & R.CONVERGED == 0)
    assert early.sum() >= 10 and late.sum() >= 10 and np.all(run[late] == 64), (early.sum(), late.sum())
    got = solve_on_device(pa, X0, Y0, 0, (64,))[0][64]
    assert got["X"].tobytes() == ref.tobytes()
    assert got["info"]["status"].tobytes() == status.tobytes() and got["info"]["sweeps_run"].tobytes() == run.tobytes()
    assert got["info"]["converged"] == int((status & R.CONVERGED != 0).sum()) and got["info"]["sweeps_total"] == int(run.sum())


def test_the_padding_of_a_rank_20_factor_stays_zero():
    import torch
    pa, X0, Y0, lens, _ = problem(20, 0)
    api = hip()
    h = api.create(pa)
    try:
        ld = api.factor_ld(h)
        dX, dY = torch.zeros(ld * pa.m, dtype=torch.float64, device="cuda"), torch.zeros(ld * pa.n, dtype=torch.float64, device="cuda")
        oc, orow = torch.zeros(pa.n, dtype=torch.float64, device="cuda"), torch.zeros(pa.m, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        api.bind_buffers(h, dX.data_ptr(), dY.data_ptr(), oc.data_ptr(), orow.data_ptr())
        api.set_factors(h, X0, Y0)
        api.cd_solve(h, 0, 3)
        api.synchronize(h)
        raw = dX.cpu().numpy().reshape(pa.m, ld)
        assert ld == 32 and not raw[:, 20:].any()
        assert np.asfortranarray(raw[:, :20].T).tobytes() == references(20, 0)[3][0].tobytes()
    finally:
        api.destroy(h)


@pytest.mark.parametrize("tiled", [1, 2])
def test_the_family_of_the_handle_changes_no_bit(tiled):
    """tiled = 1: gather sweeps only; tiled = 2: the LDS-tiled sweeps wherever the lists allow.  The solve reads the lists the handle holds
    and nothing of a family."""
    pa, X0, Y0, lens, _ = problem(32, 0)
    got = solve_on_device(pa, X0, Y0, 0, (3,), tiled=tiled)[0][3]
    ref, status, run = references(32, 0)[3]
    assert got["X"].tobytes() == ref.tobytes()
    assert np.array_equal(got["info"]["status"], status) and np.array_equal(got["info"]["sweeps_run"], run)


@functools.lru_cache(maxsize=None)
def driver_runs():
    """fit_b(CdParams(max_iter=3, abs_tol=0, rel_tol=0)) on the device and on the HostEngine, from the same start, run once
    -> ((X, Y, history, cd_info) of the device, the same of the host engine, the model's recipe)"""
    import oracle as O
    rng = np.random.default_rng(41)
    m, n, k = 60, 40, 4
    A = rng.random((m, k)) @ rng.random((k, n)) + 0.01 * rng.random((m, n))
    flat = np.sort(rng.permutation(m * n)[: m * n // 2])
    obs = (flat // n, flat % n)
    X0, Y0 = rng.standard_normal((k, m)), rng.random((k, n))           # negative entries in X: the first objective is infinite
    p = L.CdParams(max_iter=3, abs_tol=0, rel_tol=0)
    model = lambda X, Y: L.GLRM(A, L.QuadLoss(), L.NonNegConstraint(), [L.OneReg(0.1)] * 20 + [L.NonNegConstraint()] * 20, k, obs=obs, X=X, Y=Y)
    # the host engine adds the objective as the device's handle of this model does (the column view's order, glrm_hip_sum's)
    api = hip()
    h = api.create(model(X0.copy(), Y0.copy()).problem_arrays())
    try:
        order = api.sum_order(h, 1)
    finally:
        api.destroy(h)
    runs = []
    for engine in (None, R.HostEngine(O.oracle_api(), column_order=order)):
        g = model(X0.copy(), Y0.copy())
        try:
            X, Y, ch = L.fit_b(g, p, verbose=False) if engine is None else L.fit_b(g, p, engine=engine, verbose=False)
            runs.append((np.asfortranarray(X).copy(), np.asfortranarray(Y).copy(), np.array(ch.objective), g._cd_info))
        finally:
            g.close()
    return runs[0], runs[1], (model, X0, Y0, p)


def test_fit_with_cdparams_lands_on_the_factors_of_the_host_engine_run():
    (Xd, Yd, od, infod), (Xh, Yh, oh, infoh), (model, X0, Y0, p) = driver_runs()
    assert Xd.tobytes() == Xh.tobytes() and Yd.tobytes() == Yh.tobytes()
    assert infod == infoh and infod[0]["sweeps_total"] >= 60
    assert len(od) == 4 and od[0] == np.inf and np.all(np.isfinite(od[1:])) and np.all(np.diff(od[1:]) < 0)
    # every entry of the device's history is the full objective of the restatement's iterate, through the same entry points on a fresh handle
    from lowrankmodels.jl_amd.als import _Objective
    g = model(X0.copy(), Y0.copy())
    pa = g.problem_arrays()
    api = hip()
    h = api.create(pa)
    full = _Objective(api, h, -1, pa.m, pa.n)
    try:
        Xr, Yr = np.asfortranarray(X0), np.asfortranarray(Y0)
        for i in range(4):
            api.set_factors(h, Xr, Yr)
            assert np.float64(full()).tobytes() == od[i].tobytes(), i
            Xr = R.solve_side(pa, 0, Xr, Yr, p.sweeps)[0]
            Yr = R.solve_side(pa, 1, Xr, Yr, p.sweeps)[0]
    finally:
        full.close()
        api.destroy(h)


def test_the_history_of_the_device_fit_equals_the_host_engine_run():
    """The history of the device fit against the history of the HostEngine run, bit for bit.  The factors behind every entry are equal bit
    for bit (the test above), so this compares two evaluations of the full objective.  The CPU oracle's own col_losses and sum add in the
    reference's order and land one unit in the last place away from the device in one entry of four (measured: 0x1.d537859db2361p+3
    against 0x1.d537859db2362p+3), so the host engine is given the order the device's handle reports and adds as that engine does
    (cd_ref.engine_col_losses, cd_ref.engine_sum)."""
    (Xd, Yd, od, infod), (Xh, Yh, oh, infoh), _ = driver_runs()
    with np.errstate(invalid="ignore"):
        print("device:", [float(v).hex() for v in od], "host engine:", [float(v).hex() for v in oh], "relative difference:", np.abs(od - oh)[1:] / oh[1:])
    assert od.tobytes() == oh.tobytes()


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
    q, nn = L.QuadReg(0.1), L.NonNegConstraint()
    HDR = "include/glrm_hip_cd.h"

    def model(losses=None, rx=nn, ry=q, k=4, **kw):
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
        refused(lambda: api.cd_solve(h, 2, 4), _capi.ERR_INVALID, "side must be 0", "got 2")
        refused(lambda: api.cd_solve(h, -1, 4), _capi.ERR_INVALID, "side")
        refused(lambda: api.cd_solve(h, 0, 0), _capi.ERR_INVALID, "sweeps must be in [1, GLRM_CD_MAX_SWEEPS = 256], got 0")
        refused(lambda: api.cd_solve(h, 1, 257), _capi.ERR_INVALID, "got 257")
        refused(lambda: api.cd_info(h, 0), _capi.ERR_INVALID, "has not run on side 0")
        refused(lambda: api.cd_info(h, 3), _capi.ERR_INVALID, "side")
    on_handle(model(), arguments)
    refused(lambda: api.cd_solve(None, 0, 4), _capi.ERR_INVALID, "NULL handle")
    g = model()
    h = api.create(g.problem_arrays(), defer=True)
    try:
        refused(lambda: api.cd_solve(h, 0, 4), _capi.ERR_INVALID, "glrm_hip_finalize")
        refused(lambda: api.cd_info(h, 0), _capi.ERR_INVALID, "glrm_hip_finalize")
    finally:
        api.destroy(h)
    h = api.create(g.problem_arrays())
    try:
        refused(lambda: api.cd_solve(h, 0, 4), _capi.ERR_INVALID, "no factors on the device yet")
    finally:
        api.destroy(h)

    # the model: the engine's words are the host's (lowrankmodels.jl_amd/cd.py: check_model)
    def same_words(g, side, *words, **kw):
        def body(h):
            msg = refused(lambda: api.cd_solve(h, side, 4), _capi.ERR_UNSUPPORTED, HDR, *words)
            assert msg == host_words(g, (side,)), (msg, host_words(g, (side,)))
        on_handle(g, body, **kw)
    same_words(model(losses=L.HuberLoss()), 0, "column 0 has loss kind 2", "needs QuadLoss")
    same_words(model(losses=[L.QuadLoss()] * 7 + [L.L1Loss()] + [L.QuadLoss()] * 10), 1, "column 7 has loss kind 1")
    same_words(model(rx=L.UnitOneSparseConstraint()), 0, "rx[0] has regularizer kind 4, wrap 0")
    same_words(model(ry=[q] * 5 + [L.QuadConstraint(2.0)] + [q] * 12), 1, "ry[5] has regularizer kind 5")
    same_words(model(rx=L.QuadReg(-0.5)), 0, "rx[0] is QuadReg with scale -0.5")
    same_words(model(ry=L.OneReg(-2.0)), 1, "ry[0] is OneReg with scale -2")
    same_words(model(k=65), 0, "rank k = 65 is above GLRM_CD_MAX_K = 64")
    same_words(model(offset=True), 0, "rx[0] has regularizer kind 3, wrap 1")
    same_words(model(ry=L.lastentry_unpenalized(L.QuadReg(0.1))), 0, "general sweeps")   # the other side's wrapper: the handle is on the general sweeps
    # the other side's regularizer is not looked at
    g = model(ry=L.UnitOneSparseConstraint())
    on_handle(g, lambda h: refused(lambda: api.cd_solve(h, 1, 4), _capi.ERR_UNSUPPORTED, "ry[0]"))
    h = api.create(g.problem_arrays())
    try:
        api.set_factors(h, np.asfortranarray(g.X), np.asfortranarray(g.Y))
        api.cd_solve(h, 0, 4)                                                            # rows: rx is a NonNegConstraint
        info = api.cd_info(h, 0, nseg=m)
        assert info["sweeps_total"] == int(info["sweeps_run"].sum()) >= m
        refused(lambda: api.cd_info(h, 1), _capi.ERR_INVALID, "has not run on side 1")
    finally:
        api.destroy(h)
    # a regularizer that carries a vector
    gv = model()
    gv.ry = _capi.TrackedList(L.fixed_latent_features(r, gv.Y[:2, j]) for j, r in enumerate(gv.ry))
    on_handle(gv, lambda h: refused(lambda: api.cd_solve(h, 1, 4), _capi.ERR_UNSUPPORTED, HDR, "ry[0]"), vec=True)
    refused(lambda: check_model(gv), _capi.ERR_UNSUPPORTED, HDR, "ry[0]")

    # the handle
    on_handle(model(), lambda h: refused(lambda: api.cd_solve(h, 0, 4), _capi.ERR_UNSUPPORTED, HDR, "storage = f32"), storage=1)
    full = L.GLRM(A, L.QuadLoss(), q, q, 12, rng=np.random.default_rng(1))
    assert full.dense_eligible()
    h = api.create(full.problem_arrays(dense=True))
    try:
        api.set_factors(h, np.asfortranarray(full.X), np.asfortranarray(full.Y))
        refused(lambda: api.cd_solve(h, 0, 4), _capi.ERR_UNSUPPORTED, HDR, "dense_A")
    finally:
        api.destroy(h)
    g = model()
    h = api.create(g.problem_arrays(rows=(0, m // 2)), defer=True)
    try:
        api.finalize(h, api.signature(h))
        api.set_factors(h, np.asfortranarray(g.X), np.asfortranarray(g.Y))
        refused(lambda: api.cd_solve(h, 0, 4), _capi.ERR_UNSUPPORTED, HDR, "this one is a shard", f"rows [0, {m // 2}) of {m}")
    finally:
        api.destroy(h)
