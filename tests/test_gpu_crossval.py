"""-m gpu: glrm_hip_subset (device-side compaction of both Omega views) and the cross-validation drivers on the HIP engine
against the same drivers on the CPU oracle."""
import numpy as np
import pytest

import cases
import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd import _capi, crossval
from lowrankmodels.jl_amd.domains import pack_domains

pytestmark = pytest.mark.gpu
TOL = 1e-5


def hip():
    return _capi.hip_api()


def model(rng, m=300, n=80, k=4, density=0.5, losses=None, rx=None, ry=None):
    A = rng.standard_normal((m, k)) @ rng.standard_normal((k, n)) + 0.1 * rng.standard_normal((m, n))
    I, J = np.nonzero(rng.random((m, n)) < density)
    return L.GLRM(A, L.QuadLoss() if losses is None else losses, L.QuadReg(0.1) if rx is None else rx,
                  L.QuadReg(0.1) if ry is None else ry, k, obs=(I, J), X=rng.standard_normal((k, m)), Y=rng.standard_normal((k, n)))


@pytest.mark.parametrize("shape", [(300, 80, 0.5), (5000, 40, 0.9), (37, 11, 0.3), (20000, 64, 0.3)])
def test_subset_matches_oracle(shape):
    """Counts are exact; the child's objective and a short fit agree with the oracle's child built from the same tags."""
    m, n, dens = shape
    rng = np.random.default_rng(m + n)
    g = model(rng, m, n, 4, dens)
    rt = rng.integers(0, 4, len(g._colidx)).astype(np.uint8)
    ct = rng.integers(0, 4, len(g._rowidx)).astype(np.uint8)
    X, Y = np.asfortranarray(g.X), np.asfortranarray(g.Y)
    p = L.ProxGradParams(max_iter=6)
    res = {}
    for name, api in (("cpu", O.oracle_api()), ("hip", hip())):
        h = api.create(g.problem_arrays())
        out = []
        try:
            for match, inv in ((2, False), (2, True), (9, False), (9, True)):
                hc = api.subset(h, rt, ct, match, inv)
                try:
                    st = api.kernel_stats(hc)
                    Xc, Yc = X.copy(order="F"), Y.copy(order="F")
                    obj0 = api.objective(hc, Xc, Yc, True)
                    obj, _ = api.fit(hc, p, Xc, Yc)
                    out.append((st["nnz_rows"], st["nnz_cols"], obj0, obj, Xc, Yc))
                finally:
                    api.destroy(hc)
        finally:
            api.destroy(h)
        res[name] = out
    for c, g_ in zip(res["cpu"], res["hip"]):
        assert c[0] == g_[0] and c[1] == g_[1]
        assert g_[2] == pytest.approx(c[2], rel=1e-11)
        assert cases.rel_err(g_[3], c[3]) < TOL and cases.fro_err(g_[4], c[4]) < TOL and cases.fro_err(g_[5], c[5]) < TOL


def test_subset_child_outlives_parent_and_keeps_kernel_family():
    rng = np.random.default_rng(3)
    g = model(rng, 4000, 200, 8, 0.5)
    api = hip()
    h = api.create(g.problem_arrays(), tiled=2)
    tags_r = (rng.random(len(g._colidx)) < 0.2).astype(np.uint8)
    sp = crossval._Split(g)
    hc = api.subset(h, tags_r, tags_r[sp.perm], 1, True)
    api.destroy(h)
    try:
        assert api.kernel_stats(hc)["tiled"] == 3  # sorted lists stay sorted: the child runs the LDS-tiled sweeps too
        X, Y = np.asfortranarray(g.X), np.asfortranarray(g.Y)
        obj, _ = api.fit(hc, L.ProxGradParams(max_iter=5), X, Y)
        assert obj[-1] < obj[1]
    finally:
        api.destroy(hc)


def test_error_metric_of_a_subset_child_has_the_bits_of_a_fresh_handle():
    """error_metric takes the longest column from the handle's own record.  The parent's longest column spans two 65536-entry chunks and
    is not in the child, whose longest spans one chunk plus 17 entries: a child that carried its parent's length, or a fresh handle that
    measured wrong, would chunk differently or lose entries.  Inexact factors, so the sums depend on their order."""
    chunk = 65536
    m, lens = 2 * chunk, [2 * chunk, chunk + 17, 300, 0]
    rng = np.random.default_rng(17)
    A = rng.standard_normal((m, len(lens)))
    I = np.concatenate([np.sort(rng.choice(m, n_f, replace=False)) for n_f in lens])
    g = L.GLRM(A, L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 2, obs=(I, np.repeat(np.arange(len(lens)), lens)))
    X, Y, doms = np.asfortranarray(rng.standard_normal((2, m))), np.asfortranarray(rng.standard_normal((2, len(lens)))), pack_domains([L.RealDomain()] * len(lens))
    sp = crossval._Split(g)
    keep = (sp.J != 0).astype(np.uint8)
    fresh = L.GLRM(A, L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 2, obs=(sp.I[keep == 1], sp.J[keep == 1]))
    assert np.diff(fresh.problem_arrays().colptr).tolist() == [0] + lens[1:]
    api = hip()
    h = api.create(g.problem_arrays())
    try:
        hc = api.subset(h, keep, keep[sp.perm], 1, False)
    finally:
        api.destroy(h)
    hf = api.create(fresh.problem_arrays())
    try:
        assert api.error_metric(hc, X, Y, doms, False) == api.error_metric(hf, X, Y, doms, False)
        assert api.signature(hc).max_col_len == api.signature(hf).max_col_len == chunk + 17
    finally:
        api.destroy(hc)
        api.destroy(hf)


def test_subset_rejects_dense_parent():
    rng = np.random.default_rng(4)
    A = rng.standard_normal((64, 48))
    g = L.GLRM(A, L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 16)
    api = hip()
    h = api.create(g.problem_arrays(dense=True))
    try:
        with pytest.raises(_capi.GLRMError) as ei:
            api.subset(h, np.zeros(1, np.uint8), np.zeros(1, np.uint8), 0, False)
        assert ei.value.code == _capi.ERR_UNSUPPORTED
    finally:
        api.destroy(h)


def test_subset_of_shard_parents_is_deferred_until_the_host_finalizes(monkeypatch):
    """include/glrm_hip.h, glrm_hip_subset: the child of ONE SHARD is a shard of the subset problem and comes back in the
    GLRM_PROBLEM_DEFER_SETUP state -- step calls fail until the host has combined the children's signatures and finalized every child.
    Two shard parents -> subset -> combine -> finalize -> three outer iterations on shared buffers == the child of the single-shard
    parent, bit for bit.  A finalize that fails half way latches: the retry is refused, the handle can only be destroyed."""
    import torch
    rng = np.random.default_rng(11)
    g = model(rng, 2000, 96, 4, 0.4)
    pa = g.problem_arrays()
    rt = rng.integers(0, 3, len(g._colidx)).astype(np.uint8)
    ct = rng.integers(0, 3, len(g._rowidx)).astype(np.uint8)
    X0, Y0 = np.asfortranarray(g.X), np.asfortranarray(g.Y)
    p = L.ProxGradParams(max_iter=3, abs_tol=0.0, rel_tol=-1.0)
    api = hip()
    # the single-shard parent's child is ready on return
    h = api.create(pa)
    hc = api.subset(h, rt, ct, 1, True)
    api.destroy(h)
    try:
        X1, Y1 = X0.copy(order="F"), Y0.copy(order="F")
        obj1, _ = api.fit(hc, p, X1, Y1)
    finally:
        api.destroy(hc)
    rbs, cbs = [0, 900, 2000], [0, 40, 96]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    parents, kids = [], []
    try:
        for s in range(2):
            parents.append(api.create(cases.shard_of(pa, rbs[s], rbs[s + 1], cbs[s], cbs[s + 1]), stream=stream, defer=True))
        whole = _capi.CSignature.combine([api.signature(q) for q in parents])
        with pytest.raises(_capi.GLRMError):  # an un-finalized parent cannot be subset
            api.subset(parents[0], rt[: int(pa.rowptr[rbs[1]])], ct[: int(pa.colptr[cbs[1]])], 1, True)
        for q in parents:
            api.finalize(q, whole)
        for s in range(2):
            r0, r1, c0, c1 = int(pa.rowptr[rbs[s]]), int(pa.rowptr[rbs[s + 1]]), int(pa.colptr[cbs[s]]), int(pa.colptr[cbs[s + 1]])
            kids.append(api.subset(parents[s], rt[r0:r1], ct[c0:c1], 1, True))
        for q in parents:
            api.destroy(q)
        parents = []
        for c in kids:  # deferred: nothing steps before the combined finalize
            with pytest.raises(_capi.GLRMError) as ei:
                api.step_x(c, 0.01)
            assert ei.value.code == _capi.ERR_INVALID
        sub_whole = _capi.CSignature.combine([api.signature(c) for c in kids])
        assert sub_whole.nnz_rows == int((rt != 1).sum()) and sub_whole.nnz_cols == int((ct != 1).sum())
        for c in kids:
            api.finalize(c, sub_whole)
        with pytest.raises(_capi.GLRMError):  # once
            api.finalize(kids[0], sub_whole)
        ld = api.factor_ld(kids[0])
        dX, dY = torch.zeros(pa.m * ld, dtype=torch.float64, device=dev), torch.zeros(pa.n * ld, dtype=torch.float64, device=dev)
        dC, dR = torch.zeros(pa.n, dtype=torch.float64, device=dev), torch.zeros(pa.m, dtype=torch.float64, device=dev)
        for c in kids:
            api.bind_buffers(c, dX.data_ptr(), dY.data_ptr(), dC.data_ptr(), dR.data_ptr())
        api.set_factors(kids[0], X0, Y0)
        objs = []
        for c in kids:
            api.reset_stepsizes(c, p.stepsize)
        for _ in range(p.max_iter):
            for c in kids:
                api.step_x(c, p.min_stepsize)
            for c in kids:
                api.step_y(c, p.min_stepsize)
            objs.append(api.sum(kids[0], dC.data_ptr(), pa.n))
        X2, Y2 = np.zeros_like(X0), np.zeros_like(Y0)
        api.get_factors(kids[0], X2, Y2)
        assert np.array_equal(np.array(objs), obj1[1:]) and np.array_equal(X2, X1) and np.array_equal(Y2, Y1)
    finally:
        for q in parents + kids:
            api.destroy(q)
    # the latch: a set-up that failed half way refuses a second finalize.  The failure is injected through a hook that exists in the TEST BUILD
    # of the engine only (libglrm_hip_testing.so, csrc/glrm_testhooks.hip); the product library ignores the variable
    monkeypatch.setenv("GLRM_HIP_TEST_FAIL_FINALIZE", "1")
    q = api.create(cases.shard_of(pa, 0, 900, 0, 40), defer=True)
    try:
        api.finalize(q, whole)          # the product library: no such hook
    finally:
        api.destroy(q)
    api = _capi.hip_testing_api()
    q = api.create(cases.shard_of(pa, 0, 900, 0, 40), defer=True)
    try:
        with pytest.raises(_capi.GLRMError) as ei:
            api.finalize(q, whole)
        assert "injected" in str(ei.value)
        monkeypatch.delenv("GLRM_HIP_TEST_FAIL_FINALIZE")
        with pytest.raises(_capi.GLRMError) as ei:
            api.finalize(q, whole)
        assert ei.value.code == _capi.ERR_INVALID and "earlier glrm_hip_finalize" in str(ei.value)
        with pytest.raises(_capi.GLRMError):
            api.step_x(q, 0.01)
    finally:
        api.destroy(q)


@pytest.mark.parametrize("kind", ["quad", "categorical"])
def test_cross_validate_hip_vs_oracle(kind):
    rng = np.random.default_rng(11)
    if kind == "quad":
        g = model(rng)
    else:
        kwargs, _ = cases.build_multidim_case("mnl")
        g = L.GLRM(**kwargs)
    tags = rng.integers(0, 3, int(g._rowptr[-1]))
    p = L.ProxGradParams(max_iter=12)
    out = {}
    for name, api in (("cpu", O.oracle_api()), ("hip", hip())):
        tr, te, trg, teg = L.cross_validate(g, nfolds=3, params=p, verbose=False, groups=tags, engine=api)
        out[name] = (tr, te, [t.X.copy() for t in trg])
        for t in trg + teg:
            t.close()
        g.close()
    assert cases.rel_err(out["hip"][0], out["cpu"][0]) < TOL and cases.rel_err(out["hip"][1], out["cpu"][1]) < TOL
    for a, b in zip(out["hip"][2], out["cpu"][2]):
        assert cases.fro_err(a, b) < TOL


def test_regularization_path_and_cv_by_iter_hip_vs_oracle():
    rng = np.random.default_rng(12)
    draws = None
    res = {}
    for name, api in (("cpu", O.oracle_api()), ("hip", hip())):
        g = model(np.random.default_rng(12))
        draws = np.random.default_rng(99).random(int(g._rowptr[-1]))
        tr, te, tt, rp = L.regularization_path(g, params=L.ProxGradParams(max_iter=10), reg_params=[5.0, 0.5, 0.05], holdout_proportion=0.2,
                                               verbose=False, groups=draws, engine=api)
        g2 = model(np.random.default_rng(12))
        ctr, cte = L.cv_by_iter(g2, 0.2, L.ProxGradParams(1.0, max_iter=6, abs_tol=0.0, rel_tol=0.0), verbose=False, groups=draws, engine=api)
        res[name] = (tr, te, ctr, cte)
    for a, b in zip(res["hip"], res["cpu"]):
        assert cases.rel_err(a, b) < TOL


def test_fused_and_unfused_drivers_agree_on_the_gpu():
    rng = np.random.default_rng(13)
    g = model(rng, 2000, 100, 6, 0.4)
    tags = rng.integers(0, 4, int(g._rowptr[-1]))
    p = L.HipProxGradParams(max_iter=8)
    a = L.cross_validate(g, nfolds=4, params=p, verbose=False, groups=tags, fused=True)
    b = L.cross_validate(g, nfolds=4, params=p, verbose=False, groups=tags, fused=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])  # the compacted views are the same arrays


# ================================================================== the compaction against a numpy mask, exactly
# A, X and Y hold small integers, so every probe below is a sum of integers (or one rounding of an integer): free of order, compared with ==.
WG = 4096   # entries one workgroup of glrm_subset.hip compacts; scan_blocks_kernel carries across blocks of 1024 workgroups


def int_model(rng, m, n, observed=None, k=2):
    A = rng.integers(-9, 10, (m, n)).astype(np.float64)
    X, Y = rng.integers(-2, 3, (k, m)).astype(np.float64), rng.integers(-2, 3, (k, n)).astype(np.float64)
    obs = None if observed is None else np.nonzero(observed)
    return L.GLRM(A, L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), k, obs=obs, X=X, Y=Y)


def check_child(api, h, g, sp, rt, match, invert):
    """The child of `h` under the row-view tags rt (column-view tags rt[perm], the same entries) against the masked lists:
    the counts; the COLUMN view through error_metric (RealDomain, QuadLoss) at X = 0 -- the sum of a^2 -- and at the model's X, where u_ij
    depends on i and j, so a value that lost its row index or sits in another column's segment changes the sum; the ROW view through one
    fixed-size gradient step on X (alpha a power of two, ZeroReg): x_i + (sum_j 2 (u_ij - a_ij) y_j) * (-(alpha / (len_i + 1)))."""
    rt = np.ascontiguousarray(rt, dtype=np.uint8)
    keep = (rt == match) != bool(invert)
    I, J, a = sp.I[keep], sp.J[keep], g._rowvals[keep]
    X, Y = np.asfortranarray(g.X), np.asfortranarray(g.Y)
    doms = pack_domains([L.RealDomain()] * g.n)
    r = np.einsum("ki,ki->i", X[:, I], Y[:, J]) - a
    G = np.stack([np.bincount(I, weights=2 * r * Y[c, J], minlength=g.m) for c in range(g.k)])
    alpha = 0.125
    want_X = X + G * (-(alpha / (np.bincount(I, minlength=g.m) + 1.0)))
    hc = api.subset(h, rt, rt[sp.perm], match, invert)
    try:
        st = api.kernel_stats(hc)
        assert st["nnz_rows"] == int(keep.sum()) and st["nnz_cols"] == int(keep.sum())
        assert api.error_metric(hc, np.zeros_like(X), Y, doms, False) == float(np.sum(a * a))
        assert api.error_metric(hc, X, Y, doms, False) == float(np.sum(r * r))
        api.set_factors(hc, X, Y)
        api.gradstep_x(hc, alpha)
        Xn, Yn = np.zeros_like(X), np.zeros_like(Y)
        api.get_factors(hc, Xn, Yn)
        assert np.array_equal(Xn, want_X) and np.array_equal(Yn, Y)
    finally:
        api.destroy(hc)


@pytest.mark.parametrize("m,n", [(65, 63), (64, 64), (241, 17)], ids=["nnz4095", "nnz4096", "nnz4097"])
def test_subset_around_one_workgroup(m, n):
    rng = np.random.default_rng(m)
    g = int_model(rng, m, n)
    assert len(g._colidx) in (WG - 1, WG, WG + 1)
    sp = crossval._Split(g)
    api = hip()
    h = api.create(g.problem_arrays())
    try:
        rt = rng.integers(0, 3, m * n)
        for match, invert in ((0, False), (2, True)):
            check_child(api, h, g, sp, rt, match, invert)
        last = np.zeros(m * n, np.uint8)
        last[-1] = 1                                                            # the entry past the workgroup when nnz = 4097
        check_child(api, h, g, sp, last, 1, False)
        check_child(api, h, g, sp, last, 1, True)
    finally:
        api.destroy(h)


def tag_patterns(g, sp):
    nnz = len(g._colidx)
    z = np.zeros(nnz, np.uint8)
    first, last, row, col, head = z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
    first[0] = 1
    last[-1] = 1
    row[sp.I == g.m // 3] = 1                                                   # one whole segment of the row view
    col[sp.J == g.n // 2] = 1                                                   # one whole segment of the column view
    head[(sp.I < g.m // 2) & (sp.J < g.n // 2)] = 1                             # the trailing segments of both views come out empty
    return {"first": first, "last": last, "row": row, "col": col, "head": head}


@pytest.mark.parametrize("pattern", ["first", "last", "row", "col", "head"])
@pytest.mark.parametrize("shape", ["sparse", "full4097"])
def test_subset_tag_patterns(shape, pattern):
    """Only the first entry, only the last, one whole segment, everything but them (invert), and children whose trailing segments are empty.
    The sparse parent's own last three rows and last two columns hold nothing: ptr[s] == nnz for s < nseg."""
    rng = np.random.default_rng(17)
    if shape == "sparse":
        obs = rng.random((90, 70)) < 0.5
        obs[-3:, :] = False
        obs[:, -2:] = False
        g = int_model(rng, 90, 70, obs)
        assert g._rowptr[-4] == g._rowptr[-1] and g._colptr[-3] == g._colptr[-1]
    else:
        g = int_model(rng, 241, 17)
    sp = crossval._Split(g)
    rt = tag_patterns(g, sp)[pattern]
    assert rt.any()
    api = hip()
    h = api.create(g.problem_arrays())
    try:
        check_child(api, h, g, sp, rt, 1, False)
        check_child(api, h, g, sp, rt, 1, True)
    finally:
        api.destroy(h)


def test_subset_carries_across_1024_workgroups():
    """66000 x 64 fully observed: 4 224 000 observations, 1032 workgroups, so scan_blocks_kernel runs its second block of 1024 and the carry
    between them.  The tags keep one entry in three before workgroup 1024 of the row view and two in five after it, and what lies past
    workgroup 1024 of the column view is shifted once more.  Probes only, no fit."""
    m, n = 66000, 64
    rng = np.random.default_rng(1032)
    g = int_model(rng, m, n)
    nnz = m * n
    assert (nnz + WG - 1) // WG == 1032
    sp = crossval._Split(g)
    t = np.arange(nnz)
    rt = np.where(t < 1024 * WG, t % 3, (t % 5 < 2).astype(np.int64))
    colpos = np.empty(nnz, np.int64)
    colpos[sp.perm] = t                                                         # where the column view lists row-view entry t
    rt = np.where(colpos >= 1024 * WG, (rt + 1) % 3, rt).astype(np.uint8)
    api = hip()
    h = api.create(g.problem_arrays())
    try:
        check_child(api, h, g, sp, rt, 1, False)
        check_child(api, h, g, sp, rt, 1, True)
    finally:
        api.destroy(h)
