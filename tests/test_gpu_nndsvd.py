"""-m gpu: glrm_hip_init_nndsvd (include/glrm_hip_nmf.h) against the dense numpy routine of tests/nndsvd_ref.py.

Every comparison calls the engine with svd_tol = 1e-13 and svd_max_iter = 400 and holds the factors to the project's factor contract,
max|X - X_ref| <= 1e-5 max|X_ref| (likewise Y; relative to the largest entry because an entry of a singular vector within rounding of 0
may land on either side of it), and the singular values to rtol 1e-8 -- what tests/test_gpu_init_svd.py uses.

The comparison only means something where the singular vectors are well conditioned and no split is a coin flip, so every case asserts
on the CPU, for every soft-impute round and BEFORE the engine is called (it fails, it never skips), the three conditions of
nndsvd_ref.check_conditions: smallest gap among the first k + 1 singular values >= 0.03 sigma_1, sigma_l / sigma_k <= 0.45 with
l = min(k + 8, m, n) the engine's block, and |mp - mn| / max(mp, mn) >= 5e-3 for every component.  Variant `a` fills the zeros of W
and H with the mean, which makes the imputed matrix of a later round nearly rank-deficient beyond k on the masked fixtures (gaps of
0.003 sigma_1); it is therefore compared in round 0 on every fixture and in later rounds on the fully observed one, where the conditions
hold and the mean still goes through the residual sum and the (X 1)'(Y 1) term."""
import functools

import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import nndsvd_ref as R
from lowrankmodels.jl_amd import _capi

pytestmark = pytest.mark.gpu

SVD = dict(svd_tol=1e-13, svd_max_iter=400)
FULL = R.FIXTURES[3]          # 64 x 1500, fully observed


def hip():
    return _capi.hip_api()


def model(A, mask, k, scales=None, rx=None, ry=None):
    losses = L.QuadLoss() if scales is None else [L.QuadLoss(float(s)) for s in scales]
    return L.GLRM(np.array(A), losses, rx or L.ZeroReg(), ry or L.ZeroReg(), k, obs=np.nonzero(mask))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def compare(g, ref, what=""):
    info = g._init_nndsvd_info
    ex = np.abs(g.X - ref["X"]).max() / np.abs(ref["X"]).max()
    ey = np.abs(g.Y - ref["Y"]).max() / max(np.abs(ref["Y"]).max(), 1e-300)
    es = np.abs(info["singular_values"] / ref["singular_values"] - 1).max()
    print(what, "X", ex, "Y", ey, "sigma", es, "iterations", info["iterations"].tolist())
    np.testing.assert_allclose(info["singular_values"], ref["singular_values"], rtol=1e-8)
    assert np.abs(g.X - ref["X"]).max() <= 1e-5 * np.abs(ref["X"]).max()
    assert np.abs(g.Y - ref["Y"]).max() <= 1e-5 * np.abs(ref["Y"]).max()
    assert g.X.min() >= 0 and g.Y.min() >= 0
    # the diagnostic: products of norms of parts of unit vectors, so absolute 1e-6 is relative to 1 (an all-positive vector's smaller
    # product is rounding noise around 0)
    np.testing.assert_allclose(info["split"], ref["split"], rtol=0, atol=1e-6)


def run(A, mask, k, scales=None, **kw):
    """Reference (conditions asserted) and engine on one problem; returns (model, reference)."""
    m, n = A.shape
    ref = R.init_nndsvd(A, mask, np.ones(n) if scales is None else scales, k, **kw)
    print("conditions (gap, tail, margin) per round:", R.check_conditions(ref, k, min(k + 8, m, n)))
    g = model(A, mask, k, scales)
    L.init_nndsvd_(g, engine=hip(), **kw, **SVD)
    compare(g, ref)
    g.close()
    return g, ref


@pytest.mark.parametrize("max_iters", R.ROUNDS)
@pytest.mark.parametrize("fx", R.FIXTURES, ids=lambda fx: f"{fx[0]}x{fx[1]}k{fx[2]}")
def test_fixtures(fx, max_iters):
    A, mask = R.fixture(*fx)
    m, n, k = fx[:3]
    ref = R.fixture_reference(fx, max_iters)
    R.check_conditions(ref, k, min(k + 8, m, n))
    g = model(A, mask, k)
    L.init_nndsvd_(g, scale=False, max_iters=max_iters, engine=hip(), **SVD)
    compare(g, ref)
    assert len(g._init_nndsvd_info["iterations"]) == max_iters + 1 and np.all(g._init_nndsvd_info["iterations"] >= 1)
    g.close()


@pytest.mark.parametrize("fx, max_iters", [(fx, 0) for fx in R.FIXTURES] + [(FULL, 1), (FULL, 2)],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_variant_a_fills_the_zeros_with_the_mean(fx, max_iters):
    A, mask = R.fixture(*fx)
    m, n, k = fx[:3]
    ref = R.fixture_reference(fx, max_iters, "a")
    R.check_conditions(ref, k, min(k + 8, m, n))
    assert ref["rounds"][-1]["v0"] > 1 and (ref["X"] == ref["rounds"][-1]["v0"]).any()     # the mean is visible in the result
    g = model(A, mask, k)
    L.init_nndsvd_(g, scale=False, variant="a", max_iters=max_iters, engine=hip(), **SVD)
    compare(g, ref)
    g.close()


@pytest.mark.parametrize("max_iters", [0, 1])
def test_zeroh(max_iters):
    fx = R.FIXTURES[0]
    A, mask = R.fixture(*fx)
    g, ref = run(A, mask, fx[2], zeroh=True, max_iters=max_iters)
    assert not g.Y.any() and g.X.any()


@pytest.mark.parametrize("max_iters", [0, 2])
def test_per_column_loss_scales_on_and_off(max_iters):
    A, mask, k, scales = R.scaled_case()
    on, ref_on = run(A, mask, k, scales, scale=True, max_iters=max_iters)
    off, ref_off = run(A, mask, k, scales, scale=False, max_iters=max_iters)
    assert np.array_equal(ref_off["Y"], R.fixture_reference(R.FIXTURES[0], max_iters)["Y"])  # scale off: the scales are not read
    assert np.abs(on.Y - off.Y).max() > 1e-3 * np.abs(off.Y).max()


@pytest.mark.parametrize("max_iters", [0, 2])
def test_an_empty_row_and_an_empty_column(max_iters):
    A, mask, k, _ = R.empty_case()
    assert not mask[5].any() and not mask[:, 7].any()
    g, ref = run(A, mask, k, max_iters=max_iters)
    if max_iters == 0:
        assert not g.X[:, 5].any() and not g.Y[:, 7].any()


def test_a_column_longer_than_one_chunk():
    """40000 x 12: every column list spans three 16384-entry chunks of the column product and of the residual pass."""
    A, mask, k, _ = R.long_case()
    assert mask.all() and mask.shape[0] > 2 * 16384
    run(A, mask, k, max_iters=1)


def test_a_block_wider_than_64_lanes():
    """k = 70, l = 78: two values per lane in the products, more than one trip of the residual kernel's component loop.  Fully
    observed, so the soft-impute round decomposes the same matrix again; singular values only."""
    rng = np.random.default_rng(4)
    m, n, k = 300, 200, 70
    A = rng.standard_normal((m, k)) @ (rng.standard_normal((k, n)) * np.linspace(3, 1, k)[:, None]) + 0.01 * rng.standard_normal((m, n))
    s = np.linalg.svd(A, compute_uv=False)
    for max_iters in (0, 1):
        g = model(A, np.ones((m, n), bool), k)
        L.init_nndsvd_(g, max_iters=max_iters, engine=hip(), **SVD)
        np.testing.assert_allclose(g._init_nndsvd_info["singular_values"], s[:k], rtol=1e-8)
        assert g.X.min() >= 0 and g.Y.min() >= 0
        g.close()


def test_fully_observed_soft_impute_changes_nothing():
    A, mask = R.fixture(*FULL)
    assert mask.all()
    g0, g2 = model(A, mask, FULL[2]), model(A, mask, FULL[2])
    L.init_nndsvd_(g0, max_iters=0, engine=hip(), **SVD)
    L.init_nndsvd_(g2, max_iters=2, engine=hip(), **SVD)
    assert np.abs(g2.X - g0.X).max() <= 1e-5 * np.abs(g0.X).max() and np.abs(g2.Y - g0.Y).max() <= 1e-5 * np.abs(g0.Y).max()
    np.testing.assert_allclose(g2._init_nndsvd_info["singular_values"], g0._init_nndsvd_info["singular_values"], rtol=1e-8)
    g0.close()
    g2.close()


@functools.lru_cache(maxsize=None)
def raw_problem():
    fx = R.FIXTURES[0]
    A, mask = R.fixture(*fx)
    g = model(A, mask, fx[2], rx=L.QuadReg(0.1), ry=L.QuadReg(0.1))
    return g.problem_arrays(), fx


def call(api, h, fx, **kw):
    m, n, k = fx[:3]
    X, Y = np.zeros((k, m), order="F"), np.zeros((k, n), order="F")
    info = api.init_nndsvd(h, X, Y, **{**SVD, **kw})
    return X, Y, info


def test_two_calls_return_the_same_bits():
    pa, fx = raw_problem()
    api = hip()
    h = api.create(pa)
    try:
        a = call(api, h, fx, variant="a", max_iters=2)
        b = call(api, h, fx, variant="a", max_iters=2)
    finally:
        api.destroy(h)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    assert same_bits(a[2]["singular_values"], b[2]["singular_values"]) and same_bits(a[2]["split"], b[2]["split"])
    assert a[2]["iterations"].tolist() == b[2]["iterations"].tolist()


def test_the_handle_is_left_alone_and_fits_afterwards():
    pa, fx = raw_problem()
    m, n, k = fx[:3]
    rng = np.random.default_rng(3)
    X0, Y0 = np.asfortranarray(rng.standard_normal((k, m))), np.asfortranarray(rng.standard_normal((k, n)))
    api = hip()
    h = api.create(pa)
    try:
        before = api.objective(h, X0, Y0)                       # leaves X0, Y0 resident in the handle
        X, Y, _ = call(api, h, fx, max_iters=1)
        Xg, Yg = np.zeros_like(X0), np.zeros_like(Y0)
        api.get_factors(h, Xg, Yg)
        assert same_bits(Xg, X0) and same_bits(Yg, Y0)
        assert api.objective(h, X0, Y0) == before
        obj, _ = api.fit(h, L.HipProxGradParams(max_iter=5), X, Y)
        assert len(obj) >= 2 and np.all(np.isfinite(obj)) and obj[-1] < obj[0]
    finally:
        api.destroy(h)


def test_refusals():
    pa, fx = raw_problem()
    m, n, k = fx[:3]
    api = hip()
    A, mask = R.fixture(*fx)

    def refused(h, code, text, shape=(k, m, n), **kw):
        kk, mm, nn = shape
        X, Y = np.full((kk, mm), 7.0, order="F"), np.full((kk, nn), 7.0, order="F")
        try:
            with pytest.raises(_capi.GLRMError) as ei:
                api.init_nndsvd(h, X, Y, **kw)
            assert ei.value.code == code and text in ei.value.message, ei.value
            assert (X == 7.0).all() and (Y == 7.0).all()
        finally:
            api.destroy(h)

    gd = L.GLRM(np.random.default_rng(6).standard_normal((64, 48)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 16)
    refused(api.create(gd.problem_arrays(dense=True)), _capi.ERR_UNSUPPORTED, "dense_A", shape=(16, 64, 48))
    refused(api.create(gd.problem_arrays(rows=(0, 32))), _capi.ERR_INVALID, "single-shard", shape=(16, 64, 48))
    refused(api.create(pa, defer=True), _capi.ERR_INVALID, "glrm_hip_finalize")
    refused(api.create(pa, storage=1), _capi.ERR_UNSUPPORTED, "storage = f32")
    gm = L.GLRM(np.ones((8, 2)), [L.QuadLoss(), L.MultinomialLoss(3)], L.ZeroReg(), L.ZeroReg(), 2)
    refused(api.create(gm.problem_arrays()), _capi.ERR_UNSUPPORTED, "multi-dimensional loss", shape=(2, 8, 4))
    gk = L.GLRM(np.ones((6, 9)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 7)
    refused(api.create(gk.problem_arrays()), _capi.ERR_INVALID, "exceeds min(m, n)", shape=(7, 6, 9))
    refused(api.create(pa), _capi.ERR_UNSUPPORTED, "variant ar", variant="ar")
    refused(api.create(pa), _capi.ERR_INVALID, "negative", max_iters=-1)


def test_no_rank_above_128_reaches_the_routine():
    """k > 128 is refused by glrm_hip_create for every handle, so the routine's own k <= 128 check cannot be reached through a handle."""
    g = L.GLRM(np.ones((130, 130)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 129)
    with pytest.raises(_capi.GLRMError) as ei:
        hip().create(g.problem_arrays())
    assert ei.value.code == _capi.ERR_UNSUPPORTED and "128" in ei.value.message


def test_the_python_layer_refuses_before_the_handle_is_touched():
    A, mask = R.fixture(*R.FIXTURES[1])
    I, J = np.nonzero(mask)
    g = L.GLRM(np.array(A), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 3, obs=(np.append(I, I[0]), np.append(J, J[0])))
    X0 = g.X.copy()
    with pytest.raises(ValueError, match="twice"):
        L.init_nndsvd_(g, engine=hip())
    assert np.array_equal(g.X, X0) and g._handle_cache is None and not hasattr(g, "_init_nndsvd_info")


def test_no_device_memory_leak():
    """20 call cycles in two windows of ten under the accounting of tests/test_gpu_leaks.py (torch.cuda.mem_get_info; run alone, nearly all
    of this test's time is torch starting up, which the suite pays once)."""
    import torch
    pa, fx = raw_problem()
    api = hip()

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    h = api.create(pa)       # one handle: the call's scratch (blocks, residual arrays, factors) is what could leak
    try:
        def cycle():
            call(api, h, fx, variant="a", max_iters=1, svd_tol=1e-8)
        cycle()
        cycle()
        levels = [free_bytes()]
        for _ in range(2):       # two windows of ten, as tests/test_gpu_storage_f32.py: a leak loses memory in both
            for _ in range(10):
                cycle()
            levels.append(free_bytes())
    finally:
        api.destroy(h)
    lost = [levels[i] - levels[i + 1] for i in range(2)]
    assert min(lost) < 4 << 20, f"device memory lost per window of 10 call cycles (MiB): {[round(x / 2**20, 2) for x in lost]}"


def test_nnmf_fit_from_the_engines_start_never_increases():
    rng = np.random.default_rng(8)
    m, n, k = 300, 200, 5
    A = np.abs(rng.standard_normal((m, k))) @ np.abs(rng.standard_normal((k, n))) + 0.05 * np.abs(rng.standard_normal((m, n)))
    g = L.GLRM(A, L.QuadLoss(), L.NonNegConstraint(), L.NonNegConstraint(), k, obs=np.nonzero(rng.random((m, n)) < 0.8))
    L.init_nndsvd_(g, max_iters=1, engine=hip())
    assert g.X.min() >= 0 and g.Y.min() >= 0 and g.X.max() > 0 and g.Y.max() > 0
    X, Y, ch = L.fit_b(g, L.HipProxGradParams(max_iter=30), verbose=False)
    obj = np.asarray(ch.objective)
    print("objective", obj[:4].tolist(), "...", obj[-1])
    assert len(obj) >= 3 and np.all(np.isfinite(obj)) and np.all(np.diff(obj[1:]) <= 0) and obj[-1] < obj[1]
    assert X.min() >= 0 and Y.min() >= 0
    g.close()
