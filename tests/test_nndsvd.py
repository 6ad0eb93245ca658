"""The NMF initialization extension (include/glrm_hip_nmf.h: glrm_hip_init_nndsvd) is exported by both builds of the engine, stays
OUTSIDE the 37-symbol boundary of include/glrm_hip.h, is bound by name in the Julia file and in _capi, and is refused clearly where it
cannot run.  The dense numpy routine the GPU tests compare against (tests/nndsvd_ref.py) is held to its own invariants, and the
problems of the GPU suite to the three conditions that make the comparison meaningful, in every soft-impute round."""
import ctypes
import os
import re

import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import nndsvd_ref as R
from lowrankmodels.jl_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lowrankmodels.jl_amd")


def declared(header, pattern=r"glrm_hip_\w+"):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(" + pattern + r")\s*\(", txt)))


# ---- the boundary

def test_both_builds_export_the_entry_point():
    from lowrankmodels.jl_amd import build
    build.build_all(verbose=False)
    assert declared("glrm_hip_nmf.h") == ["glrm_hip_init_nndsvd"]
    for so in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        lib = ctypes.CDLL(os.path.join(PKG, so), mode=ctypes.RTLD_LOCAL)
        assert hasattr(lib, "glrm_hip_init_nndsvd"), so


def test_binding_table_lists_the_extension_apart():
    assert _capi.NMF_SYMBOLS == ("init_nndsvd",)
    assert sorted("glrm_hip_" + s for s in _capi.NMF_SYMBOLS) == declared("glrm_hip_nmf.h")
    others = (_capi.ABI_SYMBOLS, _capi.SCALE_SYMBOLS, _capi.INIT_SYMBOLS, _capi.STORAGE_SYMBOLS, _capi.REGVEC_SYMBOLS, _capi.TOPK_SYMBOLS)
    for t in others:
        assert not set(_capi.NMF_SYMBOLS) & set(t)
    assert len(declared("glrm_hip.h")) == 37 == len(_capi.ABI_SYMBOLS) and "glrm_hip_init_nndsvd" not in declared("glrm_hip.h")
    assert declared("glrm_hip_init.h") == ["glrm_hip_init_kmeanspp"] and _capi.ABI_VERSION == 3
    assert hasattr(_capi.Api, "init_nndsvd") and L.init_nndsvd_ is not None and "init_nndsvd_" in L.__all__


def test_julia_file_ccalls_the_declared_symbol_literally():
    src = open(os.path.join(ROOT, "julia", "HipGLRMNmf.jl")).read()
    code = "\n".join(line.split("#", 1)[0] for line in src.splitlines())
    calls = re.findall(r"ccall\(\s*\(\s*([^,]+?)\s*,", code)
    assert calls == [":glrm_hip_init_nndsvd"] and code.count("ccall(") == 1
    assert re.search(r"function\s+hip_init_nndsvd!\(", code)
    assert "no julia" in src                                   # like the other shims: never executed here
    # 13 arguments, as the header declares them
    types = re.search(r"Cint,\s*\((.*?)\),\s*h,", code, flags=re.S).group(1)
    assert len([t for t in types.split(",") if t.strip()]) == 13
    assert code.index("has_duplicates(glrm.observed_features)") < code.index("with_handle(")


# ---- the reference against itself

def triplets(seed, m=40, n=30, k=5):
    rng = np.random.default_rng(seed)
    U, s, Vt = np.linalg.svd(rng.standard_normal((m, n)) + 0.5, full_matrices=False)
    return U[:, :k], s[:k], Vt[:k].T


@pytest.mark.parametrize("v0", [0.0, 0.37])
def test_reference_outputs_are_nonnegative_and_sign_invariant(v0):
    for seed in range(5):
        U, s, V = triplets(seed)
        W, H, mp, mn = R.split_factors(U, s, V, v0)
        assert W.min() >= 0 and H.min() >= 0 and (mp != mn).all()
        flips = np.where(np.random.default_rng(100 + seed).random(len(s)) < 0.5, -1.0, 1.0)
        assert (flips < 0).any()
        W2, H2, mp2, mn2 = R.split_factors(U * flips, s, V * flips, v0)
        assert np.array_equal(W.view(np.uint64), W2.view(np.uint64)) and np.array_equal(H.view(np.uint64), H2.view(np.uint64))
        assert np.array_equal(np.maximum(mp, mn), np.maximum(mp2, mn2))


def test_reference_recovers_a_positive_rank_one_matrix():
    rng = np.random.default_rng(3)
    a, b = 0.5 + rng.random(30), 0.5 + rng.random(20)
    A = np.outer(a, b)
    for variant in ("std", "a"):
        W, H, info = R.nndsvd(A, 1, variant)
        assert np.abs(W @ H - A).max() <= 1e-12 * np.abs(A).max()
    out = R.init_nndsvd(A, rng.random(A.shape) < 2.0, np.ones(20), 1, max_iters=2)
    assert np.abs(out["X"].T @ out["Y"] - A).max() <= 1e-12 * np.abs(A).max()
    assert not R.init_nndsvd(A, np.ones(A.shape, bool), np.ones(20), 1, zeroh=True)["Y"].any()
    with pytest.raises(NotImplementedError):
        R.nndsvd(A, 1, "ar")


def test_reference_soft_impute_keeps_the_observed_entries_and_fills_the_rest():
    """One round by hand: B_1 is s A on the mask and W_0 H_0 elsewhere."""
    fx = R.FIXTURES[1]
    A, mask = R.fixture(*fx)
    k = fx[2]
    scales = 1.0 + np.arange(fx[1]) / fx[1]
    r0 = R.init_nndsvd(A, mask, scales, k, max_iters=0)
    r1 = R.init_nndsvd(A, mask, scales, k, max_iters=1)
    B1 = np.where(mask, A * scales, r0["X"].T @ r0["Y"])
    W, H, info = R.nndsvd(B1, k)
    assert np.array_equal(r1["X"], W.T) and np.array_equal(r1["Y"], H)
    np.testing.assert_allclose(r1["rounds"][0]["sigma"], np.linalg.svd(np.where(mask, A * scales, 0.0), compute_uv=False), rtol=1e-12)


# ---- the problems of the GPU suite meet the conditions in every round

@pytest.mark.parametrize("fx", R.FIXTURES, ids=lambda fx: f"{fx[0]}x{fx[1]}k{fx[2]}")
def test_fixture_conditions(fx):
    m, n, k = fx[:3]
    A, mask = R.fixture(*fx)
    assert A.shape == (m, n) and np.linalg.matrix_rank(A) == fx[3] + 1 == k
    assert mask.all() if fx[4] == 1.0 else abs(mask.mean() - fx[4]) < 0.02
    l = min(k + 8, m, n)
    for max_iters in R.ROUNDS:
        figs = R.check_conditions(R.fixture_reference(fx, max_iters), k, l)
        assert len(figs) == max_iters + 1
        print(fx, max_iters, figs)
    R.check_conditions(R.fixture_reference(fx, 0, "a"), k, l)


def test_further_gpu_cases_meet_the_conditions():
    full = R.FIXTURES[3]
    R.check_conditions(R.fixture_reference(full, 2, "a"), full[2], min(full[2] + 8, full[0], full[1]))
    A, mask, k, scales = R.scaled_case()
    for scale in (True, False):
        R.check_conditions(R.init_nndsvd(A, mask, scales, k, scale=scale, max_iters=2), k, k + 8)
    A, mask, k, scales = R.empty_case()
    R.check_conditions(R.init_nndsvd(A, mask, scales, k, max_iters=2), k, k + 8)
    R.check_conditions(R.fixture_reference(R.FIXTURES[0], 1, "std", True), 4, 12)
    A, mask, k, scales = R.long_case()
    R.check_conditions(R.init_nndsvd(A, mask, scales, k, max_iters=1), k, 11)


# ---- refusals that need no GPU

def small_model(k=2, **kw):
    rng = np.random.default_rng(0)
    return L.GLRM(1.0 + rng.random((12, 5)), L.QuadLoss(), L.NonNegConstraint(), L.NonNegConstraint(), k, rng=rng, **kw)


def untouched(g, X0, Y0):
    return np.array_equal(g.X, X0) and np.array_equal(g.Y, Y0) and g._handle_cache is None and not hasattr(g, "_init_nndsvd_info")


def test_multidimensional_losses_are_refused_before_anything_is_touched():
    g = L.GLRM(np.ones((5, 1)), L.MultinomialLoss(3), L.QuadReg(), L.QuadReg(), 2)
    X0, Y0 = g.X.copy(), g.Y.copy()
    with pytest.raises(NotImplementedError, match="multi-dimensional"):
        L.init_nndsvd_(g)
    assert untouched(g, X0, Y0)


def test_variant_ar_and_bad_arguments_are_refused():
    g = small_model()
    X0, Y0 = g.X.copy(), g.Y.copy()
    with pytest.raises(NotImplementedError, match="NMF.jl's own random draws"):
        L.init_nndsvd_(g, variant="ar")
    with pytest.raises(ValueError, match="variant"):
        L.init_nndsvd_(g, variant="b")
    with pytest.raises(ValueError, match="negative"):
        L.init_nndsvd_(g, max_iters=-1)
    assert untouched(g, X0, Y0)


def test_a_duplicated_pair_is_refused():
    I, J = np.nonzero(np.ones((12, 5), bool))
    g = small_model(obs=(np.append(I, 3), np.append(J, 2)))
    X0, Y0 = g.X.copy(), g.Y.copy()
    with pytest.raises(ValueError, match=r"observed_features\[3\] lists 2 twice"):
        L.init_nndsvd_(g)
    assert untouched(g, X0, Y0)


def test_an_engine_without_the_extension_refuses_clearly():
    import oracle as O
    g = small_model()
    X0 = g.X.copy()
    with pytest.raises(_capi.GLRMError) as ei:
        L.init_nndsvd_(g, engine=O.oracle_api())
    assert ei.value.code == _capi.ERR_UNSUPPORTED and "NMF initialization extension" in ei.value.message
    assert np.array_equal(g.X, X0) and not hasattr(g, "_init_nndsvd_info")
    g.close()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_fails_loudly_without_a_gpu():
    from lowrankmodels.jl_amd import build
    build.build_all(verbose=False)
    g = small_model()
    X0 = g.X.copy()
    with pytest.raises(_capi.GLRMError) as ei:
        L.init_nndsvd_(g)
    assert ei.value.code == _capi.ERR_HIP and "no CPU fallback" in ei.value.message
    assert np.array_equal(g.X, X0)
