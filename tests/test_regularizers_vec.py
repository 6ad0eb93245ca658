"""The regularizers that carry a vector, on the host: the Python mirrors of fixed_latent_features, fixed_last_latent_features and RemQuadReg
(src/regularizers.jl:193-231,412-423) on known answers; fix_latent_features_ (src/modify_glrm.jl:25-29); their descriptors, placeholders
and the model's soft key; the extension header's symbols in both builds; and the seed selection of the GPU fits (tests/regs_vec.py)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import cases
import lowrankmodels.jl_amd as L
import regs_extra as RX
import regs_vec as RV
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd import regularizers as R
from test_oracle_vs_numpy import numpy_proxgrad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lowrankmodels.jl_amd")


# ------------------------------------------------------------------------------------------------ known answers

def test_fixed_last_prox_is_the_reference_s_literally():
    """:223 feeds the base u[n+1:end] -- the LAST k - n entries -- and puts the result FIRST: [3, 4, 5, 9, 8], not [1, 2, 3, 9, 8]."""
    r = L.fixed_last_latent_features(L.ZeroReg(), [9, 8])
    np.testing.assert_array_equal(r.prox([1, 2, 3, 4, 5], 0.3), [3, 4, 5, 9, 8])
    r = L.fixed_last_latent_features(L.QuadReg(0.5), [9, 8])     # prox_QuadReg(u, a) = u / (1 + 2 a scale)
    np.testing.assert_array_equal(r.prox([1, 2, 3, 4, 5], 1.0), [3 * (1 / 2), 4 * (1 / 2), 5 * (1 / 2), 9, 8])
    r = L.fixed_last_latent_features(L.OneReg(1), [7.0])         # nfix < k - nfix: the two ranges overlap
    np.testing.assert_array_equal(r.prox([5, -4, 3, -2, 1], 0.5), [-3.5, 2.5, -1.5, 0.5, 7])


def test_fixed_first_prox_and_the_constraint_constructors():
    r = L.fixed_latent_features(L.NonNegConstraint(), [-1.0, 2.0])
    np.testing.assert_array_equal(r.prox([5, 5, -3, 4, -0.5], 0.1), [-1, 2, 0, 4, 0])
    c = L.FixedLatentFeaturesConstraint([1.5, 2.5])
    assert isinstance(c, L.fixed_latent_features) and isinstance(c.r, L.ZeroReg) and c.n == 2
    np.testing.assert_array_equal(c.prox([0, 0, 7, 8], 1), [1.5, 2.5, 7, 8])
    c = L.FixedLastLatentFeaturesConstraint([1.5])
    assert isinstance(c, L.fixed_last_latent_features) and isinstance(c.r, L.ZeroReg)
    np.testing.assert_array_equal(c.prox([0, 6, 7, 8], 1), [6, 7, 8, 1.5])
    full = L.fixed_latent_features(L.QuadReg(2), [1.0, 2.0, 3.0])   # nfix = k: the base sees an empty vector
    np.testing.assert_array_equal(full.prox([9, 9, 9], 1), [1, 2, 3])
    assert full.evaluate([1, 2, 3]) == 0 and full.evaluate([1, 2, 4]) == math.inf
    np.testing.assert_array_equal(L.fixed_last_latent_features(L.SimplexConstraint(), [1.0, 2.0]).prox([9, 9], 1), [1, 2])
    with pytest.raises(ValueError):                                 # argmax of an empty vector throws in the reference as well
        L.fixed_latent_features(L.OneSparseConstraint(), [1.0, 2.0]).prox([9, 9], 1)


def test_evaluate_compares_exactly():
    y = np.array([0.1, -2.0])
    first, last = L.fixed_latent_features(L.QuadReg(2), y), L.fixed_last_latent_features(L.QuadReg(2), y)
    assert first.evaluate([0.1, -2.0, 3.0]) == 2 * 9.0 and last.evaluate([3.0, 0.1, -2.0]) == 2 * 9.0
    off = np.nextafter(0.1, 1.0)                                    # one ulp off the pin
    assert first.evaluate([off, -2.0, 3.0]) == math.inf and last.evaluate([3.0, off, -2.0]) == math.inf
    assert first.evaluate([0.1, np.nextafter(-2.0, 0.0), 3.0]) == math.inf
    assert first.evaluate([np.nan, -2.0, 3.0]) == math.inf and last.evaluate([3.0, 0.1, np.nan]) == math.inf
    zero = L.fixed_latent_features(L.ZeroReg(), [0.0])
    assert zero.evaluate([-0.0, 5.0]) == 0                          # IEEE ==: -0.0 equals +0.0
    assert first.evaluate([3.0, 0.1, -2.0]) == math.inf             # the pin is at the FRONT for fixed_latent_features
    bad_base = L.fixed_latent_features(L.NonNegConstraint(), [1.0])
    assert bad_base.evaluate([1.0, -1.0]) == math.inf and bad_base.evaluate([1.0, 1.0]) == 0


def test_rem_quad_reg_on_hand_values():
    r = L.RemQuadReg(2, [1.0, -3.0])
    # prox(u, a) = (u + 2 a s m) / (1 + 2 a s); a = 0.25, s = 2: (u + m) / 2
    np.testing.assert_array_equal(r.prox([3.0, 1.0], 0.25), [2.0, -1.0])
    assert r.evaluate([3.0, 1.0]) == 2 * (4.0 + 16.0) and r.evaluate([1.0, -3.0]) == 0
    one = L.RemQuadReg([0.5, 0.5])                                  # RemQuadReg(m) = RemQuadReg(1, m), :416
    assert one.scale == 1.0 and one.evaluate([1.5, 0.5]) == 1.0
    u, a, s, m = np.array([0.3, -0.7, 1.1]), 0.37, 0.7, np.array([0.2, 0.4, -0.6])
    want = np.array([(u[c] + ((2 * a) * s) * m[c]) / (1 + (2 * a) * s) for c in range(3)])   # this association, a division per entry
    np.testing.assert_array_equal(L.RemQuadReg(s, m).prox(u, a), want)


def test_scaling_methods_follow_the_reference():
    y = [1.0, 2.0]
    for r in (L.fixed_latent_features(L.QuadReg(3), y), L.fixed_last_latent_features(L.OneReg(3), y)):
        assert r.scale == 3 and r.mul_(5) is r and r.scale == 5 and r.r.scale == 5          # forwarded to the base (:209-210,230-231)
        with pytest.raises(TypeError):                                                      # typeof(r)() has no method (:40)
            2 * r
    q = L.RemQuadReg(3, y)
    assert q.mul_(0.5) is q and q.scale == 0.5 and q.descriptor() == (R.REM_QUAD, 0, 0.5)   # the generic mul! sets the scale
    with pytest.raises(TypeError):
        2 * q
    c = L.FixedLatentFeaturesConstraint(y)
    assert c.mul_(4) is c and c.scale == 1                                                  # mul!(::ZeroReg, _) is a no-op


def test_nesting_with_the_other_wrappers_is_refused():
    y = [1.0]
    for make in (lambda: L.lastentry1(L.fixed_latent_features(L.QuadReg(), y)), lambda: L.fixed_latent_features(L.lastentry1(L.QuadReg()), y),
                 lambda: L.fixed_last_latent_features(L.OrdinalReg(L.QuadReg()), y), lambda: L.MNLOrdinalReg(L.fixed_last_latent_features(L.QuadReg(), y)),
                 lambda: L.fixed_latent_features(L.fixed_last_latent_features(L.QuadReg(), y), y), lambda: L.fixed_latent_features(L.RemQuadReg(y), y),
                 lambda: L.lastentry_unpenalized(L.RemQuadReg(y))):
        with pytest.raises(NotImplementedError):
            make()


def test_fix_latent_features():
    """fix_latent_features!(glrm, n): ry[i] <- fixed_latent_features(ry[i], Y[1:n, i]) (src/modify_glrm.jl:25-29)."""
    rng = np.random.default_rng(3)
    g = L.GLRM(rng.standard_normal((6, 4)), L.QuadLoss(), L.QuadReg(0.1), L.OneReg(0.2), 3, rng=rng)
    Y = g.Y.copy()
    assert L.fix_latent_features_(g, 2) is g
    for j, r in enumerate(g.ry):
        assert isinstance(r, L.fixed_latent_features) and isinstance(r.r, L.OneReg) and r.r.scale == 0.2
        np.testing.assert_array_equal(r.y, Y[:2, j])
        assert r.evaluate(g.Y[:, j]) == 0.2 * abs(Y[2, j])
    g.Y[0, 0] += 1.0                                     # the pins are copies: they do not follow Y
    np.testing.assert_array_equal(g.ry[0].y, Y[:2, 0])
    assert not g.dense_eligible()


# ------------------------------------------------------------------------------------------------ descriptors, packing, soft key

def test_descriptors_placeholders_and_tables():
    fa, fb = L.fixed_latent_features(L.QuadReg(0.5), [1.0, 2.0]), L.fixed_last_latent_features(L.KSparseConstraint(2), [3.0])
    q = L.RemQuadReg(0.7, [1.0, 2.0, 3.0, 4.0])
    assert fa.descriptor() == (R.QUAD, R.WRAP_FIXED_FIRST, 0.5) and fb.descriptor() == (R.K_SPARSE, R.WRAP_FIXED_LAST, 2.0)
    assert q.descriptor() == (R.REM_QUAD, 0, 0.7) and (R.REM_QUAD, R.WRAP_FIXED_FIRST, R.WRAP_FIXED_LAST) == (10, 16, 32)
    regs = [fa, L.OneReg(3), fb, q]
    as_tuples = lambda a: [(int(x["kind"]), int(x["wrap"]), float(x["scale"])) for x in a]   # noqa: E731
    # what glrm_hip_create takes: the base kind without the new flag, ZeroReg for RemQuadReg, one entry per regularizer
    assert as_tuples(R.pack_regs(regs)) == [(R.QUAD, 0, 0.5), (R.ONE, 0, 3.0), (R.K_SPARSE, 0, 2.0), (R.ZERO, 0, 1.0)]
    descs, table, lens = R.pack_reg_vectors(regs, 4)
    assert as_tuples(descs) == [r.descriptor() for r in regs]
    assert lens.dtype == np.int32 and lens.tolist() == [2, 0, 1, 4]
    np.testing.assert_array_equal(table.reshape(4, 4), [[1, 2, 0, 0], [0, 0, 0, 0], [3, 0, 0, 0], [1, 2, 3, 4]])   # k x count, column-major
    assert R.pack_reg_vectors([L.QuadReg(), L.SimplexConstraint()], 4) is None and not R.carries_vector([L.lastentry1(L.QuadReg())])
    # one descriptor for the side only when the vectors are the same too; the placeholder count follows
    same = [L.RemQuadReg(1, [1.0, 2.0]) for _ in range(3)]
    assert len(R.pack_regs(same)) == 1 and len(R.pack_reg_vectors(same, 2)[0]) == 1
    other = same[:2] + [L.RemQuadReg(1, [1.0, 2.5])]
    assert len(R.pack_regs(other)) == 3 and R.pack_reg_vectors(other, 2)[2].tolist() == [2, 2, 2]


def test_the_soft_key_follows_the_contents_of_a_vector():
    rng = np.random.default_rng(5)
    g = L.GLRM(rng.standard_normal((5, 4)), L.QuadLoss(), L.QuadReg(0.1), [L.RemQuadReg(1, [1.0, 2.0]) for _ in range(4)], 2, rng=rng)
    hard, soft = g._descriptor_key()
    assert g._descriptor_key() == (hard, soft)
    with pytest.raises(ValueError):                      # the stored vector is read-only: contents change by assignment only
        g.ry[2].m[1] = 9.0
    e = _capi.EPOCH[0]
    g.ry[2].m = [1.0, 2.5]                               # only one entry of one vector changes
    assert _capi.EPOCH[0] > e
    hard2, soft2 = g._descriptor_key()
    assert hard2[0] == hard[0] and soft2 != soft
    g.ry[2].m = [1.0, 2.0]
    assert g._descriptor_key()[1] == soft                # and back
    f = L.GLRM(rng.standard_normal((5, 4)), L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.1), 3, rng=rng)
    k0 = f._descriptor_key()
    L.fix_latent_features_(f, 1)
    k1 = f._descriptor_key()
    assert k1[1] != k0[1]
    f.ry[0].y = [f.ry[0].y[0] + 1.0]
    assert f._descriptor_key()[1] != k1[1]
    plain = L.GLRM(rng.standard_normal((5, 4)), L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.2), 3, rng=rng)
    assert len(plain._descriptor_key()[1]) == 2          # models without vectors keep the key they had


def declared(header, pattern):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(" + pattern + r")\s*\(", txt)))


def test_both_builds_export_the_entry_points_of_the_extension_header():
    from lowrankmodels.jl_amd import build
    build.build_all(verbose=False)
    names = declared("glrm_hip_regvec.h", r"glrm_hip_\w+")
    assert names == ["glrm_hip_multi_set_regularizers_vec", "glrm_hip_set_regularizers_vec"]
    assert sorted("glrm_hip_" + s for s in _capi.REGVEC_SYMBOLS) == names and not set(_capi.REGVEC_SYMBOLS) & set(_capi.ABI_SYMBOLS)
    for so in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        lib = ctypes.CDLL(os.path.join(PKG, so), mode=ctypes.RTLD_LOCAL)
        for n in names:
            assert hasattr(lib, n), (so, n)
    assert hasattr(ctypes.CDLL(os.path.join(PKG, "libglrm_hip_testing.so"), mode=ctypes.RTLD_LOCAL), "glrm_test_regvec_prox_eval")
    assert not hasattr(ctypes.CDLL(os.path.join(PKG, "libglrm_hip.so"), mode=ctypes.RTLD_LOCAL), "glrm_test_regvec_prox_eval")
    hdr = open(os.path.join(ROOT, "include", "glrm_hip_regvec.h")).read()
    for name, value in (("GLRM_REG_REM_QUAD", R.REM_QUAD), ("GLRM_WRAP_FIXED_FIRST", R.WRAP_FIXED_FIRST), ("GLRM_WRAP_FIXED_LAST", R.WRAP_FIXED_LAST)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", hdr), name
    assert len(declared("glrm_hip.h", r"glrm_hip_\w+")) == 37 and _capi.ABI_VERSION == 3   # the boundary header is unchanged
    assert ctypes.sizeof(_capi.CReg) == 16 and ctypes.sizeof(_capi.CRegVec) == 16


def test_an_engine_without_the_extension_refuses_clearly():
    """The CPU oracle does not know these regularizers: the fit must raise, never run the placeholders."""
    import oracle as O
    mdl = RV.model("remquad_both", 5, 1)
    g = RV.glrm_of(mdl, 5)
    with pytest.raises(L.GLRMError) as ei:
        L.fit_b(g, mdl[-1], verbose=False, engine=O.oracle_api())
    assert ei.value.code == _capi.ERR_UNSUPPORTED and "carry a vector" in ei.value.message
    assert g._handle_cache is None


# ------------------------------------------------------------------------------------------------ seeds of the GPU fits

@pytest.mark.parametrize("key", list(RV.FITS), ids=lambda k: f"{k[0]}-k{k[1]}-inner{k[2]}")
def test_seeds_of_the_gpu_fits_do_not_fork_under_summation_order(key):
    name, k, inner = key
    A, losses, rx, ry, feats, exs, X0, Y0, p = RV.model(name, k, RV.FITS[key], inner)
    a = numpy_proxgrad(A, losses, rx, ry, feats, exs, X0, Y0, p)
    b = numpy_proxgrad(A, losses, rx, ry, feats, exs, X0.view(RX.SeqArray), Y0.view(RX.SeqArray), p)
    assert len(a[2]) == len(b[2]) == p.max_iter + 1
    worst = max(cases.rel_err(a[2], b[2]), cases.fro_err(a[0], b[0]), cases.fro_err(a[1], b[1]),
                float(np.max(np.abs(a[3] - b[3]) / b[3])), float(np.max(np.abs(a[4] - b[4]) / b[4])))
    print(key, "worst two-order difference:", worst)
    assert worst < 1e-9
    # a start that does not satisfy a pin has an infinite objective; every later one is finite
    assert (a[2][0] == math.inf) == (name in RV.INF_START), a[2][0]
    assert np.all(np.isfinite(a[2][1:])) and np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1]))
    assert RV.pinned_ok(rx, ry, a[0], a[1])


@pytest.mark.parametrize("last", [False, True], ids=["fixed_latent_features", "fixed_last_latent_features"])
def test_seed_of_the_replayed_fixedfeatures_script_does_not_fork(last):
    """test/fixedfeatures_test.jl with numpy's generator (tests/regs_vec.py): the simplex projection of the rows selects entries."""
    (A, losses, rx, ry, feats, exs, X0, Y0, p), Yfix = RV.fixedfeatures_script(last)
    a = numpy_proxgrad(A, losses, rx, ry, feats, exs, X0, Y0, p)
    b = numpy_proxgrad(A, losses, rx, ry, feats, exs, X0.view(RX.SeqArray), Y0.view(RX.SeqArray), p)
    assert len(a[2]) == len(b[2])
    worst = max(cases.rel_err(a[2], b[2]), cases.fro_err(a[0], b[0]), cases.fro_err(a[1], b[1]),
                float(np.max(np.abs(a[3] - b[3]) / b[3])), float(np.max(np.abs(a[4] - b[4]) / b[4])))
    print("fixedfeatures", last, "worst two-order difference:", worst, "iterations:", len(a[2]) - 1)
    assert worst < 1e-9
    assert np.array_equal(a[1][1:] if last else a[1][:3], Yfix) and a[2][0] == math.inf and np.all(np.isfinite(a[2][1:]))
