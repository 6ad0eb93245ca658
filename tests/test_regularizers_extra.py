"""The vector regularizers on the host: the Python mirrors of QuadConstraint, NonNegOneReg, OneSparseConstraint, KSparseConstraint and
SimplexConstraint (src/regularizers.jl:68-76,118-138,235-291,323-348) against the reference's own known answers (test/reg_test.jl) and
against properties; their descriptors; the frozen CPU oracle refusing them; and the seed selection of the GPU fits (tests/regs_extra.py)."""
import math

import numpy as np
import pytest

import cases
import lowrankmodels.jl_amd as L
import oracle as O
import regs_extra as RX
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd import regularizers as R
from test_oracle_vs_numpy import numpy_proxgrad


def test_reference_known_answers():
    """test/reg_test.jl"""
    r = L.QuadConstraint(7)
    assert r.evaluate(np.ones(7)) == 0 and r.evaluate(np.ones(100)) == math.inf
    np.testing.assert_array_equal(r.prox(np.ones(100), 1), np.ones(100) * 7 / 10)
    r = L.KSparseConstraint(3)
    v = np.array([-1.0, 2, -3, 4, -5])
    assert r.evaluate(v) == math.inf
    np.testing.assert_array_equal(r.prox(v, 1), [0, 0, -3, 4, -5])
    assert r.evaluate(r.prox(v, 1)) == 0


def test_quad_constraint_always_rescales_and_zero_gives_nan():
    r = L.QuadConstraint(2)
    np.testing.assert_allclose(np.linalg.norm(r.prox([0.1, 0.2], 0.5)), 2, rtol=1e-15)   # from inside the ball too
    assert np.all(np.isnan(r.prox(np.zeros(3), 1)))
    assert r.evaluate([2, 0]) == 0 and r.evaluate([2 + 1e-13, 0]) == 0 and r.evaluate([2 + 1e-11, 0]) == math.inf


def test_nonneg_one_reg():
    r = L.NonNegOneReg(3)
    np.testing.assert_array_equal(r.prox([1.0, -2.0, 0.25], 0.5), [0.5, 0, 0])   # max(u - alpha, 0): scale is not in it
    assert r.evaluate([1, 2]) == 9 and r.evaluate([1, -1e-300]) == math.inf


def test_one_sparse_keeps_the_largest_signed_entry():
    r = L.OneSparseConstraint()
    np.testing.assert_array_equal(r.prox([-3.0, -1.0, -2.0]), [0, -1, 0])
    np.testing.assert_array_equal(r.prox([-5.0, 2.0, 2.0, 1.0]), [0, 2, 0, 0])   # first maximal index
    assert r.evaluate([0, 0, 0]) == 0 and r.evaluate([0, -4, 0]) == 0 and r.evaluate([1, 0, 1]) == math.inf


def test_k_sparse_ties_and_bounds():
    r = L.KSparseConstraint(2)
    np.testing.assert_array_equal(r.prox([0.0, 0, 0, 0]), [0, 0, 0, 0])
    np.testing.assert_array_equal(r.prox([1.0, -1.0, 1.0]), [1, -1, 0])          # equal |u|: the lower indices stay
    assert r.evaluate([1, 0, 2]) == 0 and r.evaluate([1, 3, 2]) == math.inf
    with pytest.raises(IndexError):
        L.KSparseConstraint(4).prox([1.0, 2.0, 3.0])


@pytest.mark.parametrize("k", [1, 2, 3, 7, 33])
def test_simplex_prox_properties(k):
    """Results are >= 0 and sum to 1 within 1e-15 k.  The sum bound is checked on u = z + e, z on the simplex and |e_i| <= 1 / k, because
    the error of sum(p) grows with the size of the running sums, not only with k: with s entries in the support, sum(p) = ysum_s - s t, and
    its error is that of the sequential ysum ((s - 1) additions, each within 2^-53 |partial sum|), of ysum - 1 and of the division
    (together within 2^-52 |ysum_s - 1|), of the s subtractions u_j - t (within 2^-53 sum(p) in total) and of this test's own np.sum(p)
    ((k - 1) 2^-53).  For these inputs every partial sum is at most sum(z) + sum|e| <= 2, so the total is below
    (k - 1)(2^-52 + 2^-53) + 2^-51 < 3.4e-16 k + 4.5e-16 <= 1e-15 k.  For |u| of size 30 the partial sums, and with them the error, are
    30 times larger and the bound is not attainable; such inputs are checked for sign and feasibility only."""
    rng = np.random.default_rng(k)
    r = L.SimplexConstraint()
    for _ in range(50):
        u = rng.dirichlet(np.ones(k)) + rng.uniform(-1, 1, k) / k
        p = r.prox(u, 0.3)
        assert np.all(p >= 0) and abs(np.sum(p) - 1) <= 1e-15 * k, (u, p, abs(np.sum(p) - 1))
        assert r.evaluate(p) == 0
    for _ in range(50):
        u = rng.standard_normal(k) * rng.choice([0.1, 1, 10])
        p = r.prox(u, 0.3)
        assert np.all(p >= 0) and r.evaluate(p) == 0, (u, p)
    for _ in range(20):   # points of the simplex are fixed (to rounding of the threshold)
        z = rng.dirichlet(np.ones(k))
        np.testing.assert_allclose(r.prox(z, 1.0), z, rtol=0, atol=4e-16)
    e = np.zeros(k); e[k // 2] = 1.0
    np.testing.assert_array_equal(r.prox(e), e)
    assert r.evaluate(np.full(k, -1.0)) == math.inf and r.evaluate(2 * e) == math.inf


def test_simplex_prox_is_the_closest_point():
    """200 random vectors: no point of a fine cover of the simplex (vertices, 4 000 Dirichlet draws, the grid of step 1/40) is closer."""
    rng = np.random.default_rng(200)
    r = L.SimplexConstraint()
    for t in range(200):
        k = 2 + t % 3
        u = rng.standard_normal(k) * (0.3 if t % 2 else 2.0)
        p = r.prox(u)
        steps = np.arange(41) / 40
        grid = np.array(np.meshgrid(*[steps] * (k - 1))).reshape(k - 1, -1).T
        grid = grid[grid.sum(axis=1) <= 1 + 1e-12]
        grid = np.hstack([grid, np.maximum(1 - grid.sum(axis=1, keepdims=True), 0)])
        cover = np.vstack([np.eye(k), rng.dirichlet(np.ones(k) * rng.choice([0.3, 1, 3]), 4000), grid])
        best = np.min(np.sum((cover - u) ** 2, axis=1))
        assert np.sum((p - u) ** 2) <= best + 1e-12, (u, p)


def test_scaling_methods_follow_the_reference():
    """mul! is a no-op and scale() is 1 (src/regularizers.jl:75-76,137-138,254-255,347-348); newscale * r builds typeof(r)() (:40)."""
    for r in (L.QuadConstraint(7), L.NonNegOneReg(3), L.OneSparseConstraint(), L.KSparseConstraint(2), L.SimplexConstraint()):
        before = r.descriptor()
        assert r.mul_(5) is r and r.descriptor() == before and r.scale == 1
    q = 2 * L.QuadConstraint(7)
    assert isinstance(q, L.QuadConstraint) and q.max_2norm == 1      # reset to the default parameter
    q = 2 * L.NonNegOneReg(3)
    assert isinstance(q, L.NonNegOneReg) and q.descriptor() == (R.NONNEG_ONE, 0, 1.0)
    assert isinstance(3 * L.SimplexConstraint(), L.SimplexConstraint) and isinstance(3 * L.OneSparseConstraint(), L.OneSparseConstraint)
    with pytest.raises(TypeError):   # KSparseConstraint has no zero-argument constructor
        2 * L.KSparseConstraint(2)
    g = L.lastentry1(L.QuadConstraint(3))
    g.mul_(9)
    assert g.descriptor() == (R.QUAD_CONSTRAINT, R.WRAP_LASTENTRY1, 3.0)


def test_descriptors_pack_to_the_table():
    want = [(L.QuadConstraint(2.5), (5, 0, 2.5)), (L.NonNegOneReg(0.7), (6, 0, 0.7)), (L.OneSparseConstraint(), (7, 0, 1.0)),
            (L.KSparseConstraint(3), (8, 0, 3.0)), (L.SimplexConstraint(), (9, 0, 1.0)),
            (L.lastentry1(L.SimplexConstraint()), (9, 1, 1.0)), (L.lastentry_unpenalized(L.KSparseConstraint(2)), (8, 2, 2.0))]
    for r, d in want:
        assert r.descriptor() == d
    packed = R.pack_regs([r for r, _ in want])
    assert [(int(x["kind"]), int(x["wrap"]), float(x["scale"])) for x in packed] == [d for _, d in want]
    r = L.QuadConstraint(1)
    e = _capi.EPOCH[0]
    r.max_2norm = 4.0                                   # a changed field invalidates cached packed descriptors
    assert _capi.EPOCH[0] > e and r.descriptor() == (5, 0, 4.0)


@pytest.mark.parametrize("kind", list(RX.NEW_KINDS))
@pytest.mark.parametrize("side", ["rx", "ry"])
def test_the_frozen_oracle_refuses_the_new_kinds(kind, side):
    """oracle/glrm_oracle.c validates against GLRM_REG_KIND_COUNT = 5: it must never compute a new kind as ZeroReg."""
    mdl = RX.model(f"{kind}_{side}", 5, 1)
    g = RX.glrm_of(mdl, 5)
    with pytest.raises(L.GLRMError) as ei:
        L.fit_b(g, mdl[-1], verbose=False, engine=O.oracle_api())
    assert ei.value.code == _capi.ERR_UNSUPPORTED


@pytest.mark.parametrize("key", list(RX.FITS), ids=lambda k: f"{k[0]}-k{k[1]}-inner{k[2]}")
def test_seeds_of_the_gpu_fits_do_not_fork_under_summation_order(key):
    name, k, inner = key
    A, losses, rx, ry, feats, exs, X0, Y0, p = RX.model(name, k, RX.FITS[key], inner)
    a = numpy_proxgrad(A, losses, rx, ry, feats, exs, X0, Y0, p)
    b = numpy_proxgrad(A, losses, rx, ry, feats, exs, X0.view(RX.SeqArray), Y0.view(RX.SeqArray), p)
    assert len(a[2]) == len(b[2]) == p.max_iter + 1
    assert cases.rel_err(a[2], b[2]) < 1e-9
    assert cases.fro_err(a[0], b[0]) < 1e-9 and cases.fro_err(a[1], b[1]) < 1e-9
    np.testing.assert_allclose(a[3], b[3], rtol=1e-9)
    np.testing.assert_allclose(a[4], b[4], rtol=1e-9)
    assert np.all(np.isfinite(a[2][1:])) and np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1]))
