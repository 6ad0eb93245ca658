"""-m gpu: glrm_hip_impute / glrm_hip_error_metric against the oracle (same domains, same factors): the rule table on inputs whose dot
products are exact, error_metric on integer data with columns at the 65536-entry chunk boundary, and the refusals."""
import math

import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.domains import pack_domains
from lowrankmodels.jl_amd.losses import enforce_MNLOrdRules
from test_impute import heterogeneous_model

pytestmark = pytest.mark.gpu


def hip():
    return _capi.hip_api()


def test_impute_and_error_metric_match_oracle():
    rng = np.random.default_rng(4)
    losses, X, Y, k = heterogeneous_model(rng, 500)
    m = X.shape[1]
    g0 = L.GLRM(np.ones((m, len(losses))), losses, L.ZeroReg(), L.ZeroReg(), k, X=X, Y=Y)
    A_c = L.impute(g0, engine=O.oracle_api())
    g0.close()
    A_g = L.impute(g0, engine=hip())
    # dots differ in the last bits only; rounding to levels can flip at exact ties, which random data does not produce
    assert np.array_equal(A_c[:, 4:10], A_g[:, 4:10])                          # ordinal / boolean / categorical columns: exact
    np.testing.assert_allclose(A_g, A_c, rtol=1e-12, atol=1e-13)
    I, J = np.nonzero(rng.random(A_c.shape) < 0.7)
    g = L.GLRM(A_c, losses, L.ZeroReg(), L.ZeroReg(), k, obs=(I, J), X=X, Y=Y)
    assert L.error_metric(g, engine=hip()) == 0.0 and L.error_metric(g, standardize=True, engine=hip()) == 0.0   # test/err_test.jl:49
    Xp = X + 0.3 * rng.standard_normal(X.shape)
    for std in (False, True):
        g.close()
        e_c = L.error_metric(g, Xp, Y, standardize=std, engine=O.oracle_api())
        g.close()
        e_g = L.error_metric(g, Xp, Y, standardize=std, engine=hip())
        assert e_g == pytest.approx(e_c, rel=1e-10) and e_c > 0
    doms = [L.default_domain(l) for l in losses]
    doms[0] = L.OrdinalDomain(-3, 3); doms[1] = L.BoolDomain(); doms[7] = L.OrdinalDomain(1, 4)   # non-default pairings
    g.close()
    e_c = L.error_metric(g, Xp, Y, doms, engine=O.oracle_api())
    g.close()
    assert L.error_metric(g, Xp, Y, doms, engine=hip()) == pytest.approx(e_c, rel=1e-10)


def test_long_columns_and_unsupported_pairs():
    rng = np.random.default_rng(8)
    m, n, k = 150000, 3, 5
    A = np.round(rng.standard_normal((m, k)) @ rng.standard_normal((k, n)))
    g = L.GLRM(A, L.QuadLoss(), L.QuadReg(), L.QuadReg(), k, rng=rng)
    doms = [L.OrdinalDomain(-4, 4)] * n
    e_g = L.error_metric(g, domains=doms, standardize=True, engine=hip())     # columns longer than one 65536-entry chunk
    g.close()
    assert e_g == pytest.approx(L.error_metric(g, domains=doms, standardize=True, engine=O.oracle_api()), rel=1e-10)
    gl = L.GLRM(A[:100] > 0, L.LogisticLoss(), L.QuadReg(), L.QuadReg(), 2, rng=rng)
    with pytest.raises(L.GLRMError) as ei:
        L.impute(gl, domains=[L.RealDomain()] * n, engine=hip())
    assert ei.value.code == _capi.ERR_UNSUPPORTED


# ================================================================== the rule table on exact inputs
# Every entry of X and Y is a small multiple of 1/2, so every u = <x_i, y_j> is a multiple of 1/4 far below 2^53: the dot products are
# exact in any order and under any contraction, and whatever differs between the device and the oracle is the RULE, not the sum.
EPS = 1e-9
R, P, B = L.RealDomain(), L.PeriodicDomain(2.5), L.BoolDomain()
ORDS = [L.OrdinalDomain(1, 7), L.OrdinalDomain(-3, 3), L.OrdinalDomain(0, 3), L.OrdinalDomain(2, 3), L.CountDomain(3), L.CountDomain(12)]
DIFF = [L.QuadLoss(), L.L1Loss(2.0), L.HuberLoss(), L.QuantileLoss(quantile=0.3), L.PeriodicLoss(2.5)]
OH, LG, WH = L.OrdinalHingeLoss(1, 10), L.LogisticLoss(), L.WeightedHingeLoss(1.0, case_weight_ratio=2.0)
HINGE = L.HingeLoss

# rules that decide without exp / log / cos: the device must return the oracle's matrix bit for bit (+-inf included: 1 / u at u = +-0)
EXACT = ([(D, l) for D in [R, P] + ORDS for l in DIFF + [OH, WH]]                                   # DiffLoss, OrdinalHinge, WeightedHinge rules
         + [(D, LG) for D in [B] + ORDS]                                                            # Logistic on Bool and on Ordinal / Count
         + [(B, l) for l in [WH, L.QuadLoss(), L.L1Loss(2.0), L.HuberLoss(), L.QuantileLoss(quantile=0.3), OH]]   # Bool through evaluate
         + [(L.CategoricalDomain(4), L.MultinomialLoss(4)), (L.CategoricalDomain(3), L.OvALoss(3)), (L.CategoricalDomain(4), L.OvALoss(4, bin_loss=HINGE())),
            (L.CategoricalDomain(2), L.MultinomialLoss(2)), (L.CategoricalDomain(32), L.OvALoss(32)), (L.CategoricalDomain(32), L.MultinomialLoss(32))]  # argmax
         + [(L.OrdinalDomain(1, 4), L.OrdisticLoss(4)), (L.OrdinalDomain(-3, 3), L.OrdisticLoss(4)), (L.CountDomain(3), L.OrdisticLoss(2)),
            (L.OrdinalDomain(1, 32), L.OrdisticLoss(32))]                                            # argmin(u.^2)
         + [(D, L.OvALoss(3, bin_loss=HINGE())) for D in ORDS] + [(D, L.BvSLoss(4, bin_loss=HINGE())) for D in ORDS]   # generic ordinal, hinge
         + [(L.OrdinalDomain(-3, 3), L.OvALoss(2, bin_loss=HINGE())), (L.OrdinalDomain(1, 32), L.OvALoss(32, bin_loss=HINGE())),
            (L.OrdinalDomain(-3, 3), L.OvALoss(32, bin_loss=HINGE())), (L.OrdinalDomain(1, 33), L.BvSLoss(33, bin_loss=HINGE())),
            (L.CountDomain(3), L.BvSLoss(33, bin_loss=HINGE()))])


def half_ints(rng, shape, r=4):
    return rng.integers(-r, r + 1, shape) / 2.0


def factors(rng, m, k, d):
    X = np.asfortranarray(half_ints(rng, (k, m)))
    X[:, 3::7] = 0.0                                   # zero rows of X: u = 0 in every column
    return X, np.asfortranarray(half_ints(rng, (k, d)))


def table_model(pairs, m, k, seed):
    losses = [l for _, l in pairs]
    X, Y = factors(np.random.default_rng(seed), m, k, L.embedding_dim(losses))
    g = L.GLRM(np.ones((m, len(losses))), losses, L.ZeroReg(), L.ZeroReg(), k, X=X, Y=Y)
    return g, X, Y, pack_domains([D for D, _ in pairs])


def impute_on(api, pa, X, Y, doms):
    h = api.create(pa)
    try:
        return api.impute(h, X, Y, doms, pa.m, pa.n)
    finally:
        api.destroy(h)


@pytest.mark.parametrize("m,k", [(1, 1), (127, 5), (128, 33), (129, 1), (300, 5)])
def test_rule_table_without_transcendentals_is_exact(m, k):
    """Every (domain, loss) pair whose rule is comparisons, rounding and IEEE division: array_equal with the oracle, ties, half-integers, u = 0
    and the ordinal domains with negative / zero / raised minimum included.  m straddles the 128-thread block, k = 1 / 5 / 33 pads the rank
    differently, the vector columns have d = 2 ... 32 (GLRM_MAX_EMBEDDING_DIM)."""
    g, X, Y, doms = table_model(EXACT, m, k, seed=100 + m)
    pa = g.problem_arrays()
    assert len(pa.losses) == len(EXACT)                                         # a loss per column
    A_c, A_g = impute_on(O.oracle_api(), pa, X, Y, doms), impute_on(hip(), pa, X, Y, doms)
    U = X.T @ Y
    if m >= 127:                                                                # the inputs do present what the test is about
        assert (U == 0).any() and (np.abs(U % 1.0) == 0.5).any() and np.isinf(A_c).any()
    bad = np.argwhere(A_c != A_g)
    assert bad.size == 0, [(EXACT[f], int(i), A_c[i, f], A_g[i, f]) for i, f in bad[:5]]
    assert np.array_equal(A_c, A_g)


@pytest.mark.parametrize("pair,m,n,k", [((L.OrdinalDomain(-3, 3), L.OvALoss(2, bin_loss=HINGE())), 1, 1, 1),
                                        ((L.OrdinalDomain(-3, 3), L.OvALoss(32, bin_loss=HINGE())), 300, 3, 5),
                                        ((L.CategoricalDomain(32), L.MultinomialLoss(32)), 129, 1, 33),
                                        ((L.OrdinalDomain(1, 4), L.OrdisticLoss(4)), 127, 2, 1)],
                         ids=["ova2-hinge-m1-n1-k1", "ova32-hinge-m300-n3-k5", "multinomial32-m129-n1-k33", "ordistic4-m127-n2-k1"])
def test_single_loss_vector_models_are_exact(pair, m, n, k):
    """n_losses == 1 with a vector loss: column f reads Y[:, f d : (f + 1) d] (the other indexing of ystart); n = 1 and m = 1 included."""
    g, X, Y, doms = table_model([pair] * n, m, k, seed=7 + m)
    pa = g.problem_arrays()
    assert len(pa.losses) == 1
    A_c, A_g = impute_on(O.oracle_api(), pa, X, Y, doms), impute_on(hip(), pa, X, Y, doms)
    assert np.array_equal(A_c, A_g)
    if n > 1:
        assert not np.array_equal(A_c[:, 0], A_c[:, 1])                         # the columns do read different blocks of Y


# ---------------------------------------------------------------- rules that decide through exp / log / cos
# Device exp and log are good to ~1e-16 relative, so a decision whose candidates are 1e-9 apart is the same on both sides.  The test first
# PROVES that about its own inputs, entry by entry, with the mirror on the CPU; then it asks for exact equality.
PER = L.PeriodicLoss(161 / 64)   # Bool + PeriodicLoss ties where u = 1/2 + j T / 2: with this T no other multiple of 1/4 below 40 does
MNLO = [(L.OrdinalDomain(1, 5), L.MultinomialOrdinalLoss(5)), (L.OrdinalDomain(-3, 3), L.MultinomialOrdinalLoss(5)), (L.CountDomain(3), L.MultinomialOrdinalLoss(3)),
        (L.OrdinalDomain(1, 33), L.MultinomialOrdinalLoss(33))]
# generic ordinal rule with logistic bin losses / MultinomialLoss.  Two levels whose costs are the same terms in ANOTHER ORDER (u_a == u_b under
# OvALoss) tie in exact arithmetic and differ in the last bit of a sum: such inputs decide nothing about the rule, and random multiples of 1/2
# produce them in every few rows.  These columns therefore get Y[:, block] = w c': u_j = c_j <x, w> with distinct c_j (distinct partial sums
# for BvSLoss), so levels either differ by at least 1/8 or (x orthogonal to w, zero rows) every u_j is 0 and every level's terms are identical
GENERIC = ([(D, L.OvALoss(3)) for D in ORDS] + [(D, L.BvSLoss(5)) for D in ORDS]
           + [(L.OrdinalDomain(1, 4), L.MultinomialLoss(4)), (L.OrdinalDomain(2, 3), L.MultinomialLoss(4)), (L.OrdinalDomain(-3, 3), L.OvALoss(2)),
              (L.OrdinalDomain(-3, 3), L.OvALoss(32)), (L.OrdinalDomain(1, 33), L.BvSLoss(33)), (L.OrdinalDomain(1, 32), L.MultinomialLoss(32))])
POISSON = [(D, L.PoissonLoss(20)) for D in ORDS + [L.CountDomain(20)]]
BOOL_T = [(B, L.PoissonLoss(20)), (B, PER)]
REAL_POISSON = [(R, L.PoissonLoss(20)), (P, L.PoissonLoss(20))]
TRANS = POISSON + BOOL_T + MNLO + GENERIC + REAL_POISSON
TRANS_SEED = 1   # chosen on the CPU: every entry passes `decided` below


def apart(a, b):
    return abs(a - b) > EPS * max(1.0, abs(a), abs(b))


def same_terms(loss, u, a, b):
    """Levels a and b cost the same terms in the same order: equal on any machine (log(1 + exp(-0.0)) and log(1 + exp(0.0)) are one value)."""
    j = np.arange(len(u)) + 1
    if isinstance(loss, L.OvALoss):
        return np.array_equal(np.where(a == j, -u, u), np.where(b == j, -u, u))
    if isinstance(loss, L.BvSLoss):
        return np.array_equal(np.where(a > j, -u, u), np.where(b > j, -u, u))
    return u[a - 1] == u[b - 1]                                                  # MultinomialLoss: the level enters through u[a] alone


def decided(D, loss, u):
    """The reference's choice at u does not hang on the last bits of exp / log / cos."""
    if isinstance(D, L.CountDomain):
        D = L.OrdinalDomain(0, D.max_count)
    if isinstance(loss, L.PoissonLoss) and isinstance(D, L.OrdinalDomain):       # roundcutoff(exp(u), min, max)
        e = math.exp(u)
        h = math.floor(e) + 0.5                                                  # the half-integer next to exp(u)
        return abs(e - h) > EPS * e or h < D.min or h > D.max                    # (outside the bounds both sides of it are cut off alike)
    if isinstance(D, L.BoolDomain):                                              # evaluate(l, u, false) < evaluate(l, u, true)
        exact_tie = isinstance(loss, L.PeriodicLoss) and (0 - u) == -(1 - u)     # cos(-w) and cos(w)
        return exact_tie or apart(loss.evaluate(u, False), loss.evaluate(u, True))
    if isinstance(loss, L.MultinomialOrdinalLoss):
        eu = np.exp(enforce_MNLOrdRules(u))
        p = np.concatenate([[1 - eu[0]], -np.diff(eu), [eu[-1]]])
        b = int(np.argmax(p))
        return all(p[b] - p[j] > EPS for j in range(len(p)) if j != b)
    levels = list(range(D.min, D.max + 1))
    vals = [loss.evaluate(u, a) for a in levels]
    b = int(np.argmin(vals))
    return all(apart(vals[i], vals[b]) or same_terms(loss, u, a, levels[b]) for i, a in enumerate(levels) if i != b)


def trans_model(m=129, k=5):
    g, X, Y, doms = table_model(TRANS, m, k, seed=TRANS_SEED)
    rng = np.random.default_rng(TRANS_SEED + 1000)
    for (D, l), (y0, y1) in zip(TRANS, L.get_yidxs(g.losses)):
        d = y1 - y0
        if (D, l) in GENERIC:
            j = np.arange(d)
            c = (-1.0) ** j * (j + 1) / 2 if isinstance(l, L.BvSLoss) else rng.permutation(j - d // 2) / 2.0
            Y[:, y0:y1] = np.outer(half_ints(rng, k), c)
        if isinstance(D, L.BoolDomain) and isinstance(l, L.PoissonLoss):
            Y[:, y0:y1] *= 1.5       # evaluate(false) and evaluate(true) cross at u = -1: multiples of 3/8 never land there
    return g, X, Y, doms


def assert_decided(pairs, losses, U):
    """The condition on the test's own inputs: every entry of every deciding column, none left out."""
    for (D, l), (y0, y1) in zip(pairs, L.get_yidxs(losses)):
        for i in range(U.shape[0]):
            assert decided(D, l, U[i, y0:y1] if y1 - y0 > 1 else float(U[i, y0])), (D, l, i, U[i, y0:y1])


def test_rule_table_with_transcendentals_is_exact_where_the_inputs_decide():
    g, X, Y, doms = trans_model()
    pa = g.problem_arrays()
    U = X.T @ Y
    assert np.abs(U).max() < 2 ** 20 and (U == 0).any()
    n_dec = len(TRANS) - len(REAL_POISSON)
    assert_decided(TRANS[:n_dec], g.losses, U)
    A_c, A_g = impute_on(O.oracle_api(), pa, X, Y, doms), impute_on(hip(), pa, X, Y, doms)
    bad = np.argwhere(A_c[:, :n_dec] != A_g[:, :n_dec])
    assert bad.size == 0, [(TRANS[f], int(i), A_c[i, f], A_g[i, f]) for i, f in bad[:5]]
    np.testing.assert_allclose(A_g[:, n_dec:], A_c[:, n_dec:], rtol=1e-12, atol=0)      # exp(u) itself
    for f in range(n_dec):                                                      # the rules were exercised: no column is one constant
        assert len(np.unique(A_c[:, f])) > 1, TRANS[f]


FREE_SEED = 1   # chosen on the CPU (seeds 1, 16 and 20 of the first 21 pass `decided` in every entry)


def test_generic_ordinal_with_transcendentals_on_unstructured_factors():
    """The same rules with Y drawn like everywhere else, u_j unrelated to each other: few rows and k = 33 (|u| up to 132 in steps of 1/4),
    so that a seed exists under which no entry ties two levels through terms in another order."""
    pairs = [p for p in GENERIC if p[1].embedding_dim <= 5]
    g, X, Y, doms = table_model(pairs, 24, 33, seed=FREE_SEED)
    pa = g.problem_arrays()
    assert_decided(pairs, g.losses, X.T @ Y)
    A_c, A_g = impute_on(O.oracle_api(), pa, X, Y, doms), impute_on(hip(), pa, X, Y, doms)
    bad = np.argwhere(A_c != A_g)
    assert bad.size == 0, [(pairs[f], int(i), A_c[i, f], A_g[i, f]) for i, f in bad[:5]]


# ================================================================== error_metric on integer data
CHUNK = 65536   # entries of a column one workgroup row of error_metric_kernel covers


@pytest.fixture(scope="module")
def chunk_model():
    """m = 131072, k = 2, QuadLoss / RealDomain, integer A, X and Y; column lengths 65535, 65536, 65537, 131072, 1 and 0 (one chunk less one,
    exactly one, one more, exactly two, a single entry, none).  Every term (u - a)^2 is an integer, so the sums are free of order."""
    m, k, lens = 2 * CHUNK, 2, [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 1, 0]
    rng = np.random.default_rng(65536)
    A = rng.integers(-9, 10, (m, len(lens))).astype(np.float64)
    X, Y = np.asfortranarray(rng.integers(-3, 4, (k, m)).astype(np.float64)), np.asfortranarray(rng.integers(-3, 4, (k, len(lens))).astype(np.float64))
    I = np.concatenate([np.sort(rng.choice(m, n_f, replace=False)) for n_f in lens])
    J = np.repeat(np.arange(len(lens)), lens)
    return A, X, Y, I, J, lens


def metric_on(api, pa, X, Y, doms, standardize):
    h = api.create(pa)
    try:
        return api.error_metric(h, X, Y, doms, standardize)
    finally:
        api.destroy(h)


def test_error_metric_at_the_chunk_boundaries_is_exact(chunk_model):
    A, X, Y, I, J, lens = chunk_model
    g = L.GLRM(A, L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 2, obs=(I, J), X=X, Y=Y)
    pa = g.problem_arrays()
    assert np.diff(pa.colptr).tolist() == lens
    doms = pack_domains([R] * len(lens))
    want = float(np.sum(((X.T @ Y)[I, J] - A[I, J]) ** 2))
    assert want > 0 and want < 2 ** 53
    e_c, e_g = metric_on(O.oracle_api(), pa, X, Y, doms, False), metric_on(hip(), pa, X, Y, doms, False)
    assert e_c == want and e_g == want                                          # one lost or doubled entry moves it by an integer
    # the empty column: 0 / 0 in the reference's column mean
    assert math.isnan(metric_on(O.oracle_api(), pa, X, Y, doms, True)) and math.isnan(metric_on(hip(), pa, X, Y, doms, True))
    # without it
    keep = J < 5
    g5 = L.GLRM(A[:, :5], L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 2, obs=(I[keep], J[keep]), X=X, Y=Y[:, :5])
    pa5, Y5, doms5 = g5.problem_arrays(), np.asfortranarray(Y[:, :5]), pack_domains([R] * 5)
    assert metric_on(hip(), pa5, X, Y5, doms5, False) == want                   # (the sixth column held nothing)
    s_c, s_g = metric_on(O.oracle_api(), pa5, X, Y5, doms5, True), metric_on(hip(), pa5, X, Y5, doms5, True)
    assert s_c > 0 and s_g == pytest.approx(s_c, rel=1e-10)                     # one lost entry moves it by ~1e-5


def test_error_metric_periodic_bool_and_categorical_are_exact():
    """PeriodicDomain: (pos_mod(T, imputed) - pos_mod(T, a))^2 with imputed values 0, negative and multiples of T -- multiples of 1/4 throughout,
    so exact; BoolDomain / CategoricalDomain: misclassification counts.  == against the oracle and against the mirror, entry by entry."""
    T = 2.5
    pairs = [(L.PeriodicDomain(T), L.QuadLoss()), (L.PeriodicDomain(T), L.PeriodicLoss(T)), (B, L.LogisticLoss()), (B, L.QuadLoss()),
             (L.CategoricalDomain(4), L.MultinomialLoss(4)), (L.CategoricalDomain(3), L.OvALoss(3, bin_loss=HINGE()))]
    m, k = 200, 2
    rng = np.random.default_rng(25)
    losses = [l for _, l in pairs]
    X, Y = factors(rng, m, k, L.embedding_dim(losses))
    A = np.stack([rng.choice([0.0, -T, T, 2 * T, -2 * T, -1.0, 1.25, 3.75, -0.25], m), rng.integers(-12, 13, m) / 4.0, rng.integers(0, 2, m),
                  rng.integers(0, 2, m), rng.integers(1, 5, m), rng.integers(1, 4, m)], axis=1).astype(np.float64)
    I, J = np.nonzero(rng.random(A.shape) < 0.7)
    g = L.GLRM(A, losses, L.ZeroReg(), L.ZeroReg(), k, obs=(I, J), X=X, Y=Y)
    pa, doms = g.problem_arrays(), pack_domains([D for D, _ in pairs])
    U = X.T @ Y
    u0 = U[I[J == 0], 0]
    assert (u0 == 0).any() and (u0 < 0).any() and ((u0 != 0) & (u0 % T == 0)).any()
    spans = L.get_yidxs(losses)
    terms = [L.error_metric_entry(pairs[j][0], losses[j], U[i, spans[j][0]:spans[j][1]] if losses[j].embedding_dim > 1 else float(U[i, spans[j][0]]), A[i, j])
             for i, j in zip(I, J)]
    want = float(np.sum(terms))
    assert all(t * 16 == int(t * 16) for t in terms) and want > 0
    assert metric_on(O.oracle_api(), pa, X, Y, doms, False) == want and metric_on(hip(), pa, X, Y, doms, False) == want
    s_c = metric_on(O.oracle_api(), pa, X, Y, doms, True)
    assert metric_on(hip(), pa, X, Y, doms, True) == pytest.approx(s_c, rel=1e-10)


# ================================================================== refusals
def refused(code, fn, *args):
    with pytest.raises(L.GLRMError) as ei:
        fn(*args)
    assert ei.value.code == code, ei.value


UNSUPPORTED_PAIRS = [("real-logistic", R, L.LogisticLoss()), ("categorical-scalar", L.CategoricalDomain(4), L.QuadLoss()),
                     ("categorical-bvs", L.CategoricalDomain(4), L.BvSLoss(4)), ("bool-vector", B, L.OvALoss(3)),
                     ("ordinal-0-d-multinomial", L.OrdinalDomain(0, 4), L.MultinomialLoss(4)),
                     ("ordinal-1-d+1-multinomial", L.OrdinalDomain(1, 5), L.MultinomialLoss(4))]


@pytest.mark.parametrize("name,D,loss", UNSUPPORTED_PAIRS, ids=[p[0] for p in UNSUPPORTED_PAIRS])
def test_one_unsupported_column_among_supported_ones_is_refused(name, D, loss):
    """A pair the reference has no rule for (or throws on) fails the whole call with ERR_UNSUPPORTED, in impute and in error_metric; the handle
    serves the next call."""
    pairs = [(R, L.QuadLoss()), (L.CategoricalDomain(3), L.OvALoss(3)), (D, loss), (L.OrdinalDomain(1, 7), L.HuberLoss())]
    g, X, Y, doms = table_model(pairs, 130, 3, seed=5)
    pa = g.problem_arrays()
    good = pack_domains([R, L.CategoricalDomain(3), L.default_domain(loss), L.OrdinalDomain(1, 7)])
    want = impute_on(O.oracle_api(), pa, X, Y, good)
    refused(_capi.ERR_UNSUPPORTED, impute_on, O.oracle_api(), pa, X, Y, doms)   # the oracle refuses the same pairs
    api = hip()
    h = api.create(pa)
    try:
        refused(_capi.ERR_UNSUPPORTED, api.impute, h, X, Y, doms, g.m, g.n)
        refused(_capi.ERR_UNSUPPORTED, api.error_metric, h, X, Y, doms, False)
        refused(_capi.ERR_UNSUPPORTED, api.error_metric, h, X, Y, doms, True)
        assert np.array_equal(api.impute(h, X, Y, good, g.m, g.n), want)
    finally:
        api.destroy(h)


def test_handles_and_descriptors_post_fit_evaluation_refuses():
    rng = np.random.default_rng(9)
    m, n, k = 64, 48, 16
    A = rng.integers(-4, 5, (m, n)).astype(np.float64)
    g = L.GLRM(A, L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), k, X=half_ints(rng, (k, m)), Y=half_ints(rng, (k, n)))
    X, Y, doms = np.asfortranarray(g.X), np.asfortranarray(g.Y), pack_domains([R] * n)
    pa = g.problem_arrays()
    want = impute_on(O.oracle_api(), pa, X, Y, doms)
    api = hip()

    def both_refused(code, h, d=doms):
        refused(code, api.impute, h, X, Y, d, m, n)
        refused(code, api.error_metric, h, X, Y, d, False)

    handles = []
    try:
        dense = api.create(g.problem_arrays(dense=True))                          # the matrix hand-over keeps no lists
        handles.append(dense)
        both_refused(_capi.ERR_UNSUPPORTED, dense)
        Xd, Yd = X.copy(order="F"), Y.copy(order="F")
        assert np.isfinite(api.objective(dense, Xd, Yd, True))                    # still usable
        shard = api.create(g.problem_arrays(rows=(0, 32)), defer=True)            # one shard of a sharded fit, set up
        handles.append(shard)
        api.finalize(shard, api.signature(shard))
        both_refused(_capi.ERR_INVALID, shard)
        assert api.kernel_stats(shard)["nnz_rows"] == 32 * n
        deferred = api.create(pa, defer=True)                                     # uploaded, not finalized
        handles.append(deferred)
        both_refused(_capi.ERR_INVALID, deferred)
        api.finalize(deferred, api.signature(deferred))
        assert np.array_equal(api.impute(deferred, X, Y, doms, m, n), want)       # finalized, it serves
        f32 = api.create(pa, storage=_capi.STORAGE_F32)
        handles.append(f32)
        both_refused(_capi.ERR_UNSUPPORTED, f32)
        assert api.objective(f32, X, Y, True) == api.objective(deferred, X, Y, True)   # half-multiples narrow to float exactly
        for field, value in (("kind", 6), ("kind", -1), ("reserved", 1)):
            d = doms.copy()
            d[n // 2][field] = value
            both_refused(_capi.ERR_INVALID, deferred, d)
            refused(_capi.ERR_INVALID, impute_on, O.oracle_api(), pa, X, Y, d)
        assert np.array_equal(api.impute(deferred, X, Y, doms, m, n), want)
        assert api.error_metric(deferred, X, Y, doms, False) == float(np.sum((X.T @ Y - A) ** 2))
    finally:
        for h in handles:
            api.destroy(h)
