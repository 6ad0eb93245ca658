"""impute / error_metric (src/impute_and_err.jl, src/evaluate_fit.jl:107-168): oracle vs the Python mirrors entry by entry, the
reference's own consistency property (test/err_test.jl:33-51: data imputed from a low-rank model has error_metric == 0 at that
model), and the model-level functions on the oracle engine."""
import math

import numpy as np
import pytest

import cases
import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd.domains import pos_mod

SCALAR = [L.QuadLoss(), L.L1Loss(2.0), L.HuberLoss(), L.QuantileLoss(quantile=0.3), L.PeriodicLoss(2.5), L.PoissonLoss(20),
          L.OrdinalHingeLoss(1, 10), L.LogisticLoss(), L.WeightedHingeLoss(1.0, case_weight_ratio=2.0)]
VECTOR = [L.MultinomialLoss(4), L.OvALoss(3), L.OvALoss(4, bin_loss=L.HingeLoss()), L.BvSLoss(5), L.OrdisticLoss(4), L.MultinomialOrdinalLoss(5)]
DOMAINS = [L.RealDomain(), L.BoolDomain(), L.OrdinalDomain(1, 7), L.PeriodicDomain(2.5), L.CountDomain(12), L.CategoricalDomain(4)]


def test_known_answers():
    assert L.impute_entry(L.RealDomain(), L.QuadLoss(), 1.7) == 1.7
    assert L.impute_entry(L.OrdinalDomain(1, 5), L.QuadLoss(), 7.2) == 5 and L.impute_entry(L.OrdinalDomain(1, 5), L.QuadLoss(), 2.5) == 2  # half to even
    assert L.impute_entry(L.BoolDomain(), L.LogisticLoss(), 0.0) is True and L.impute_entry(L.BoolDomain(), L.LogisticLoss(), -0.1) is False
    assert L.impute_entry(L.BoolDomain(), L.QuadLoss(), 0.6) is True and L.impute_entry(L.BoolDomain(), L.QuadLoss(), 0.4) is False
    assert L.impute_entry(L.CountDomain(10), L.PoissonLoss(10), math.log(3.4)) == 3
    assert L.impute_entry(L.CategoricalDomain(3), L.MultinomialLoss(3), [0.1, 2.0, -1.0]) == 2
    assert L.impute_entry(L.OrdinalDomain(1, 3), L.MultinomialOrdinalLoss(3), [-0.1, -3.0]) == 2   # p = [1-e^-.1, e^-.1 - e^-3, e^-3]
    assert L.impute_entry(L.OrdinalDomain(1, 4), L.BvSLoss(4), [2.0, 1.0, -1.0]) == 3               # two thresholds passed
    assert L.error_metric_entry(L.PeriodicDomain(2.0), L.PeriodicLoss(2.0), 0.5, 2.5) == pytest.approx(0.0, abs=1e-30)
    assert L.error_metric_entry(L.BoolDomain(), L.LogisticLoss(), 0.3, True) == 0.0 and L.error_metric_entry(L.BoolDomain(), L.LogisticLoss(), 0.3, False) == 1.0
    with pytest.raises(ValueError):
        L.impute_entry(L.RealDomain(), L.LogisticLoss(), 0.3)


@pytest.mark.parametrize("loss", SCALAR + VECTOR, ids=lambda l: repr(l))
def test_oracle_impute_matches_python_mirror(loss):
    rng = np.random.default_rng(3)
    for dom in DOMAINS + [L.default_domain(loss)]:
        for _ in range(25):
            u = rng.standard_normal(loss.embedding_dim) * 2.0 if loss.embedding_dim > 1 else float(rng.standard_normal() * 3)
            try:
                ref = L.impute_entry(dom, loss, u)
            except (TypeError, ValueError):
                with pytest.raises(TypeError):
                    O.impute_entry(dom, loss, u)
                break
            assert O.impute_entry(dom, loss, u) == pytest.approx(float(ref), rel=1e-13)


# ---------------------------------------------------------------- the rule table at ties and edges, oracle vs mirror, exactly
# u: every multiple of 1/2 in [-8, 13] (11.5 and 12.5 straddle CountDomain(12)), both zeros, +-1/4 and values far beyond every bound
U_SCALAR = [i / 2 for i in range(-16, 27)] + [0.0, -0.0, 0.25, -0.25, 100.0, -100.0]
EDGE_DOMAINS = [L.OrdinalDomain(-3, 3), L.OrdinalDomain(0, 3), L.OrdinalDomain(2, 3), L.CountDomain(3)]
EDGE_VECTOR = [L.OvALoss(2, bin_loss=L.HingeLoss()), L.OvALoss(32, bin_loss=L.HingeLoss()), L.BvSLoss(3, bin_loss=L.HingeLoss()),
               L.BvSLoss(33, bin_loss=L.HingeLoss()), L.OvALoss(32), L.BvSLoss(33), L.MultinomialLoss(2), L.MultinomialLoss(32),
               L.OrdisticLoss(32), L.MultinomialOrdinalLoss(33)]


def u_grid(loss, seed=0):
    """The u values one loss is tried at.  Vector losses: constant vectors (every level ties), signed zeros, and draws of multiples of
    1/2 from a range so narrow that the maximum, the minimum and the squares tie in most of them."""
    d = loss.embedding_dim
    if d == 1:
        return U_SCALAR
    rng = np.random.default_rng(seed)
    out = [np.full(d, c) for c in (0.0, -0.0, 0.5, -0.5, -1.0, 100.0, -100.0)]
    out += [np.where(np.arange(d) % 2 == 0, 0.0, -0.0), np.arange(d) / 2.0, -np.arange(d) / 2.0, np.arange(d)[::-1] / 2.0 - 1.0]
    out += [rng.integers(-r, r + 1, d) / 2.0 for r in (1, 2, 6) for _ in range(12 if d <= 8 else 6)]
    return out


def both(fn_ref, fn_oracle):
    """The value, or 'raised', from each side: the reference throws for pairs without a rule and so must the oracle.  NaN (pos_mod of an
    infinite imputed value) is written as a string so that it compares equal to itself."""
    out = []
    for fn, errs in ((fn_ref, (TypeError, ValueError)), (fn_oracle, (TypeError,))):
        try:
            v = float(fn())
            out.append("nan" if math.isnan(v) else v)
        except errs:
            out.append("raised")
    return out


def loss_id(l):
    b = getattr(l, "bin_loss", None)
    return repr(l) + ("" if b is None or isinstance(b, L.LogisticLoss) else "-hinge")


@pytest.mark.parametrize("loss", SCALAR + VECTOR + EDGE_VECTOR, ids=loss_id)
def test_oracle_rule_table_matches_mirror_exactly_at_ties_and_edges(loss):
    """impute(D, l, u) and error_metric(D, l, u, a) of the oracle against the Python mirror on a grid made of ties, half-integers (round
    half to even), signed zeros and out-of-range values: the same value bit for bit, or both refuse."""
    doms = DOMAINS + [L.default_domain(loss)] + EDGE_DOMAINS
    if loss.embedding_dim > 1:
        doms += [L.OrdinalDomain(1, loss.embedding_dim), L.OrdinalDomain(1, loss.embedding_dim + 1), L.OrdinalDomain(0, loss.embedding_dim),
                 L.CategoricalDomain(loss.embedding_dim)]
    n = 0
    for dom in doms:
        for u in u_grid(loss):
            ref, got = both(lambda: L.impute_entry(dom, loss, u), lambda: O.impute_entry(dom, loss, u))
            assert ref == got, (dom, loss, u, ref, got)
            for a in (0.0, 1.0, 3.0, -2.5, 5.0):
                ref, got = both(lambda: L.error_metric_entry(dom, loss, u, a), lambda: O.error_metric_entry(dom, loss, u, a))
                assert ref == got, (dom, loss, u, a, ref, got)
            n += 1
    assert n == len(doms) * len(u_grid(loss))


@pytest.mark.parametrize("loss", [L.MultinomialLoss(4), L.MultinomialLoss(2), L.MultinomialLoss(32)], ids=repr)
def test_multinomial_levels_outside_1_to_d_raise(loss):
    """The generic ordinal rule evaluates MultinomialLoss at every level of the domain, and evaluate indexes u[a]: a BoundsError in the
    reference for a level below 1 or above d, whatever u is."""
    d = loss.embedding_dim
    for dom in (L.OrdinalDomain(0, d), L.OrdinalDomain(1, d + 1), L.OrdinalDomain(-3, 3), L.OrdinalDomain(d + 1, d + 2), L.CountDomain(d)):
        for u in u_grid(loss)[:8]:
            with pytest.raises(TypeError):
                L.impute_entry(dom, loss, u)
            with pytest.raises(TypeError):
                O.impute_entry(dom, loss, u)
    for u in u_grid(loss)[:8]:
        assert L.impute_entry(L.OrdinalDomain(1, d), loss, u) == O.impute_entry(L.OrdinalDomain(1, d), loss, u)


@pytest.mark.parametrize("impute_entry", [L.impute_entry, O.impute_entry], ids=["mirror", "oracle"])
def test_known_answers_at_ties_and_edges(impute_entry):
    """Worked out by hand from src/impute_and_err.jl, for the mirror and for the oracle."""
    inf = math.inf
    # generic ordinal rule (:100-102): (D.min:D.max)[argmin(...)] is the FIRST minimum.  OvALoss tells no level below 1 from another (a == j
    # never holds) and each level j >= 1 costs u_j less than those: with every u_j < 0 the levels -3..0 tie for the minimum -> -3
    for lo in (L.OvALoss(3), L.OvALoss(3, bin_loss=L.HingeLoss())):
        assert impute_entry(L.OrdinalDomain(-3, 3), lo, [-1.0, -1.0, -1.0]) == -3
        assert impute_entry(L.OrdinalDomain(0, 3), lo, [-1.0, -1.0, -1.0]) == 0
        assert impute_entry(L.OrdinalDomain(-3, 3), lo, [-1.0, 2.0, 0.5]) == 2
        assert impute_entry(L.OrdinalDomain(2, 3), lo, [3.0, -1.0, -1.0]) == 2   # levels 2 and 3 tie; level 1 is outside the domain
    # BvSLoss: a > j is false for every j at each level <= 1, so -3..1 tie
    for lo in (L.BvSLoss(4), L.BvSLoss(4, bin_loss=L.HingeLoss())):
        assert impute_entry(L.OrdinalDomain(-3, 3), lo, [-1.0, -1.0, -1.0]) == -3
        assert impute_entry(L.OrdinalDomain(-3, 3), lo, [2.0, 1.0, -1.0]) == 3
        assert impute_entry(L.CountDomain(3), lo, [-1.0, -1.0, -1.0]) == 0
    # roundcutoff (:30): round half to even, then the bounds
    D = L.OrdinalDomain(-3, 3)
    for u, want in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (3.5, 3), (-3.5, -3), (100.0, 3), (-100.0, -3)):
        assert impute_entry(D, L.QuadLoss(), u) == want and impute_entry(D, L.OrdinalHingeLoss(1, 10), u) == want
    assert impute_entry(L.RealDomain(), L.OrdinalHingeLoss(1, 10), 0.5) == 1 and impute_entry(L.RealDomain(), L.OrdinalHingeLoss(1, 10), 10.5) == 10
    assert impute_entry(L.RealDomain(), L.OrdinalHingeLoss(1, 10), 2.5) == 2 and impute_entry(L.RealDomain(), L.OrdinalHingeLoss(1, 10), 3.5) == 4
    assert impute_entry(L.CountDomain(12), L.QuadLoss(), 11.5) == 12 and impute_entry(L.CountDomain(12), L.QuadLoss(), 12.5) == 12
    assert impute_entry(L.CountDomain(12), L.QuadLoss(), -0.5) == 0 and impute_entry(L.CountDomain(12), L.PoissonLoss(12), 0.0) == 1
    # BoolDomain through evaluate (:63): false only when strictly better, so the tie at u = 1/2 imputes true
    assert impute_entry(L.BoolDomain(), L.QuadLoss(), 0.5) == 1 and impute_entry(L.BoolDomain(), L.L1Loss(), 0.5) == 1
    assert impute_entry(L.BoolDomain(), L.QuadLoss(), 0.25) == 0 and impute_entry(L.BoolDomain(), L.HuberLoss(), 0.5) == 1
    # OrdinalDomain + LogisticLoss (:76): u > 0 ? max : min
    assert impute_entry(L.OrdinalDomain(2, 7), L.LogisticLoss(), 0.0) == 2 and impute_entry(L.OrdinalDomain(2, 7), L.LogisticLoss(), -0.0) == 2
    assert impute_entry(L.OrdinalDomain(2, 7), L.LogisticLoss(), 0.25) == 7
    # WeightedHingeLoss: 1/u on the reals (:46-49), u >= 0 on Bool (:60), ceil / floor of 1/u then roundcutoff on ordinals (:77-81)
    wh = L.WeightedHingeLoss(1.0, case_weight_ratio=2.0)
    for u, real, boolean, ordinal in ((0.0, inf, 1, 3), (-0.0, -inf, 1, -3), (0.25, 4.0, 1, 3), (-0.5, -2.0, 0, -2)):
        assert impute_entry(L.RealDomain(), wh, u) == real and impute_entry(L.PeriodicDomain(2.5), wh, u) == real
        assert impute_entry(L.BoolDomain(), wh, u) == boolean
        assert impute_entry(L.OrdinalDomain(-3, 3), wh, u) == ordinal
    assert impute_entry(L.OrdinalDomain(1, 7), wh, 0.25) == 4 and impute_entry(L.OrdinalDomain(1, 7), wh, 0.375) == 3   # ceil(8/3)


@pytest.mark.parametrize("err", [L.error_metric_entry, O.error_metric_entry], ids=["mirror", "oracle"])
def test_pos_mod_known_answers(err):
    """pos_mod(T, x) = x > 0 ? x % T : (x % T) + T (:127): 0 and the negative multiples of T map to T, the positive ones to 0."""
    T = 2.5
    for x, want in ((0.0, T), (-0.0, T), (-1.0, 1.5), (-2.5, T), (-5.0, T), (-6.0, 1.5), (2.5, 0.0), (5.0, 0.0), (3.5, 1.0), (1.0, 1.0)):
        assert pos_mod(T, x) == want
    D, q = L.PeriodicDomain(T), L.QuadLoss()
    assert err(D, q, 0.0, 2.5) == T * T            # (pos_mod(0) - pos_mod(T))^2 = (T - 0)^2
    assert err(D, q, -5.0, 0.0) == 0.0 and err(D, q, -5.0, 5.0) == T * T and err(D, q, 5.0, 2.5) == 0.0
    assert err(D, q, -1.0, 1.5) == 0.0 and err(D, q, -6.0, 3.5) == 0.25 and err(D, q, 3.5, -1.0) == 0.25


def heterogeneous_model(rng, m=60):
    losses = [L.QuadLoss(), L.L1Loss(), L.HuberLoss(), L.PeriodicLoss(1), L.OrdinalHingeLoss(1, 10), L.LogisticLoss(), L.WeightedHingeLoss(),
              L.MultinomialLoss(4), L.BvSLoss(5), L.MultinomialOrdinalLoss(4), L.PoissonLoss(30), L.OvALoss(3)]
    k = 4
    d = L.embedding_dim(losses)
    X, Y = rng.standard_normal((k, m)), rng.standard_normal((k, d))
    return losses, X, Y, k


def test_imputation_is_consistent():
    """test/err_test.jl:33-51: A = impute(doms, losses, X'Y) has zero error metric at (X, Y), standardized or not."""
    rng = np.random.default_rng(4)
    losses, X, Y, k = heterogeneous_model(rng)
    api = O.oracle_api()
    m = X.shape[1]
    g0 = L.GLRM(np.ones((m, len(losses))), losses, L.ZeroReg(), L.ZeroReg(), k, X=X, Y=Y, checknan=False)
    A = L.impute(g0, engine=api)
    doms = [L.default_domain(l) for l in losses]
    U = X.T @ Y
    for f, (lo, (y0, y1)) in enumerate(zip(losses, L.get_yidxs(losses))):      # the matrix equals the entry-wise mirror
        for i in range(0, m, 7):
            assert A[i, f] == pytest.approx(float(L.impute_entry(doms[f], lo, U[i, y0:y1] if y1 - y0 > 1 else U[i, y0])), rel=1e-12)
    g = L.GLRM(A, losses, L.ZeroReg(), L.ZeroReg(), k, X=X, Y=Y)
    assert L.error_metric(g, engine=api) == 0.0 and L.error_metric(g, standardize=True, engine=api) == 0.0
    Xp = X + 0.3 * rng.standard_normal(X.shape)
    e_raw, e_std = L.error_metric(g, Xp, Y, engine=api), L.error_metric(g, Xp, Y, standardize=True, engine=api)
    assert e_raw > 0 and e_std > 0 and e_raw != e_std
    # transcription of raw / std error metric with the Python mirrors
    tot_raw = tot_std = 0.0
    Up = Xp.T @ Y
    for f, (lo, (y0, y1)) in enumerate(zip(losses, L.get_yidxs(losses))):
        errs = [L.error_metric_entry(doms[f], lo, Up[i, y0:y1] if y1 - y0 > 1 else Up[i, y0], A[i, f]) for i in range(m)]
        cm = float(np.mean(A[:, f] ** 2))
        tot_raw += sum(errs)
        tot_std += sum(errs) / cm if cm != 0 else sum(errs)
    assert e_raw == pytest.approx(tot_raw, rel=1e-12) and e_std == pytest.approx(tot_std, rel=1e-12)


def test_error_metric_as_cross_validation_error_fn():
    """test/err_test.jl:26,57: error_fn = error_metric(glrm, X, Y, doms, standardize=true) inside cross_validate."""
    rng = np.random.default_rng(5)
    losses, X, Y, k = heterogeneous_model(rng, 50)
    api = O.oracle_api()
    g0 = L.GLRM(np.ones((50, len(losses))), losses, L.ZeroReg(), L.ZeroReg(), k, X=X, Y=Y)
    A = L.impute(g0, engine=api)
    g = L.GLRM(A, losses, L.QuadReg(0.05), L.QuadReg(0.05), k, rng=rng)
    doms = [L.default_domain(l) for l in losses]
    fn = lambda glrm, Xf, Yf, **kw: L.error_metric(glrm, Xf, Yf, doms, standardize=True, **kw)
    tr, te, _, _ = L.cross_validate(g, nfolds=3, params=L.ProxGradParams(max_iter=30), verbose=False, error_fn=fn, rng=rng, engine=api)
    assert np.all(np.isfinite(tr)) and np.all(te >= tr * 0.5)


def test_impute_missing_keeps_observed_entries_and_unsupported_pairs_fail():
    rng = np.random.default_rng(6)
    A = rng.standard_normal((20, 6))
    I, J = np.nonzero(rng.random((20, 6)) < 0.5)
    g = L.GLRM(A, L.QuadLoss(), L.QuadReg(), L.QuadReg(), 2, obs=(I, J), rng=rng)
    api = O.oracle_api()
    Ahat = L.impute_missing(g, engine=api)
    assert np.array_equal(Ahat[I, J], A[I, J]) and np.allclose(Ahat[0, :][~np.isin(np.arange(6), J[I == 0])], (g.X.T @ g.Y)[0, :][~np.isin(np.arange(6), J[I == 0])])
    gl = L.GLRM(A > 0, L.LogisticLoss(), L.QuadReg(), L.QuadReg(), 2, rng=rng)
    with pytest.raises(L.GLRMError):
        L.error_metric(gl, domains=[L.RealDomain()] * 6, engine=api)  # RealDomain + LogisticLoss: the reference errors out
