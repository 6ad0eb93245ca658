"""The definition of include/glrm_hip_sample.h without a GPU, on its numpy restatement (tests/sample_ref.py): the generator's known
answers, the uniforms, and -- over 20000 distinct counters at one fixed u, with fixed seeds, so deterministically -- that every rule
draws from the distribution the header states, within 5 standard errors."""
import math

import numpy as np

import lowrankmodels.jl_amd as L
import sample_ref as S

N = 20000
ROWS, COLS = np.arange(N) % 4000, np.arange(N) // 4000 + 3           # 20000 distinct (row, column) counters


def words(ctr, key):
    return [int(x[0]) for x in S.philox4x32_10(ctr, key)]


def test_philox_known_answers():
    assert words((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    assert words((f, f, f, f), (f, f)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert words((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_the_header_states_the_generator():
    import os
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glrm_hip_sample.h")).read()
    for c in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "6627e8d5 e169c58d bc57ac4c 9b00dbd8", "408f276d 41c83b0e a20bc7c6 6d5451fd",
              "d16cfe09 94fdcceb 5001e420 24126ea1", "6.283185307179586", "nothing is written"):
        assert c in txt, c


def test_uniforms_lie_in_the_half_open_unit_interval():
    z = [np.zeros(1, dtype=np.uint64)] * 4
    assert S.words_to_uniforms(z) == (0.0, 0.0)                       # all-zero words: exactly 0
    f = [np.full(1, 0xffffffff, dtype=np.uint64)] * 4
    top = S.words_to_uniforms(f)
    assert top[0] == top[1] == 1.0 - 2.0 ** -53                       # all-one words: the largest double below 1
    U0, U1 = S.uniforms(12345, ROWS, COLS)
    for U in (U0, U1):
        assert U.min() >= 0.0 and U.max() < 1.0
        assert abs(U.mean() - 0.5) < 5 * math.sqrt(1 / 12 / N)
    assert len(set(zip(U0.tolist(), U1.tolist()))) == N
    assert not np.array_equal(S.uniforms(12346, ROWS, COLS)[0], U0)   # another seed: other draws
    assert not np.array_equal(S.uniforms(12345 + 2 ** 32, ROWS, COLS)[0], U0)   # the high word of the seed is part of the key
    again = S.uniforms(12345, ROWS[::-1], COLS[::-1])                 # a function of (seed, row, column)
    assert np.array_equal(again[0][::-1], U0) and np.array_equal(again[1][::-1], U1)


def entry_draws(D, l, u, seed, sd=math.nan):
    U0, U1 = S.uniforms(seed, ROWS, COLS)
    return np.array([S.draw_entry(D, l, u, float(a), float(b), sd)[0] for a, b in zip(U0, U1)])


def test_s1_is_gaussian_around_u_and_the_two_rules_give_reciprocal_spreads():
    u, v = 0.75, 0.36
    sd0, sd1 = float(S.noise_sd(v, "residual")), float(S.noise_sd(v, "reference"))
    assert sd0 == math.sqrt(v) and sd1 == 1 / math.sqrt(v) and abs(sd0 * sd1 - 1) < 1e-15
    for sd in (sd0, sd1):
        x = entry_draws(L.RealDomain(), L.QuadLoss(), u, 7, sd)
        assert abs(x.mean() - u) < 5 * sd / math.sqrt(N)
        assert abs(x.var() - sd * sd) < 5 * sd * sd * math.sqrt(2 / N)
    a, b = entry_draws(L.RealDomain(), L.QuadLoss(), u, 7, sd0), entry_draws(L.RealDomain(), L.QuadLoss(), u, 7, sd1)
    z = S.gauss(*S.uniforms(7, ROWS, COLS))
    np.testing.assert_allclose((a - u) * (b - u), z * z, rtol=1e-12, atol=1e-15)    # the same z, spreads sd and 1 / sd
    assert abs(np.abs(z).max()) < 9 and abs((np.abs(z) < 1).mean() - 0.6826894921) < 5 * math.sqrt(0.68 * 0.32 / N)


def test_s2_is_bernoulli_with_the_logistic_probability():
    for u in (-1.5, 0.25, 2.0):
        x = entry_draws(L.BoolDomain(), L.LogisticLoss(), u, 11)
        p = 1 / (1 + math.exp(-u))
        assert set(np.unique(x)) <= {0.0, 1.0} and abs(x.mean() - p) < 5 * math.sqrt(p * (1 - p) / N)


def check_levels(D, l, u, seed):
    first, w = S.level_weights(D, l, u)
    p = np.array(w) / sum(w)
    x = entry_draws(D, l, np.array(u), seed)
    assert x.min() >= first and x.max() <= first + len(w) - 1
    for i, pi in enumerate(p):
        assert abs((x == first + i).mean() - pi) < 5 * math.sqrt(pi * (1 - pi) / N), (D, l, i)
    return p


def test_s3_and_s4_draw_levels_with_the_stated_weights():
    p = check_levels(L.CategoricalDomain(4), L.MultinomialLoss(4), [0.5, -1.0, 1.25, 0.0], 13)
    np.testing.assert_allclose(p, np.exp([0.5, -1.0, 1.25, 0.0]) / np.exp([0.5, -1.0, 1.25, 0.0]).sum())
    check_levels(L.CategoricalDomain(3), L.OvALoss(3), [0.5, -1.0, 1.25], 14)
    check_levels(L.OrdinalDomain(1, 5), L.BvSLoss(5), [1.0, 0.5, -0.25, -1.0], 15)
    check_levels(L.OrdinalDomain(1, 4), L.OrdisticLoss(4), [0.5, -1.0, 1.25, 0.1], 16)
    p = check_levels(L.OrdinalDomain(1, 5), L.MultinomialOrdinalLoss(5), [-0.5, -1.0, -1.25, -3.0], 17)
    assert abs(p.sum() - 1) < 1e-12
    check_levels(L.OrdinalDomain(2, 3), L.OvALoss(3), [0.5, -1.0, 1.25], 18)            # a sub-range of the levels: D.min + index
    check_levels(L.OrdinalDomain(1, 3), L.MultinomialLoss(3), [0.5, -1.0, 1.25], 19)    # Ordinal x Multinomial is S4, through evaluate


def test_wsample_edges_and_margins():
    assert S.wsample([1.0, 2.0, 1.0], 0.5) == (1, 0.25)
    assert S.wsample([0.0, 0.0], 0.7)[0] == 0 and S.wsample([math.nan, 1.0], 0.7)[0] == 0          # a zero or NaN sum: the first level
    assert S.wsample([1.0, 1.0], 0.999999)[0] == 1
    v, margin = S.draw_entry(L.BoolDomain(), L.LogisticLoss(), 0.0, 0.25, 0.0)
    assert v == 1.0 and margin == 0.25


def test_everything_else_is_the_imputation():
    assert S.rule(L.OrdinalDomain(1, 5), L.QuadLoss()) == "impute" and S.rule(L.PeriodicDomain(2.0), L.QuadLoss()) == "impute"
    assert S.rule(L.CountDomain(3), L.BvSLoss(4)) == "impute" and S.rule(L.BoolDomain(), L.OvALoss(3)) == "refused"
    for D, l, u in ((L.OrdinalDomain(1, 5), L.QuadLoss(), 2.6), (L.BoolDomain(), L.HingeLoss(), -0.3), (L.RealDomain(), L.L1Loss(), 0.4),
                    (L.CountDomain(9), L.PoissonLoss(9), 1.1), (L.PeriodicDomain(2.5), L.PeriodicLoss(2.5), 0.7)):
        v, margin = S.draw_entry(D, l, u, 0.3, 0.6)
        assert v == float(L.impute_entry(D, l, u)) and margin == math.inf
