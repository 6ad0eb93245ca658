"""-m gpu: glrm_hip_sample_at (include/glrm_hip_sample.h; csrc/glrm_sample.hip) and L.sample_at / sample_missing_at / sample /
sample_missing.

The reference is the numpy restatement of the header (tests/sample_ref.py).  Factors are multiples of 1/8 in [-1/2, 1/2], so every
product and every partial sum of the chain is exact: the restatement's u has the device's bits, and |u| stays below about 3.
  - deterministic entries ("everything else" of the rule table) have the bits of glrm_hip_impute_at;
  - discrete draws (S2, S3, S4) equal the restatement exactly wherever its margin exceeds MARGIN = 1e-9 (DESIGN.md section 4.12's
    figure for in-kernel exp / log against libm), and the test asserts on the CPU, before the engine is called, that at most 0.1 % of
    its entries lie below it (expected: T x levels x 2e-9, none at these sizes);
  - Gaussian draws (S1) under the "given" rule: |out - ref| <= S1_TOL * (|u| + 9 sd), 9 > sqrt(2 * 53 * ln 2) being the largest |z|.
    S1_TOL is 16 x the largest |out - ref| / (|u| + 9 sd) measured on the MI355X against the numpy restatement (5.1e-17, printed by
    test_rule_table), rounded up to a power of ten; 16 covers other libm versions; the project's ceiling is 1e-9.
Everything else is bit for bit."""
import math

import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import precision_ref as R
import sample_ref as S
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.domains import pack_domains
from lowrankmodels.jl_amd.losses import pack_losses
from lowrankmodels.jl_amd.regularizers import pack_regs
from test_gpu_leaks import free_bytes
from test_gpu_topk import Handle, hip

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
S1_TOL = 1e-15
BLOCKS = [0, 1, 64, 1000]
KS = [5, 20, 32, 64]
PS = [0, 1, 63, 64, 65, 257, 1000]
SEED = 0x9E3779B97F4A7C15

# one column per row of the rule table
TABLE = [(L.RealDomain(), L.QuadLoss()), (L.RealDomain(), L.QuadLoss(0.5)),                                    # S1, two spreads
         (L.BoolDomain(), L.LogisticLoss()),                                                                   # S2
         (L.CategoricalDomain(4), L.MultinomialLoss(4)),                                                       # S3
         (L.CategoricalDomain(3), L.OvALoss(3)), (L.OrdinalDomain(1, 5), L.BvSLoss(5)),                        # S4
         (L.OrdinalDomain(1, 4), L.OrdisticLoss(4)), (L.OrdinalDomain(1, 5), L.MultinomialOrdinalLoss(5)),
         (L.OrdinalDomain(1, 7), L.QuadLoss()), (L.BoolDomain(), L.HingeLoss()), (L.RealDomain(), L.L1Loss()),  # the imputation
         (L.CountDomain(9), L.PoissonLoss(9)), (L.PeriodicDomain(2.5), L.PeriodicLoss(2.5))]
TABLE_SD = [0.7, 1.9]


def eighths(rng, shape):
    return rng.integers(-4, 5, shape) / 8.0


def model(pairs, m, k, seed):
    """(problem arrays, X, Y, packed domains, losses, domains) of a fully observed model (A = 1) with one column per pair."""
    losses, doms = [l for _, l in pairs], [D for D, _ in pairs]
    rng = np.random.default_rng(seed)
    X, Y = np.asfortranarray(eighths(rng, (k, m))), np.asfortranarray(eighths(rng, (k, L.embedding_dim(losses))))
    g = L.GLRM(np.ones((m, len(pairs))), losses, L.ZeroReg(), L.ZeroReg(), k, X=X, Y=Y)
    pa = g.problem_arrays()
    g.close()
    return pa, X, Y, pack_domains(doms), losses, doms


def given_sd(pairs, rng=None):
    """n values: a spread at every S1 column, a poison elsewhere (never read)."""
    sd, it = np.full(len(pairs), -1e300), 0
    for j, (D, l) in enumerate(pairs):
        if S.rule(D, l) == "S1":
            sd[j] = TABLE_SD[it % 2] if rng is None else float(rng.uniform(0.25, 2.0))
            it += 1
    return sd


def shuffled_with_repeats(rng, m, n):
    t = np.concatenate([rng.permutation(m * n), rng.integers(0, m * n, 300)])
    return (t % m).astype(np.int64), (t // m).astype(np.int32)


def check_against_restatement(pairs, losses, doms, U, rows, cols, sd, got, imputed):
    kinds = np.array([S.rule(*pairs[j]) for j in cols])
    ref, margin = S.draws(doms, losses, U, rows, cols, SEED, sd)
    det = kinds == "impute"
    assert R.same_bits(got[det], imputed[det])                                                # the bits of impute_at
    disc = np.isin(kinds, ["S2", "S3", "S4"])
    sure = disc & (margin > MARGIN)
    bad = np.flatnonzero(sure & (got != ref))
    assert bad.size == 0, [(pairs[cols[t]], int(rows[t]), got[t], ref[t], margin[t]) for t in bad[:5]]
    s1 = kinds == "S1"
    spans = L.get_yidxs(losses)
    u = np.array([U[i, spans[j][0]] for i, j in zip(rows[s1], cols[s1])])
    ratio = np.abs(got[s1] - ref[s1]) / (np.abs(u) + 9 * sd[cols[s1]])
    print("S1 entries", int(s1.sum()), "max |out - ref| / (|u| + 9 sd) =", float(ratio.max()) if s1.any() else 0.0, "; discrete entries", int(disc.sum()),
          "smallest margin", float(margin[disc].min()) if disc.any() else math.inf)
    assert (ratio <= S1_TOL).all(), float(ratio.max())
    return ref, margin


# ================================================================== 1. the rule table

@pytest.mark.parametrize("m,k", [(129, 5), (130, 33)])
def test_rule_table(m, k):
    pa, X, Y, dd, losses, doms = model(TABLE, m, k, seed=700 + m)
    n = len(TABLE)
    rows, cols = shuffled_with_repeats(np.random.default_rng(m), m, n)
    U = R.xy_chain(X, Y)
    assert np.array_equal(U, X.T @ Y) and np.abs(U).max() <= 3.5                             # exact in any order; |u| <~ 3
    sd = given_sd(TABLE)
    # on the CPU, before the engine is called: (almost) every discrete draw is decided by more than the exponentials can move
    ref, margin = S.draws(doms, losses, U, rows, cols, SEED, sd)
    kinds = np.array([S.rule(*TABLE[j]) for j in cols])
    disc = np.isin(kinds, ["S2", "S3", "S4"])
    assert (margin[disc] <= MARGIN).sum() <= 0.001 * len(rows)
    assert {"S1", "S2", "S3", "S4", "impute"} == set(kinds)
    for j in range(2, 8):                                                                     # every level of every discrete column is drawn
        D = doms[j]
        want = {0.0, 1.0} if isinstance(D, L.BoolDomain) else set(map(float, range(D.min, D.max + 1)))
        assert set(ref[cols == j]) == want, (TABLE[j], sorted(set(ref[cols == j])))
    with Handle(pa) as (api, h):
        imputed = api.impute_at(h, X, Y, dd, m, n, rows, cols)
        for b in [0, 1000]:
            got, kept, sd_out = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED, noise="given", noise_sd=sd, block_entries=b)
            info = api.sample_at_info()
            print("m", m, "k", k, "block_entries", b, info)
            check_against_restatement(TABLE, losses, doms, U, rows, cols, sd, got, imputed)
            n_general = int(sum(losses[j].embedding_dim > 1 for j in cols))
            assert info["entries_general"] == n_general and info["entries_fast"] == len(rows) - n_general and info["entries_kept"] == 0
            assert info["variance_columns"] == 0 and kept is None
            assert R.same_bits(sd_out, np.where(np.arange(n) < 2, sd, np.nan))                # noise_sd_in echoed, NaN elsewhere
        # a wrong word order, the wrong column's sd or a wrong counter would miss by order sd: the two S1 columns have the spreads given
        s1 = np.isin(cols, [0, 1])
        z = (got[s1] - np.array([U[i, j] for i, j in zip(rows[s1], cols[s1])])) / sd[cols[s1]]
        assert abs(z.mean()) < 5 / math.sqrt(s1.sum()) and abs(z.var() - 1) < 5 * math.sqrt(2 / s1.sum())


# ================================================================== 2. the variance pass

VAR_LENS = [0, 1, 63, 64, 65, 1100]


def variance_model():
    """Six Real x QuadLoss columns of 0 .. 1100 observations, a Bool x LogisticLoss and an Ordinal x QuadLoss column (not S1)."""
    m, k = 1200, 5
    pairs = [(L.RealDomain(), L.QuadLoss())] * len(VAR_LENS) + [(L.BoolDomain(), L.LogisticLoss()), (L.OrdinalDomain(1, 5), L.QuadLoss())]
    lens = VAR_LENS + [40, 40]
    rng = np.random.default_rng(52)
    A = rng.standard_normal((m, len(pairs)))
    A[:, 6], A[:, 7] = rng.integers(0, 2, m), rng.integers(1, 6, m)
    I = np.concatenate([np.sort(rng.choice(m, c, replace=False)) for c in lens])
    J = np.repeat(np.arange(len(lens)), lens)
    losses, doms = [l for _, l in pairs], [D for D, _ in pairs]
    X, Y = np.asfortranarray(eighths(rng, (k, m))), np.asfortranarray(eighths(rng, (k, len(pairs))))
    g = L.GLRM(A, losses, L.ZeroReg(), L.ZeroReg(), k, obs=(I, J), X=X, Y=Y)
    pa = g.problem_arrays()
    g.close()
    return pa, X, Y, pack_domains(doms), pairs, m


def test_variance_pass():
    pa, X, Y, dd, pairs, m = variance_model()
    n = len(pairs)
    U = R.xy_chain(X, Y)
    v = np.array([S.column_variance(U, pa.colptr, pa.rowidx, pa.colvals, j, j) if j < len(VAR_LENS) else np.nan for j in range(n)])
    assert np.isnan(v[0]) and (v[1:6] > 0).all()
    rng = np.random.default_rng(53)
    rows, cols = rng.integers(0, m, 500).astype(np.int64), rng.integers(0, n, 500).astype(np.int32)
    with Handle(pa) as (api, h):
        for noise in ("residual", "reference"):
            got, _, sd = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED, noise=noise)
            info = api.sample_at_info()
            want = S.noise_sd(v, noise)
            print(noise, "sd", sd.tolist(), "restatement", want.tolist(), info)
            assert info["variance_columns"] == len(VAR_LENS)
            assert np.isnan(sd[0]) and np.isnan(sd[6:]).all()                                  # the empty column, the columns that are not S1
            for j in range(1, 6):
                assert abs(sd[j] - want[j]) <= (VAR_LENS[j] + 4) * 2.0 ** -52 * want[j], (noise, j, sd[j], want[j])
            again, _, echoed = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED, noise="given", noise_sd=sd)
            assert R.same_bits(again, got) and R.same_bits(echoed, sd)                          # rule 0 / 1 = rule 2 fed with the returned sd
            assert api.sample_at_info()["variance_columns"] == 0
            assert np.isnan(got[cols == 0]).all() and np.isfinite(got[cols != 0]).all()         # an empty column: NaN draws
        sd_res = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED, noise="residual")[2]
        sd_ref = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED, noise="reference")[2]
        np.testing.assert_allclose(sd_res[1:6] * sd_ref[1:6], 1.0, rtol=1e-15)                 # reciprocal spreads
        # the pass runs only when its result is used
        only = np.flatnonzero(cols >= 6)
        api.sample_at(h, X, Y, dd, m, n, rows[only], cols[only], seed=SEED, want_noise_sd=False)
        assert api.sample_at_info()["variance_columns"] == 0
        none, _, sd0 = api.sample_at(h, X, Y, dd, m, n, rows[:0], cols[:0], seed=SEED)          # T == 0 writes only noise_sd_out
        assert none.shape == (0,) and R.same_bits(sd0, sd_res) and api.sample_at_info()["blocks"] == 0


# ================================================================== 3. a function of (seed, row, column) only

MIX = [TABLE[j % len(TABLE)] for j in range(40)]


@pytest.mark.parametrize("k", KS)
def test_a_draw_is_a_function_of_seed_row_and_column(k):
    m = 129 + (k == 64)
    pa, X, Y, dd, losses, doms = model(MIX, m, k, seed=800 + k)
    n = len(MIX)
    rng = np.random.default_rng(k)
    sd = given_sd(MIX, rng)
    with Handle(pa) as (api, h):
        assert api.factor_ld(h) == {5: 8, 20: 32, 32: 32, 64: 64}[k]
        grid = api.sample_at(h, X, Y, dd, m, n, rows=np.arange(m), seed=SEED, noise="given", noise_sd=sd)[0]
        assert grid.shape == (m, n) and np.isfinite(grid).all()
        for P in PS:
            rows, cols = rng.integers(0, m, P).astype(np.int64), rng.integers(0, n, P).astype(np.int32)
            for b in BLOCKS:
                got = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED, noise="given", noise_sd=sd, block_entries=b)[0]
                info = api.sample_at_info()
                assert R.same_bits(got, grid[rows, cols]), (P, b)
                assert info["blocks"] == (0 if P == 0 else -(-P // b) if b else 1) and info["entries_fast"] + info["entries_general"] == P
        for b in BLOCKS + [37]:
            rs = [m - 1, 0, 64, 64]
            assert R.same_bits(api.sample_at(h, X, Y, dd, m, n, rows=rs, seed=SEED, noise="given", noise_sd=sd, block_entries=b)[0], grid[rs, :]), b
            cs = [n - 1, 0, 5, 3]
            slab = api.sample_at(h, X, Y, dd, m, n, cols=cs, seed=SEED, noise="given", noise_sd=sd, block_entries=b)[0]
            assert slab.shape == (m, 4) and slab.flags.f_contiguous and R.same_bits(slab, grid[:, cs]), b
        rows, cols = rng.integers(0, m, 1000).astype(np.int64), rng.integers(0, n, 1000).astype(np.int32)
        base = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED, noise="given", noise_sd=sd)[0]
        perm = rng.permutation(1000)
        assert R.same_bits(api.sample_at(h, X, Y, dd, m, n, rows[perm], cols[perm], seed=SEED, noise="given", noise_sd=sd)[0], base[perm])
        api.set_factors(h, X, Y)                                                               # resident against uploaded factors
        assert R.same_bits(api.sample_at(h, None, None, dd, m, n, rows, cols, seed=SEED, noise="given", noise_sd=sd)[0], base)
        other = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED + 1, noise="given", noise_sd=sd)[0]
        high = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED ^ (1 << 40), noise="given", noise_sd=sd)[0]
        rnd = np.array([S.rule(*MIX[j]) != "impute" for j in cols])
        assert (other[rnd] != base[rnd]).mean() > 0.3 and (high[rnd] != base[rnd]).mean() > 0.3  # two seeds differ (both key words count)
        assert R.same_bits(other[~rnd], base[~rnd])
        if k == 20:                                                                            # against the restatement at this size too
            U = R.xy_chain(X, Y)
            imputed = api.impute_at(h, X, Y, dd, m, n, rows, cols)
            check_against_restatement(MIX, losses, doms, U, rows, cols, sd, base, imputed)


# ================================================================== 4. keep_observed

def raw_lists_model(m, n, k, rng):
    """Raw row lists in arbitrary order, 0 .. 40 entries a row (lengths around the 16-lane walk among them), columns listed twice with
    different values; the COLUMN view lists other entries (the rows shifted by one) with other values: the row view decides."""
    lens = [0, 1, 15, 16, 17, 31, 32, 33, 40] + rng.integers(0, 41, m - 9).tolist()
    lists = [rng.integers(0, n, c) for c in lens]
    lists[5][[0, 30]] = 7                                                                     # twice in one row, 30 places apart
    lists[7][[16, 17]] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    colidx = np.concatenate(lists).astype(np.int32)
    rowvals = 100.0 + np.arange(len(colidx), dtype=np.float64)                                # every stored value is different
    I = (np.repeat(np.arange(m, dtype=np.int64), lens) + 1) % m
    pc = np.argsort(colidx, kind="stable")
    colptr = np.concatenate([[0], np.cumsum(np.bincount(colidx, minlength=n))]).astype(np.int64)
    pa = _capi.ProblemArrays(m, n, k, rowptr, colidx, rowvals, colptr, np.ascontiguousarray(I[pc].astype(np.int32)), -rowvals[pc],
                             pack_losses([L.QuadLoss()] * n), pack_regs([L.ZeroReg()]), pack_regs([L.ZeroReg()]))
    return pa, lists, rowptr, rowvals


def test_keep_observed():
    m, n, k = 130, 40, 20
    rng = np.random.default_rng(41)
    pa, lists, rowptr, rowvals = raw_lists_model(m, n, k, rng)
    X, Y = np.asfortranarray(eighths(rng, (k, m))), np.asfortranarray(eighths(rng, (k, n)))
    dd = pack_domains([L.RealDomain()] * n)
    sd = np.full(n, 0.5)
    rows, cols = shuffled_with_repeats(rng, m, n)

    def host(rows, cols, plain):
        want, kept = plain.copy(), np.zeros(len(rows), dtype=bool)
        for t, (i, j) in enumerate(zip(rows, cols)):
            at = np.flatnonzero(lists[i] == j)
            if at.size:
                want[t], kept[t] = rowvals[rowptr[i] + at[0]], True                            # the first occurrence in list order
        return want, kept

    with Handle(pa) as (api, h):
        plain = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED, noise="given", noise_sd=sd)[0]
        want, wkept = host(rows, cols, plain)
        assert 0 < wkept.sum() < len(rows) and want[(rows == 5) & (cols == 7)][0] == rowvals[rowptr[5]]
        for b in BLOCKS:
            got, kept, _ = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED, noise="given", noise_sd=sd, keep_observed=True, block_entries=b)
            info = api.sample_at_info()
            assert np.array_equal(kept, wkept) and info["entries_kept"] == int(wkept.sum()), b
            assert R.same_bits(got, want), b                                                  # unobserved entries: the draws of keep_observed = 0
        got, kept, _ = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED, noise="given", noise_sd=sd, keep_observed=True, want_kept=False)
        assert kept is None and R.same_bits(got, want) and api.sample_at_info()["entries_kept"] == int(wkept.sum())   # kept may be NULL
        ii, jj = np.tile(np.arange(m), n), np.repeat(np.arange(n), m)
        full = api.sample_at(h, X, Y, dd, m, n, rows=np.arange(m), seed=SEED, noise="given", noise_sd=sd)[0]
        w2, k2 = host(ii, jj, full.reshape(-1, order="F"))
        for b in [0, 37]:
            got, kept, _ = api.sample_at(h, X, Y, dd, m, n, rows=np.arange(m), seed=SEED, noise="given", noise_sd=sd, keep_observed=True, block_entries=b)
            assert got.shape == kept.shape == (m, n) and R.same_bits(got.reshape(-1, order="F"), w2) and np.array_equal(kept.reshape(-1, order="F"), k2)
        got, kept, _ = api.sample_at(h, X, Y, dd, m, n, cols=[7, 0], seed=SEED, noise="given", noise_sd=sd, keep_observed=True)
        assert R.same_bits(got, np.stack([w2[jj == 7], w2[jj == 0]], axis=1)) and np.array_equal(kept[:, 0], k2[jj == 7])
        # residual noise reads the COLUMN view (values -rowvals), keeping reads the ROW view
        res, kept, sdr = api.sample_at(h, X, Y, dd, m, n, rows, cols, seed=SEED, keep_observed=True)
        assert np.array_equal(kept, wkept) and R.same_bits(res[wkept], want[wkept]) and (sdr > 50).all()


# ================================================================== 5. refusals

def test_refusals_touch_nothing():
    """Every refusal of the header with out, kept and noise_sd_out pre-filled.  (keep_observed on a handle without a row view cannot
    be produced: every list handle the engine finalizes has one.)"""
    pa, X, Y, dd, losses, doms = model([(L.RealDomain(), L.QuadLoss())] * 40, 130, 5, seed=9)
    api = hip()
    N = 40
    rows, cols = np.array([3, 5, 129], dtype=np.int64), np.array([0, 39, 7], dtype=np.int32)
    out, kept, sdo, sdi = np.full(3 * N, -7.0), np.full(3 * N, 7, dtype=np.uint8), np.full(N, -7.0), np.full(N, 0.5)
    p = lambda a: None if a is None else a.ctypes.data                                       # noqa: E731

    def refused(h, code, word, *, X=X, Y=Y, d=dd, r=rows, nr=3, c=cols, nc=3, mode=0, rule=0, si=None, keep=1, b=0, o=out, kp=kept, so=sdo):
        rc = api._f["sample_at"](h, p(X), p(Y), p(d), p(r), nr, p(c), nc, mode, SEED, rule, p(si), keep, b, p(o), p(kp), p(so))
        assert rc == code and word in api.last_error(), (rc, api.last_error())
        assert (out == -7.0).all() and (kept == 7).all() and (sdo == -7.0).all()              # a refusal touches nothing

    with Handle(pa) as (_, h):
        I = _capi.ERR_INVALID
        refused(h, I, "noise_rule 3", rule=3)
        refused(h, I, "noise_rule -1", rule=-1)
        refused(h, I, "needs noise_sd_in", rule=2)
        refused(h, I, "noise_rule 2 (given) only", rule=0, si=sdi)
        refused(h, I, "noise_rule 2 (given) only", rule=1, si=sdi)
        refused(h, I, "keep_observed 2", keep=2)
        refused(h, I, "keep_observed -1", keep=-1)
        refused(h, I, "kept needs keep_observed", keep=0)
        # inherited from impute_at
        refused(h, I, "rows[1] = 130", r=np.array([3, 130, 0], dtype=np.int64))
        refused(h, I, "cols[0] = -1", c=np.array([-1, 0, 0], dtype=np.int32))
        refused(h, I, "rows[0] = 130", r=np.array([130, 0, 0], dtype=np.int64), c=None, nc=0, mode=1)
        refused(h, I, "cols[1] = 40", c=np.array([0, 40, 0], dtype=np.int32), r=None, nr=0, mode=2)
        refused(h, I, "negative", nr=-1, nc=-1)
        refused(h, I, "n_rows 3 == n_cols 2", nc=2)
        refused(h, I, "row slab", mode=1)
        refused(h, I, "column slab", mode=2)
        refused(h, I, "NULL", r=None)
        refused(h, I, "mode 3", mode=3)
        refused(h, I, "out is NULL", o=None)
        refused(h, I, "domains is NULL", d=None)
        refused(h, I, "block_entries -1", b=-1)
        bad = dd.copy()
        bad[20]["kind"] = 6
        refused(h, I, "domain descriptor 20 is invalid", d=bad)
        refused(h, I, "both", Y=None)
        refused(None, I, "NULL handle")
        rc = api._f["sample_at"](h, p(X), p(Y), p(dd), p(rows), 3, p(cols), 3, 0, SEED, 2, p(sdi), 0, 0, p(out), None, None)   # kept and noise_sd_out may be NULL
        assert rc == 0 and np.isfinite(out[:3]).all() and (out[:3] != -7.0).all() and (out[3:] == -7.0).all()
        out[:] = -7.0

    g = L.GLRM(np.ones((64, 40)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 16)                 # (k = 16: eligible for the dense hand-over)
    Xg, Yg = np.zeros((16, 64), order="F"), np.zeros((16, 40), order="F")
    r2 = np.array([3, 5, 63], dtype=np.int64)
    for make, code, word in ((lambda: api.create(g.problem_arrays(dense=True)), _capi.ERR_UNSUPPORTED, "dense_A"),
                             (lambda: api.create(g.problem_arrays(), storage=_capi.STORAGE_F32), _capi.ERR_UNSUPPORTED, "storage = f32"),
                             (lambda: api.create(g.problem_arrays(rows=(0, 32))), _capi.ERR_INVALID, "single-shard"),
                             (lambda: api.create(g.problem_arrays(), defer=True), _capi.ERR_INVALID, "glrm_hip_finalize")):
        hh = make()
        try:
            refused(hh, code, word, X=Xg, Y=Yg, r=r2)
        finally:
            api.destroy(hh)
    g.close()


CANNOT = [("real-logistic", L.RealDomain(), L.LogisticLoss()), ("bool-ova", L.BoolDomain(), L.OvALoss(3)),
          ("levels-above", L.OrdinalDomain(1, 4), L.OvALoss(3)), ("levels-below", L.OrdinalDomain(0, 3), L.BvSLoss(4)),
          ("levels-above-mnlord", L.OrdinalDomain(1, 6), L.MultinomialOrdinalLoss(5)), ("real-ordistic", L.RealDomain(), L.OrdisticLoss(3))]


@pytest.mark.parametrize("name,D,loss", CANNOT, ids=[c[0] for c in CANNOT])
def test_a_column_that_cannot_be_sampled_is_refused_only_where_it_is_queried(name, D, loss):
    pairs = [(L.RealDomain(), L.QuadLoss()), (L.CategoricalDomain(3), L.OvALoss(3)), (D, loss), (L.OrdinalDomain(1, 4), L.BvSLoss(4))]
    pa, X, Y, dd, losses, doms = model(pairs, 130, 3, seed=5)
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 130, 400).astype(np.int64)
    cols = rng.choice([0, 1, 3], 400).astype(np.int32)
    sd = np.full(4, 0.5)
    with Handle(pa) as (api, h):
        got = api.sample_at(h, X, Y, dd, 130, 4, rows, cols, seed=SEED, noise="given", noise_sd=sd)[0]   # nobody asks for column 2
        ref, margin = S.draws(doms, losses, R.xy_chain(X, Y), rows, cols, SEED, sd)
        disc = (cols != 0) & (margin > MARGIN)
        assert np.array_equal(got[disc], ref[disc]) and np.allclose(got[cols == 0], ref[cols == 0], rtol=0, atol=1e-12)
        out = np.full(400 * 4, -7.0)
        fn = api._f["sample_at"]
        touching = cols.copy()
        touching[399] = 2
        only = np.array([1, 2], dtype=np.int32)
        for args in ((rows.ctypes.data, 400, touching.ctypes.data, 400, 0),                  # one pair in the column
                     (rows.ctypes.data, 400, None, 0, 1),                                    # whole rows cross it
                     (None, 0, only.ctypes.data, 2, 2)):                                     # the column itself
            assert fn(h, X.ctypes.data, Y.ctypes.data, dd.ctypes.data, *args, SEED, 2, sd.ctypes.data, 0, 0, out.ctypes.data, None, None) == _capi.ERR_UNSUPPORTED
            assert "column 2 is queried" in api.last_error() and (out == -7.0).all()
        assert R.same_bits(api.sample_at(h, X, Y, dd, 130, 4, rows, cols, seed=SEED, noise="given", noise_sd=sd)[0], got)   # the handle serves the next call


# ================================================================== 6. the driver

def test_the_driver():
    rng = np.random.default_rng(28)
    m, n, k = 60, 40, 3
    A = rng.standard_normal((m, k)) @ rng.standard_normal((k, n)) + 0.1 * rng.standard_normal((m, n))
    I, J = np.nonzero(rng.random((m, n)) < 0.4)
    g = L.GLRM(A, L.QuadLoss(), L.QuadReg(.1), L.QuadReg(.1), k, obs=(I, J), rng=np.random.default_rng(29))
    L.fit_b(g, L.Params(1, max_iter=10, abs_tol=1e-5, min_stepsize=0.01), verbose=False, engine=hip())
    full = L.sample(g, seed=5)
    info = g._sample_info
    assert full.shape == (m, n) and np.isfinite(full).all() and info["seed"] == 5 and info["variance_columns"] == n and info["entries_kept"] == 0
    assert info["noise_sd"].shape == (n,) and (info["noise_sd"] > 0).all() and info["entries_fast"] == m * n
    U = L.impute(g, engine=hip())
    z = (full - U) / info["noise_sd"][None, :]
    assert abs(z.mean()) < 5 / math.sqrt(m * n) and abs(z.var() - 1) < 5 * math.sqrt(2 / (m * n))
    hi, hj = np.nonzero(~np.isin(np.arange(m * n), I * n + J).reshape(m, n))
    assert R.same_bits(L.sample_at(g, hi, hj, seed=5), full[hi, hj])
    assert R.same_bits(L.sample_at(g, rows=[59, 0, 0], seed=5), full[[59, 0, 0], :]) and R.same_bits(L.sample_at(g, cols=[39, 1], seed=5), full[:, [39, 1]])
    assert R.same_bits(L.sample_at(g, hi, hj, seed=5, noise_sd=info["noise_sd"]), full[hi, hj])           # pay for the pass once
    assert not R.same_bits(L.sample_at(g, hi, hj, seed=6), full[hi, hj])
    a, b = np.random.default_rng(77), np.random.default_rng(77)
    assert R.same_bits(L.sample_at(g, hi, hj, rng=a), L.sample_at(g, hi, hj, seed=int(b.integers(0, 2 ** 64, dtype=np.uint64))))   # rng= against seed=
    ref = L.sample_at(g, hi, hj, seed=5, noise="reference")
    np.testing.assert_allclose((ref - U[hi, hj]) * (full[hi, hj] - U[hi, hj]), ((full[hi, hj] - U[hi, hj]) / info["noise_sd"][hj]) ** 2, rtol=1e-9)
    miss = L.sample_missing(g, seed=5)
    obs = np.zeros((m, n), dtype=bool)
    obs[I, J] = True
    assert np.array_equal(miss[obs], A[obs]) and R.same_bits(miss[~obs], full[~obs]) and g._sample_info["entries_kept"] == len(I)
    assert R.same_bits(L.sample_missing_at(g, [0, 1, 2], [0, 1, 2], seed=5), miss[[0, 1, 2], [0, 1, 2]])
    gb = L.GLRM(A > 0, L.LogisticLoss(), L.ZeroReg(), L.ZeroReg(), k, X=g.X.copy(), Y=g.Y.copy())
    got = L.sample_at(gb, hi, hj, seed=5)                                                    # Bool columns come back as 1.0 / 0.0
    assert got.dtype == np.float64 and set(np.unique(got)) == {0.0, 1.0}
    gb.close()
    with pytest.raises(ValueError, match="sample"):
        L.sample_at(g, seed=5)
    with pytest.raises(_capi.GLRMError) as ei:
        L.sample_at(g, [m], [0], seed=5)
    assert ei.value.code == _capi.ERR_INVALID
    g.close()


# ================================================================== 7. leaks

def test_no_device_memory_leak():
    """20 calls leave device memory where it was, as tests/test_gpu_impute_at.py checks it: a call's scratch is tens of MiB here
    (10^6 pairs), the better of two windows of 10 calls is held to 4 MiB."""
    pa, X, Y, dd, losses, doms = model([(L.RealDomain(), L.QuadLoss())] * 40, 130, 20, seed=30)
    rng = np.random.default_rng(30)
    P = 1000000
    rows, cols = rng.integers(0, 130, P), rng.integers(0, 40, P)
    with Handle(pa) as (api, h):
        first = api.sample_at(h, X, Y, dd, 130, 40, rows, cols, seed=SEED, keep_observed=True)
        api.sample_at(h, X, Y, dd, 130, 40, rows, cols, seed=SEED, keep_observed=True)
        levels = [free_bytes()]
        for _ in range(2):
            for _ in range(10):
                last = api.sample_at(h, X, Y, dd, 130, 40, rows, cols, seed=SEED, keep_observed=True)
            levels.append(free_bytes())
        assert R.same_bits(last[0], first[0]) and np.array_equal(last[1], first[1]) and last[1].all()
        lost = [levels[i] - levels[i + 1] for i in range(2)]
        assert min(lost) < 4 << 20, f"device memory lost per window of 10 calls (MiB): {[round(x / 2**20, 1) for x in lost]}"
