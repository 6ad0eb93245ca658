"""-m gpu: glrm_hip_init_kmeanspp (include/glrm_hip_init.h) against the numpy transcription of init_kmeanspp! (tests/kmeanspp_ref.py).

Compared: `centers` (equal), `Y` (bit-equal) and `weights` (relative 1e-12, NaN positions equal).  The 1e-12 is derived, not measured:
a weight is a sum of at most 1100 non-negative terms here (the longest row of SPECIAL), so re-association moves it by at most about
1100 * 2^-53 = 1.2e-13 relatively, and the minimum and the quotient keep that bound.

Precondition, asserted on the CPU BEFORE the engine is called (it fails the test, it does not skip it): every draw's margin -- its
distance from the nearest boundary of the cumulative weights, relative to their total -- is at least 1e-9.  The engine's tree-shaped
sums of m <= 4096 weights move a boundary by at most about 4096 * 2^-53 S < 1e-12 S, so 1e-9 leaves three orders of magnitude.  A draw
that no rounding can move (t == 0 from u == 0 or a zero total, a NaN total: the walk's first comparison `cw < t` fails and row 0 is
returned) has margin +Inf in the transcription.

The problems are handed over as raw lists (_capi.ProblemArrays): unsorted rows, and columns listed twice in a row WITH DIFFERENT values,
which a model built from a matrix cannot express."""
import functools

import numpy as np
import pytest

import kmeanspp_ref as R
import lowrankmodels.jl_amd as L
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.losses import pack_losses
from lowrankmodels.jl_amd.regularizers import pack_regs

pytestmark = pytest.mark.gpu

# Row lengths of the distance pass (and 0, in the case that wants it): 63 / 64 / 65 around a wave, 257 = the first length on the whole-wave
# path (row 4, which the duplicate tests use), and lengths that need a SECOND and a THIRD trip of the batched load loop with a masked
# tail -- a 16-lane group covers 8 x 16 = 128 entries per trip (129, 200, 256), a whole wave 8 x 64 = 512 (513, 600, 1100)
SPECIAL = (1, 63, 64, 65, 257, 129, 200, 256, 513, 600, 1100)
MIX = ("quad", "huber", "logistic", "ordinal", "poisson")


def hip():
    return _capi.hip_api()


def loss_of(name):
    return {"quad": L.QuadLoss, "huber": lambda: L.HuberLoss(1.0, 0.7), "logistic": L.LogisticLoss, "ordinal": lambda: L.OrdinalHingeLoss(1, 5),
            "poisson": L.PoissonLoss, "periodic": lambda: L.PeriodicLoss(3.0)}[name]()


def values_of(name, rng, cnt):
    if name == "logistic":
        return (rng.random(cnt) < 0.5).astype(np.float64)
    if name == "ordinal":
        return rng.integers(1, 6, cnt).astype(np.float64)
    if name == "poisson":
        return rng.integers(0, 7, cnt).astype(np.float64)
    if name == "periodic":
        return 3.0 * rng.random(cnt)
    return 2.0 * rng.standard_normal(cnt)


class Problem:
    """m rows with the given lengths over n columns, lists in random order; a row longer than n repeats columns."""

    def __init__(self, lens, n, k, kinds=("quad",), seed=0, dup_rows=()):
        """dup_rows: rows whose second half lists the columns of the first half again (in another order, with other values)."""
        rng = np.random.default_rng(seed)
        self.m, self.n, self.k = len(lens), n, k
        self.kinds = [kinds[j % len(kinds)] for j in range(n)]
        self.losses = [loss_of(kd) for kd in self.kinds]
        self.rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        cols = [rng.permutation(n)[:ln] if ln <= n else rng.integers(0, n, ln) for ln in lens]
        for r in dup_rows:
            half = len(cols[r]) // 2
            cols[r][half:2 * half] = rng.permutation(cols[r][:half])
        self.colidx = (np.concatenate(cols) if self.rowptr[-1] else np.zeros(0)).astype(np.int32)
        self.rowvals = np.zeros(len(self.colidx))
        for kd in set(self.kinds):
            sel = np.flatnonzero(np.array(self.kinds)[self.colidx] == kd) if len(self.colidx) else np.zeros(0, np.int64)
            self.rowvals[sel] = values_of(kd, rng, len(sel))
        self.Y0 = np.asfortranarray(rng.standard_normal((k, n)))
        self.rng = rng

    def arrays(self):
        I = np.repeat(np.arange(self.m, dtype=np.int64), np.diff(self.rowptr))
        pc = np.argsort(self.colidx, kind="stable")
        colptr = np.concatenate([[0], np.cumsum(np.bincount(self.colidx, minlength=self.n))]).astype(np.int64)
        return _capi.ProblemArrays(self.m, self.n, self.k, self.rowptr, np.ascontiguousarray(self.colidx), np.ascontiguousarray(self.rowvals),
                                   colptr, np.ascontiguousarray(I[pc].astype(np.int32)), np.ascontiguousarray(self.rowvals[pc]),
                                   pack_losses(self.losses), pack_regs([L.ZeroReg()]), pack_regs([L.ZeroReg()]))

    def reference(self, first, u):
        return R.init_kmeanspp(self.m, self.n, self.k, self.rowptr, self.colidx, self.rowvals, self.losses, self.Y0, first, u)

    def engine(self, first, u, **opts):
        api = hip()
        h = api.create(self.arrays(), **opts)
        try:
            Y = self.Y0.copy(order="F")
            centers, weights = api.init_kmeanspp(h, Y, first, u, want_weights=True, m=self.m)
        finally:
            api.destroy(h)
        return dict(Y=Y, centers=centers, weights=weights)


def ragged(m, seed, special=SPECIAL):
    """Row lengths 1..12 with the special lengths planted at the front (as many as fit)."""
    lens = np.random.default_rng(seed).integers(1, 13, m)
    lens[: min(m, len(special))] = special[: min(m, len(special))]
    return lens.tolist()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def compare(ref, got):
    print("margins", ref["margins"].tolist(), "centers", ref["centers"].tolist(), got["centers"].tolist())
    assert got["centers"].tolist() == ref["centers"].tolist()
    assert same_bits(got["Y"], ref["Y"])
    rw, gw = ref["weights"], got["weights"]
    assert rw.shape == gw.shape and np.array_equal(np.isnan(rw), np.isnan(gw))
    ok = ~np.isnan(rw)
    err = np.abs(gw[ok] - rw[ok])
    print("worst relative weight difference", float(np.max(err / np.maximum(np.abs(rw[ok]), 1e-300), initial=0.0)))
    assert np.all(err <= 1e-12 * np.abs(rw[ok]))


def check(p, first, u, **opts):
    ref = p.reference(first, u)
    assert np.all(ref["margins"] >= 1e-9), ref["margins"]   # the precondition: fails, never skips
    got = p.engine(first, u, **opts)
    compare(ref, got)
    return ref, got


@functools.lru_cache(maxsize=None)
def quad_problem(m):
    return Problem(ragged(m, seed=m), 70, 5, seed=m)


@pytest.mark.parametrize("m", [1, 2, 1023, 1024, 1025, 2049])
def test_sampler_chunk_edges(m):
    """m around the 1024-row chunk of the sampler; one QuadLoss descriptor; ragged, unsorted rows with the special lengths."""
    p = quad_problem(m)
    u = np.random.default_rng(100 + m).random(4)
    ref, _ = check(p, m // 2, u)
    if m > 2:
        assert len(set(ref["centers"].tolist())) > 2         # the draws did spread over the rows


def test_a_draw_in_the_last_chunk_and_the_last_row():
    """u just below 1: the walk runs to the end of the last, partly filled chunk."""
    p = quad_problem(1025)
    ref, _ = check(p, 3, [1.0 - 2.0 ** -20, 0.5, 1.0 - 2.0 ** -20, 0.25])
    assert ref["centers"][1] >= 1000


def test_empty_row_makes_every_weight_sum_nan_and_every_later_centre_row_zero():
    p = Problem([5, 0] + ragged(40, seed=3), 70, 5, seed=3)
    ref, got = check(p, 7, [0.3, 0.6, 0.9, 0.1])
    assert np.all(np.isnan(got["weights"][:, 1])) and got["centers"].tolist() == [7, 0, 0, 0, 0]


@pytest.mark.parametrize("k", [1, 2, 5])
def test_one_column_and_small_ranks(k):
    """n = 1: every row lists column 0 (rows longer than 1 list it repeatedly, the last value is the centre's); k = 1: no round at all."""
    p = Problem(ragged(40, seed=5), 1, k, seed=5)
    u = np.random.default_rng(6).random(k - 1)
    ref, got = check(p, 4, u)                                  # row 4 has 257 entries of column 0
    assert got["Y"][0, 0] == p.rowvals[p.rowptr[5] - 1]
    if k == 1:
        assert got["weights"].shape == (0, 40) and got["centers"].tolist() == [4]
    p70 = Problem(ragged(40, seed=8), 70, k, seed=8)
    check(p70, 0, u)


def test_duplicated_column_in_a_centre_forced_by_first_center_and_by_u():
    p = Problem(ragged(300, seed=9), 70, 3, seed=9)
    dup = 4                                                    # 257 entries over 70 columns: every column several times, different values
    b, e = p.rowptr[dup], p.rowptr[dup + 1]
    assert len(set(p.colidx[b:e].tolist())) < e - b
    last = {int(j): v for j, v in zip(p.colidx[b:e], p.rowvals[b:e])}
    ref, got = check(p, dup, [0.4, 0.8])
    assert all(got["Y"][0, j] == v for j, v in last.items())
    # by u: the weights of round 1 do not depend on u, so aim the first draw at the middle of the duplicated row's interval
    w = p.reference(0, [0.5, 0.5])["weights"][0]
    cum = np.cumsum(w)
    u0 = (cum[dup - 1] + 0.5 * w[dup]) / cum[-1]
    ref, got = check(p, 0, [u0, 0.8])
    assert got["centers"][1] == dup and all(got["Y"][1, j] == v for j, v in last.items())


def test_a_zero_draw_in_one_round():
    p = quad_problem(1023)
    ref, got = check(p, 500, [0.3, 0.0, 0.7, 0.2])
    assert got["centers"][2] == 0 and got["weights"][1][0] > 0


def test_later_centres_keep_their_computed_weight_logistic():
    """LogisticLoss: a centre's distance to itself is not 0, so a zeroed weight would show."""
    p = Problem(ragged(200, seed=11), 70, 5, kinds=("logistic",), seed=11)
    ref, got = check(p, 17, np.random.default_rng(12).random(4))
    c = got["centers"]
    for l in range(1, 4):                                       # round l + 1 sees the centres 1 .. l as candidates
        for prev in c[1:l + 1]:
            if prev != c[0]:
                assert got["weights"][l][prev] > 0
    assert np.all(got["weights"][:, c[0]] == 0.0)


@pytest.mark.parametrize("kinds", [MIX, ("quad", "periodic")])
def test_per_column_mixed_losses(kinds):
    p = Problem(ragged(300, seed=13), 70, 5, kinds=kinds, seed=13)
    assert len(pack_losses(p.losses)) == 70
    check(p, 123, np.random.default_rng(14).random(4))


def test_handles_with_different_tiled_options_agree():
    p = quad_problem(1025)
    u = np.random.default_rng(15).random(4)
    ref = p.reference(9, u)
    assert np.all(ref["margins"] >= 1e-9)
    a, b, c = p.engine(9, u, tiled=1), p.engine(9, u, tiled=2), p.engine(9, u)
    compare(ref, a)
    assert a["centers"].tolist() == b["centers"].tolist() == c["centers"].tolist()
    assert same_bits(a["Y"], b["Y"]) and same_bits(a["Y"], c["Y"])


@pytest.mark.parametrize("n, tile_sort", [(70, False), (6000, True)])
def test_a_handle_that_reorders_its_row_lists_keeps_the_last_listed_value(n, tile_sort, monkeypatch):
    """The private copy of the row view in ANOTHER order than the caller's: with a loss descriptor per column the LDS-tiled family
    (tiled = 2) groups every tile window of a row by loss kind, and -- second case, more columns than a tile holds, lists in random
    order -- sorts the rows into tile order first (GLRM_HIP_TILE_SORT=2 lets an explicit tiled = 2 sort, as the automatic choice does at
    2e7 observations).  Both re-orderings are stable per column, which is what the scatter's rule `the largest list position writes`
    rests on: row 4 lists 128 columns twice with different values and is a centre by first_center and by u."""
    if tile_sort:
        monkeypatch.setenv("GLRM_HIP_TILE_SORT", "2")
    p = Problem(ragged(300, seed=21), n, 3, kinds=MIX, seed=21, dup_rows=(4,))
    dup = 4
    b, e = p.rowptr[dup], p.rowptr[dup + 1]
    assert len(set(p.colidx[b:e].tolist())) < e - b
    last = {int(j): v for j, v in zip(p.colidx[b:e], p.rowvals[b:e])}
    assert any(last[int(j)] != v for j, v in zip(p.colidx[b:e], p.rowvals[b:e]))      # some earlier duplicate holds another value
    w = p.reference(0, [0.5, 0.5])["weights"][0]
    cum = np.cumsum(w)
    u0 = (cum[dup - 1] + 0.5 * w[dup]) / cum[-1]
    for first, u in ((dup, [0.4, 0.8]), (0, [u0, 0.8])):
        ref, got = check(p, first, u, tiled=2)
        plain = p.engine(first, u, tiled=1)
        l = 0 if first == dup else 1
        assert got["centers"][l] == dup and all(got["Y"][l, j] == v for j, v in last.items())
        assert plain["centers"].tolist() == got["centers"].tolist() and same_bits(plain["Y"], got["Y"])
        print("weights of the two handles bit-equal:", same_bits(plain["weights"], got["weights"]))


def test_the_same_call_twice_returns_the_same_bits():
    p = Problem(ragged(1500, seed=16), 70, 5, kinds=MIX, seed=16)
    u = np.random.default_rng(17).random(4)
    api = hip()
    h = api.create(p.arrays())
    try:
        outs = []
        for _ in range(2):
            Y = p.Y0.copy(order="F")
            c, w = api.init_kmeanspp(h, Y, 33, u, want_weights=True, m=p.m)
            outs.append((Y, c, w))
    finally:
        api.destroy(h)
    assert same_bits(outs[0][2], outs[1][2]) and same_bits(outs[0][0], outs[1][0]) and outs[0][1].tolist() == outs[1][1].tolist()


def test_two_blobs_end_to_end():
    """test/runtests.jl:19-25 with the reference's own initializer: N(+5, I) x 100 and N(-5, I) x 50, k = 2, init_kmeanspp! and the
    k-means fit (UnitOneSparse rx, ZeroReg ry, inner_iter = 10) give clusters of 100 and 50."""
    seed = 0
    rng = np.random.default_rng(seed)
    A = np.vstack([rng.standard_normal((100, 2)) + 5.0, rng.standard_normal((50, 2)) - 5.0])
    g = L.GLRM(A, L.QuadLoss(), L.UnitOneSparseConstraint(), L.ZeroReg(), 2, rng=rng)
    draws = np.random.default_rng(seed + 1000)
    twin = np.random.default_rng(seed + 1000)
    Y0, first, u = twin.standard_normal((2, 2)), int(twin.integers(150)), twin.random(1)
    ref = R.init_kmeanspp(150, 2, 2, g._rowptr, g._colidx, g._rowvals, list(g.losses), Y0, first, u)
    assert (ref["centers"][0] < 100) != (ref["centers"][1] < 100)      # the transcription seeds one centre per blob
    assert ref["margins"][0] >= 1e-9
    L.init_kmeanspp_(g, draws)
    assert g._init_kmeanspp_info["centers"].tolist() == ref["centers"].tolist() and same_bits(g.Y, ref["Y"])
    X, Y, ch = L.fit_b(g, L.ProxGradParams(inner_iter=10), verbose=False)
    assert set(X.sum(axis=1).astype(int).tolist()) == {100, 50}
    g.close()


def test_refusals():
    rng = np.random.default_rng(6)
    api = hip()
    g = L.GLRM(rng.standard_normal((64, 48)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 16)
    Y, u = np.zeros((16, 48), order="F"), np.full(15, 0.5)

    def refused(h, code, first=0, uu=u):
        try:
            with pytest.raises(_capi.GLRMError) as ei:
                api.init_kmeanspp(h, Y, first, uu)
            assert ei.value.code == code, ei.value
        finally:
            api.destroy(h)

    refused(api.create(g.problem_arrays(dense=True)), _capi.ERR_UNSUPPORTED)
    refused(api.create(g.problem_arrays(rows=(0, 32))), _capi.ERR_INVALID)
    refused(api.create(g.problem_arrays(), defer=True), _capi.ERR_INVALID)
    refused(api.create(g.problem_arrays()), _capi.ERR_INVALID, first=64)
    refused(api.create(g.problem_arrays()), _capi.ERR_INVALID, first=-1)
    refused(api.create(g.problem_arrays()), _capi.ERR_INVALID, uu=np.concatenate([u[:-1], [1.0]]))
    refused(api.create(g.problem_arrays()), _capi.ERR_INVALID, uu=np.concatenate([[np.nan], u[1:]]))
    gm = L.GLRM(np.ones((8, 2)), [L.QuadLoss(), L.MultinomialLoss(3)], L.ZeroReg(), L.ZeroReg(), 2)
    h = api.create(gm.problem_arrays())
    try:
        with pytest.raises(_capi.GLRMError) as ei:
            api.init_kmeanspp(h, np.zeros((2, 2), order="F"), 0, [0.5])
        assert ei.value.code == _capi.ERR_UNSUPPORTED and "no slot for a multi-dimensional loss" in ei.value.message
    finally:
        api.destroy(h)
