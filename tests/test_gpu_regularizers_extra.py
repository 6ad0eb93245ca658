"""-m gpu: the vector regularizers QuadConstraint, NonNegOneReg, OneSparseConstraint, KSparseConstraint and SimplexConstraint on the device.

1. prox and evaluate through the test hook (glrm_test_reg_prox_eval, test build only) on every code path -- the six lane layouts of the
   sweep families, the reference-order path, the general sweeps' vector path -- against the Python mirrors: EXACTLY for four kinds; for
   QuadConstraint within (k + 4) 2^-53 relative per entry (reordering a sum of k non-negative squares, plus the square root, the divide and
   the multiply).  evaluate() is an indicator for four kinds (compared exactly); NonNegOneReg's scale * sum(a) adds k non-negative terms in
   another order than numpy and is held to (k + 1) 2^-53 relative.
2. whole fits on every sweep family, in reference-order mode and through the fixed-step (SparseProxGradParams) half-steps against
   numpy_proxgrad / a numpy restatement of the step, at the project's contract TOL (tests/test_gpu_parity.py).  Models and seeds:
   tests/regs_extra.py (the CPU suite checks that no seed forks under summation order).
3. the general sweeps: an offset model against numpy_proxgrad; a MultinomialLoss model by invariants; refusals.
4. shards against the single-device fit, bit for bit.   5. a live handle whose regularizers are replaced; invalid parameters."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cases
import lowrankmodels.jl_amd as L
import regs_extra as RX
import shapes
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd import regularizers as R
from test_gpu_edge_shapes import ALL_BITS, BLOCKED_C, BLOCKED_R, CACHED, FAMILY_RANK, LANE_C, LANE_R, SWITCHES, TILED_C, TILED_R
from test_gpu_parity import TOL
from test_oracle_vs_numpy import numpy_proxgrad

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
KS = (1, 2, 3, 7, 8, 9, 16, 17, 32, 33, 64, 65, 128)
#: code path -> (hook path, G, R, ranks it holds).  The lane layouts hold the ranks whose padded rank is theirs (both edges of each); the
#: lane-per-segment form (2, 16) exists at padded rank 32; reference order and the general sweeps exist up to rank 64.
LAYOUTS = {"(4,2)": (4, 2, 1, 8), "(4,4)": (4, 4, 9, 16), "(4,8)": (4, 8, 17, 32), "(8,8)": (8, 8, 33, 64), "(16,8)": (16, 8, 65, 128),
           "(2,16)": (2, 16, 17, 32)}


def hook(reg, k, alpha, path, G, Rr, U):
    """prox (nvec x kp, padding included), evaluate(u), evaluate(prox) through one code path of the test build."""
    fn = _capi.hip_testing_api().lib.glrm_test_reg_prox_eval
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    U = np.ascontiguousarray(U, dtype=np.float64)
    desc = R.pack_regs([reg])
    out, e0, e1 = np.full((len(U), G * Rr), 7.0), np.zeros(len(U)), np.zeros(len(U))
    rc = fn(desc.ctypes.data, k, float(alpha), path, G, Rr, U.ctypes.data, len(U), out.ctypes.data, e0.ctypes.data, e1.ctypes.data)
    assert rc == 0, (rc, _capi.hip_testing_api().last_error())
    return out, e0, e1


def _tree(v):
    """xor butterfly over a power-of-two number of slots: adjacent pairs, then pairs of pairs, ..."""
    v = [float(x) for x in v]
    while len(v) > 1:
        v = [v[i] + v[i + 1] for i in range(0, len(v), 2)]
    return v[0]


def device_sum(x, path, G, Rr):
    """sum of the entries of x in the order a code path adds them: reg_eval (lane j adds its double2 slices x + y in slice order, the G
    lanes by butterfly), ref_reg_eval (component order), block_reg_eval<1> (one entry per thread, butterfly over the 64 threads)."""
    x = [float(v) for v in x]
    if path == 1:
        s = 0.0
        for v in x:
            s += v
        return s
    if path == 2:
        return _tree([0.0 + v for v in x] + [0.0] * (64 - len(x)))
    x = x + [0.0] * (G * Rr - len(x))
    lanes = []
    for j in range(G):
        s = 0.0
        for i in range(Rr // 2):
            c0 = i * 2 * G + 2 * j
            s += x[c0] + x[c0 + 1]
        lanes.append(s)
    return _tree(lanes)


def vectors(rng, k, reg):
    """random, with exact zeros, all negative, already feasible, the zero vector (no ties in |u| or u except among exact zeros)."""
    v = [rng.standard_normal(k) * s for s in (1.0, 0.01, 30.0)]
    z = rng.standard_normal(k); z[rng.random(k) < 0.5] = 0.0
    v += [z, -np.abs(rng.standard_normal(k)) - 0.1, np.zeros(k)]
    base = reg.r if isinstance(reg, R._Wrapper) else reg
    n = k - 1 if isinstance(reg, R._Wrapper) else k
    f = np.abs(rng.standard_normal(k))
    if isinstance(base, L.SimplexConstraint) and n > 0:
        f[:n] = rng.dirichlet(np.ones(n))
    elif isinstance(base, L.QuadConstraint) and n > 0:
        f[:n] *= 0.5 * base.max_2norm / np.linalg.norm(f[:n])
    elif isinstance(base, (L.OneSparseConstraint, L.KSparseConstraint)) and n > 0:
        keep = 1 if isinstance(base, L.OneSparseConstraint) else base.k
        f[:n][rng.permutation(n)[keep:]] = 0.0
    if isinstance(reg, L.lastentry1):
        f[-1] = 1.0
    return np.array(v + [f])


def regs_for(k, wrappers):
    out = [L.QuadConstraint(1.5), L.NonNegOneReg(0.3), L.OneSparseConstraint(), L.SimplexConstraint()]
    out += [L.KSparseConstraint(r) for r in sorted({1, max(k - 1, 1), k})]
    if wrappers and k >= 2:
        out += [L.lastentry1(L.SimplexConstraint()), L.lastentry_unpenalized(L.QuadConstraint(2.0))]
        out += [L.lastentry_unpenalized(L.KSparseConstraint(r)) for r in sorted({1, k - 1})] + [L.lastentry1(L.OneSparseConstraint())]
    return out


def check_path(path, G, Rr, k, wrappers=False):
    rng = np.random.default_rng(1000 * path + 10 * k + G)
    kp = G * Rr
    for reg in regs_for(k, wrappers):
        U = vectors(rng, k, reg)
        alpha = 0.37
        got, e0, e1 = hook(reg, k, alpha, path, G, Rr, U)
        assert np.all(got[:, k:] == 0.0) and not np.any(np.signbit(got[:, k:])), ("padding", reg, k, path, G, Rr)
        base = reg.r if isinstance(reg, R._Wrapper) else reg
        for i, u in enumerate(U):
            want = np.asarray(reg.prox(u, alpha), dtype=float)
            if isinstance(base, L.QuadConstraint):
                n = k - 1 if isinstance(reg, R._Wrapper) else k
                if not np.any(u[:n]):     # the zero vector: NaN, and the trial that follows is rejected
                    assert np.all(np.isnan(got[i, :n])) and np.all(np.isnan(want[:n])), (reg, k, i, got[i, :k])
                    assert np.array_equal(got[i, n:k], want[n:k])
                else:
                    err = np.abs(got[i, :k] - want) / np.maximum(np.abs(want), 1e-300)
                    assert np.all(err[want != 0] <= (n + 4) * EPS) and np.all(got[i, :k][want == 0] == 0), (reg, k, i, err.max() / EPS)
            else:
                assert np.array_equal(got[i, :k], want), (reg, k, path, (G, Rr), i, u, got[i, :k], want)
            for e, x in ((e0[i], u), (e1[i], got[i, :k])):
                w = float(reg.evaluate(x))
                if isinstance(reg, L.NonNegOneReg) and np.isfinite(w):   # scale * sum(a), added in the code path's order
                    w = reg.param * device_sum(x, path, G, Rr)
                assert e == w, ("evaluate", reg, k, path, (G, Rr), i, x, e, w)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_hook_lane_layouts_match_the_mirrors(name):
    G, Rr, lo, hi = LAYOUTS[name]
    ks = [k for k in KS if lo <= k <= hi]
    assert ks[0] == lo and ks[-1] == hi
    for k in ks:
        check_path(0, G, Rr, k)


def test_hook_reference_order_path_matches_the_mirrors():
    for k in [k for k in KS if k <= 64]:
        kp, G = shapes.padded_rank(k)
        check_path(1, G, kp // G, k)


def test_hook_general_sweep_vector_path_matches_the_mirrors():
    """also as the base of lastentry1 / lastentry_unpenalized, where the base sees the first k - 1 entries"""
    for k in [k for k in KS if k <= 64]:
        kp, G = shapes.padded_rank(k)
        check_path(2, G, kp // G, k, wrappers=True)


# ------------------------------------------------------------------------------------------------ fits

@functools.lru_cache(maxsize=None)
def reference(key):
    name, k, inner = key
    mdl = RX.model(name, k, RX.FITS[key], inner)
    A, losses, rx, ry, feats, exs, X0, Y0, p = mdl
    Xn, Yn, chn, _, _ = numpy_proxgrad(A, losses, rx, ry, feats, exs, X0, Y0, p)
    for a in (Xn, Yn):
        a.setflags(write=False)
    return mdl, RX.glrm_of(mdl, k).problem_arrays(), Xn, Yn, tuple(chn)


def set_family(monkeypatch, env):
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)


def expected_flags(family, kp):
    if family == "gather":
        return 0
    if family == "cached":
        return CACHED if kp in (32, 64) else 0
    if family in ("four-lane tiles", "lane"):   # the lane-per-segment form exists at a padded rank of 32
        return TILED_R | TILED_C | (LANE_R | LANE_C if family == "lane" and kp == 32 else 0)
    return BLOCKED_R | BLOCKED_C


def against_numpy(obj, X, Y, ref, what):
    _, _, Xn, Yn, chn = ref
    assert len(obj) == len(chn), (what, len(obj), len(chn))
    e = (cases.rel_err(obj, chn), cases.fro_err(X, Xn), cases.fro_err(Y, Yn))
    print(what, "rel err objective / X / Y:", e)
    assert max(e) < TOL, (what, e)


SCALAR_FITS = [key for key in RX.FITS if key[0] != "offset"]


@pytest.mark.parametrize("key", SCALAR_FITS, ids=lambda k: f"{k[0]}-k{k[1]}-inner{k[2]}")
def test_fits_on_every_family_and_in_reference_order(monkeypatch, key):
    ref = reference(key)
    mdl, pa = ref[0], ref[1]
    X0, Y0, p = np.asfortranarray(mdl[6]), np.asfortranarray(mdl[7]), mdl[8]
    kp, _ = shapes.padded_rank(key[1])
    api = _capi.hip_api()
    for family, (env, kw) in FAMILY_RANK.items():
        set_family(monkeypatch, env)
        obj, X, Y, st = cases.run_engine(api, pa, X0, Y0, p, **kw)
        assert st["tiled"] & ALL_BITS == expected_flags(family, kp), (family, st["tiled"])
        against_numpy(obj, X, Y, ref, (key, family))
    set_family(monkeypatch, {})
    obj, X, Y, st = cases.run_engine(api, pa, X0, Y0, p, sum_order=1)
    assert st["tiled"] & 128, st["tiled"]
    against_numpy(obj, X, Y, ref, (key, "reference order"))


@pytest.mark.parametrize("key", [k for k in SCALAR_FITS if k[2] == 1], ids=lambda k: f"{k[0]}-k{k[1]}")
def test_fixed_step_half_steps(monkeypatch, key):
    """The SparseProxGradParams step (glrm_hip_gradstep_x / _y: one global step size, no line search) on the gather and the tiled sweeps."""
    mdl, pa = reference(key)[:2]
    A, losses, rx, ry, feats, exs, X0, Y0, p = mdl
    alpha = 0.8
    Xn, Yn = RX.numpy_gradstep(A, losses, rx, ry, feats, exs, X0, Y0, alpha)
    api, dev = _capi.hip_api(), torch.device("cuda", 0)
    for family in ("gather", "four-lane tiles"):
        env, kw = FAMILY_RANK[family]
        set_family(monkeypatch, env)
        h = api.create(pa, **kw)
        try:
            ld = api.factor_ld(h)
            bufs = [torch.zeros(pa.m * ld, dtype=torch.float64, device=dev), torch.zeros(pa.d * ld, dtype=torch.float64, device=dev),
                    torch.zeros(pa.n, dtype=torch.float64, device=dev), torch.zeros(pa.m, dtype=torch.float64, device=dev)]
            torch.cuda.synchronize()
            api.bind_buffers(h, *[b.data_ptr() for b in bufs])
            api.set_factors(h, np.asfortranarray(X0), np.asfortranarray(Y0))
            api.gradstep_x(h, alpha)
            api.gradstep_y(h, alpha)
            X, Y = np.zeros_like(X0, order="F"), np.zeros_like(Y0, order="F")
            api.get_factors(h, X, Y)
        finally:
            api.destroy(h)
        e = (cases.fro_err(X, Xn), cases.fro_err(Y, Yn))
        print(key, family, "fixed step rel err X / Y:", e)
        assert max(e) < TOL, (key, family, e)


# ------------------------------------------------------------------------------------------------ general sweeps

def test_general_sweeps_offset_model_against_numpy():
    """add_offset!: lastentry1(SimplexConstraint()) on X, lastentry_unpenalized(QuadReg) on Y, k = 4"""
    key = ("offset", 4, 1)
    ref = reference(key)
    mdl, pa = ref[0], ref[1]
    obj, X, Y, st = cases.run_engine(_capi.hip_api(), pa, np.asfortranarray(mdl[6]), np.asfortranarray(mdl[7]), mdl[8])
    assert st["tiled"] & 8, st["tiled"]
    against_numpy(obj, X, Y, ref, key)
    assert np.all(X[-1] == 1.0) and np.all(X[:-1] >= 0) and np.allclose(X[:-1].sum(axis=0), 1, rtol=0, atol=1e-14)


def multinomial_model():
    rng = np.random.default_rng(31)
    losses = [L.MultinomialLoss(4)] + [L.QuadLoss() for _ in range(6)]
    kw, _ = cases._multidim_data(rng, 28, 5, losses, RX.hello_world_rx(28), L.QuadReg(0.2), L.ProxGradParams(max_iter=8))
    return kw


def test_general_sweeps_multinomial_column_with_the_hello_world_rows():
    """No reference arithmetic exists for this combination (the oracle is frozen): invariants."""
    kw = multinomial_model()
    pa = L.GLRM(**kw).problem_arrays()
    X0, Y0 = np.asfortranarray(kw["X"]), np.asfortranarray(kw["Y"])
    api = _capi.hip_api()
    runs = [cases.run_engine(api, pa, X0, Y0, L.ProxGradParams(max_iter=8)) for _ in range(2)]
    (obj, X, Y, st), (obj2, X2, Y2, _) = runs
    assert st["tiled"] & 8
    assert np.array_equal(obj, obj2) and np.array_equal(X, X2) and np.array_equal(Y, Y2)       # two runs are bit-identical
    assert len(obj) == 9 and np.all(np.isfinite(obj[1:])) and np.all(np.diff(obj[1:]) <= 0), obj
    for it in range(1, 9):   # the trajectory is deterministic: the fit of `it` iterations is its prefix
        o, Xi, _, _ = cases.run_engine(api, pa, X0, Y0, L.ProxGradParams(max_iter=it))
        assert np.array_equal(o, obj[:it + 1])
        assert np.all(np.count_nonzero(Xi[:, 3::4], axis=0) <= 2), it                          # the KSparseConstraint(2) rows


@pytest.mark.parametrize("kind", list(RX.NEW_KINDS))
def test_new_kinds_are_refused_on_blocks_and_under_ordinal_wrappers(kind):
    kw = multinomial_model()
    api = _capi.hip_api()
    name = type(RX.NEW_KINDS[kind]()).__name__
    for ry in ([RX.NEW_KINDS[kind]()] + [L.QuadReg(0.2)] * 6,                                  # on the 4-column block of the Multinomial column
               [L.QuadReg(0.2)] + [L.OrdinalReg(RX.NEW_KINDS[kind]())] + [L.QuadReg(0.2)] * 5,
               [L.QuadReg(0.2)] * 2 + [L.MNLOrdinalReg(RX.NEW_KINDS[kind]())] + [L.QuadReg(0.2)] * 4):
        pa = L.GLRM(**dict(kw, ry=ry)).problem_arrays()
        with pytest.raises(L.GLRMError) as ei:
            api.destroy(api.create(pa))
        assert ei.value.code == _capi.ERR_UNSUPPORTED and name in str(ei.value), str(ei.value)
    pa = L.GLRM(**dict(kw, ry=[L.QuadReg(0.2)] + [RX.NEW_KINDS[kind]()] * 6)).problem_arrays()   # fine on the scalar-loss columns
    api.destroy(api.create(pa))


# ------------------------------------------------------------------------------------------------ shards

@pytest.mark.parametrize("family", ["gather", "four-lane tiles"])
@pytest.mark.parametrize("bounds", [([0, 13, 37], [0, 9, 23]), ([0, 5, 21, 37], [0, 8, 9, 23])], ids=["2 shards", "3 shards"])
def test_shards_equal_the_single_device_fit_bit_for_bit(monkeypatch, family, bounds):
    """New kinds on some rows / columns of ONE shard only: that shard launches the VR kernels, the others do not, and nothing shows."""
    A, losses, _, _, feats, exs, X0, Y0, p = RX.model("hello_world", 5, 1)
    rx = [L.QuadReg(0.1)] * RX.M
    for i in range(14, 21):
        rx[i] = [L.KSparseConstraint(2), L.SimplexConstraint(), L.OneSparseConstraint()][i % 3]
    ry = [L.QuadReg(0.1)] * RX.N
    for j in range(9, 13):
        ry[j] = L.QuadConstraint(1.5) if j % 2 else L.NonNegOneReg(0.2)
    pa = L.GLRM(A, losses, rx, ry, 5, observed_features=feats, observed_examples=exs, X=X0, Y=Y0).problem_arrays()
    env, kw = FAMILY_RANK[family]
    set_family(monkeypatch, env)
    api = _capi.hip_api()
    X0, Y0 = np.asfortranarray(X0), np.asfortranarray(Y0)
    obj, X, Y, _ = cases.run_engine(api, pa, X0, Y0, p, **kw)
    objs, Xs, Ys, _ = cases.run_shards_on_one_device(api, pa, X0, Y0, p, bounds[0], bounds[1], **kw)
    assert np.array_equal(objs, obj[1:]) and np.array_equal(Xs, X) and np.array_equal(Ys, Y)
    assert np.all(np.count_nonzero(X[:, [14, 17, 20]], axis=0) <= 2) and np.all(np.isfinite(obj[1:]))


# ------------------------------------------------------------------------------------------------ live handle

def test_replacing_regularizers_on_a_live_handle_matches_fresh_handles():
    A, losses, _, ry, feats, exs, X0, Y0, p = RX.model("ksparse_rx", 5, 1)
    quad, ksp = [L.QuadReg(0.1)] * RX.M, [L.KSparseConstraint(2)] * RX.M
    make = lambda rx: L.GLRM(A, losses, rx, ry, 5, observed_features=feats, observed_examples=exs, X=X0, Y=Y0).problem_arrays()   # noqa: E731
    pa_q, pa_k = make(quad), make(ksp)
    api = _capi.hip_api()
    X, Y = np.asfortranarray(X0).copy(order="F"), np.asfortranarray(Y0).copy(order="F")
    h = api.create(pa_q)
    try:
        for pa in (pa_q, pa_k, pa_q):
            api.set_regularizers(h, pa.rx, pa.ry)
            Xf, Yf = X.copy(order="F"), Y.copy(order="F")
            obj, _ = api.fit(h, p, X, Y)
            objf, Xf, Yf, _ = cases.run_engine(api, pa, Xf, Yf, p)
            assert np.array_equal(obj, objf) and np.array_equal(X, Xf) and np.array_equal(Y, Yf)
            if pa is pa_k:
                assert np.all(np.count_nonzero(X, axis=0) <= 2)
    finally:
        api.destroy(h)


def test_two_point_regularization_path_matches_fresh_models():
    A, losses, _, _, feats, exs, X0, Y0, _ = RX.model("ksparse_rx", 5, 1)
    p = L.ProxGradParams(max_iter=6)
    make = lambda s, X, Y: L.GLRM(A, losses, [L.KSparseConstraint(2)] * RX.M, [L.QuadReg(s)] * RX.N, 5, observed_features=feats,   # noqa: E731
                                  observed_examples=exs, X=X.copy(), Y=Y.copy())
    train, test = make(1.0, X0, Y0), make(1.0, X0, Y0)
    tr, te, _, _ = L.regularization_path(train, test, params=p, reg_params=[1.0, 0.1], verbose=False)
    X, Y = X0, Y0
    for i, s in enumerate((1.0, 0.1)):   # scale_regularizer! leaves KSparseConstraint alone and sets QuadReg's scale
        g = make(s, X, Y)
        X, Y, _ = L.fit_b(g, p, verbose=False)
        nobs = sum(len(f) for f in feats)
        assert tr[i] == L.objective(g, X, Y, include_regularization=False) / nobs
        assert te[i] == tr[i]
        assert np.all(np.count_nonzero(X, axis=0) <= 2)


@pytest.mark.parametrize("desc", [(R.K_SPARSE, 0, 0.0), (R.K_SPARSE, 0, 6.0), (R.K_SPARSE, 0, 1.5), (R.K_SPARSE, R.WRAP_LASTENTRY1, 5.0),
                                  (R.QUAD_CONSTRAINT, 0, 0.0), (R.QUAD_CONSTRAINT, 0, -1.0), (R.QUAD_CONSTRAINT, 0, float("inf"))])
def test_invalid_parameters_are_refused_at_create_and_on_a_live_handle(desc):
    mdl = RX.model("ksparse_rx", 5, 1)
    pa = RX.glrm_of(mdl, 5).problem_arrays()
    bad = np.array([desc], dtype=_capi.REG_DTYPE)
    api = _capi.hip_api()
    for side in ("rx", "ry"):
        h = api.create(pa)
        try:
            with pytest.raises(L.GLRMError) as ei:
                api.set_regularizers(h, bad if side == "rx" else pa.rx, bad if side == "ry" else pa.ry)
            assert ei.value.code == _capi.ERR_INVALID, str(ei.value)
            obj, _ = api.fit(h, mdl[8], np.asfortranarray(mdl[6]).copy(order="F"), np.asfortranarray(mdl[7]).copy(order="F"))   # still usable
            assert np.all(np.isfinite(obj[1:]))
        finally:
            api.destroy(h)
    setattr(pa, "rx", bad)
    with pytest.raises(L.GLRMError) as ei:
        api.destroy(api.create(pa))
    assert ei.value.code == _capi.ERR_INVALID
    with pytest.raises(L.GLRMError) as ei:   # and an unknown kind stays unsupported
        setattr(pa, "rx", np.array([(10, 0, 1.0)], dtype=_capi.REG_DTYPE))
        api.destroy(api.create(pa))
    assert ei.value.code == _capi.ERR_UNSUPPORTED


def test_multi_device_set_regularizers_checks_every_shard_before_changing_any():
    """A descriptor the LAST shard refuses must leave the first shards as they were: the fit after the refusal equals the fit before it."""
    mdl = RX.model("hello_world", 5, 1)
    pa = RX.glrm_of(mdl, 5).problem_arrays()
    X0, Y0, p = np.asfortranarray(mdl[6]), np.asfortranarray(mdl[7]), mdl[8]
    api = _capi.hip_api()
    mh = api.multi_create(pa, 3, device_ids=[0, 0, 0])
    try:
        before = api.multi_fit(mh, p, X0.copy(order="F"), Y0.copy(order="F"))[0]
        rx = pa.rx.copy()
        rx[:] = (R.K_SPARSE, 0, 2.0)
        rx[-1] = (R.K_SPARSE, 0, 6.0)          # r = k + 1 on the last row, i.e. in the last shard
        with pytest.raises(L.GLRMError) as ei:
            api.multi_set_regularizers(mh, rx, pa.ry)
        assert ei.value.code == _capi.ERR_INVALID
        after = api.multi_fit(mh, p, X0.copy(order="F"), Y0.copy(order="F"))[0]
        assert np.array_equal(before, after)
        rx[-1] = (R.K_SPARSE, 0, 2.0)
        api.multi_set_regularizers(mh, rx, pa.ry)
        X, Y = X0.copy(order="F"), Y0.copy(order="F")
        obj, _ = api.multi_fit(mh, p, X, Y)
        assert np.all(np.count_nonzero(X, axis=0) <= 2) and np.all(np.isfinite(obj[1:]))
    finally:
        api.multi_destroy(mh)
