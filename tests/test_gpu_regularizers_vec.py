"""-m gpu: the regularizers that carry a vector -- fixed_latent_features, fixed_last_latent_features, RemQuadReg (include/glrm_hip_regvec.h)
-- on the device.

1. prox and evaluate through the test hook (glrm_test_regvec_prox_eval, test build only: block_prox / block_reg_eval<1, true> of the general
   sweeps) against the Python mirrors, bit for bit; a sum is the mirror's terms added in the path's own order (device_eval below).
2. whole fits (tests/regs_vec.py: six models x k in {5, 33}, one inner_iter = 4 case) against numpy_proxgrad at the contract TOL of
   tests/test_gpu_parity.py, through L.fit_b and through _capi; the pinned entries equal y exactly; the fixed-step half-steps against
   numpy_gradstep; the objective with regularization against the mirrors.  The engine's ABI has no read-back of the per-segment step
   sizes: they are held through every later iterate and objective, which are compared.
3. the reference's test/fixedfeatures_test.jl and test/mult_reg.jl replayed with numpy's generator.
4. glrm_hip_multi_* with 2 and 3 shards on device 0 against the single handle, bit for bit.
5. live handles: install, replace the vectors, replace the scales, drop the vectors, cross-validate (subset children inherit).
6. refusals, each with its code, the handle usable afterwards.   7. device memory stays flat."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cases
import lowrankmodels.jl_amd as L
import regs_extra as RX
import regs_vec as RV
import shapes
import test_gpu_regularizers_extra as GX
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd import regularizers as R
from test_gpu_parity import TOL
from test_oracle_vs_numpy import numpy_proxgrad

pytestmark = pytest.mark.gpu
INF = float("inf")


# ------------------------------------------------------------------------------------------------ 1. hook

def hook(reg, k, alpha, U):
    """prox (nvec x kp, padding included), evaluate(u), evaluate(prox) of a descriptor WITH its vector on the general sweeps' path."""
    fn = _capi.hip_testing_api().lib.glrm_test_regvec_prox_eval
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    U = np.ascontiguousarray(U, dtype=np.float64)
    kp = shapes.padded_rank(k)[0]
    desc = np.array([reg.descriptor()], dtype=_capi.REG_DTYPE)
    vec = np.ascontiguousarray(reg.vector(), dtype=np.float64)
    out, e0, e1 = np.full((len(U), kp), 7.0), np.zeros(len(U)), np.zeros(len(U))
    rc = fn(desc.ctypes.data, vec.ctypes.data, len(vec), k, kp, float(alpha), U.ctypes.data, len(U), out.ctypes.data, e0.ctypes.data, e1.ctypes.data)
    assert rc == 0, (rc, _capi.hip_testing_api().last_error())
    return out, e0, e1


def tree(terms):
    """block_sum<1>: one term per thread (k <= 64), xor butterfly over the 64 threads (device_sum of tests/test_gpu_regularizers_extra.py)."""
    return GX.device_sum(terms, 2, 0, 0)


def base_eval(base, x):
    """block_reg_eval<1, true> of an unwrapped base regularizer on the vector x: 0 / Inf as the mirror says, sums in the path's order."""
    x = np.asarray(x, dtype=float)
    if isinstance(base, L.QuadReg):
        return base.scale * tree(x * x)               # fma(x, x, 0) per thread
    if isinstance(base, L.OneReg):
        return base.scale * tree(np.abs(x))
    if isinstance(base, L.NonNegOneReg):
        return INF if np.any(x < 0) else base.param * tree(x)
    return float(base.evaluate(x))                    # indicators (and ZeroReg)


def device_eval(reg, x):
    x = np.asarray(x, dtype=float)
    if isinstance(reg, L.RemQuadReg):                 # scale * sum (x_c - m_c)^2, one term per thread
        d = x - reg.m
        return reg.scale * tree(d * d)
    n = reg.n
    pin, sub = (x[:n], x[n:]) if isinstance(reg, L.fixed_latent_features) else (x[len(x) - n:], x[:len(x) - n])
    return base_eval(reg.r, sub) if np.array_equal(pin, reg.y) else INF


def quad_constraint_prox(base, u):
    """QuadConstraint's prox with the sum of squares accumulated in component order, as vector_prox_serial does (np.sum adds pairwise: the
    existing hook test holds this kind to (n + 4) 2^-53 for that reason; here the path's own order is restated and compared exactly)."""
    s = 0.0
    for v in u:
        s += v * v
    with np.errstate(divide="ignore", invalid="ignore"):
        return (base.max_2norm / np.sqrt(s)) * np.asarray(u, dtype=float)


def mirror_prox(reg, u, alpha):
    if isinstance(reg, R._FixedFeatures) and isinstance(reg.r, L.QuadConstraint):
        body = quad_constraint_prox(reg.r, u[reg.n:])
        return np.concatenate([reg.y, body] if isinstance(reg, L.fixed_latent_features) else [body, reg.y])
    return np.asarray(reg.prox(u, alpha), dtype=float)


def same_bits(a, b):
    """equal as numbers AND in the sign of zeros; a NaN matches a NaN"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    num = ~np.isnan(a)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[num]), np.signbit(b[num]))


def same_value(e, w):
    return (np.isnan(e) and np.isnan(w)) or e == w


def bases_for(nsub):
    out = [L.ZeroReg(), L.QuadReg(0.3), L.OneReg(0.2), L.NonNegConstraint(), L.QuadConstraint(1.5), L.NonNegOneReg(0.3), L.SimplexConstraint()]
    if nsub >= 1:   # (argmax / partialsortperm of an empty vector: refused by the engine, test_refusals)
        out += [L.UnitOneSparseConstraint(), L.OneSparseConstraint()] + [L.KSparseConstraint(r) for r in sorted({1, nsub})]
    return out


def pin_variants(rng, y):
    """(pinned region, finite?) : equal to the pin, equal with the other zero sign, one ulp off, random, with NaN / +inf / -inf"""
    n = len(y)
    flip = y.copy(); flip[0] = -flip[0]                       # y[0] is a zero: IEEE == holds
    ulp = y.copy(); ulp[n - 1] = np.nextafter(ulp[n - 1], INF)
    out = [(y.copy(), True), (flip, True), (ulp, True), (rng.standard_normal(n), True)]
    for bad in (np.nan, INF, -INF):
        v = y.copy(); v[rng.integers(n)] = bad
        out.append((v, False))
    return out


def check_fixed(k, nfix, last):
    rng = np.random.default_rng(10000 * k + 10 * nfix + int(last))
    nsub, alpha = k - nfix, 0.37
    y = rng.standard_normal(nfix)
    y[0] = -0.0 if nfix % 2 else 0.0                           # a pinned zero of either sign
    for base in bases_for(nsub):
        reg = (L.fixed_last_latent_features if last else L.fixed_latent_features)(base, y)
        subs = GX.vectors(rng, nsub, base) if nsub else np.zeros((1, 0))
        U, finite = [], []
        for b in subs:
            for pin, fin in pin_variants(rng, y):
                U.append(np.concatenate([b, pin] if last else [pin, b]))
                finite.append(fin)
        U = np.array(U)
        got, e0, e1 = hook(reg, k, alpha, U)
        assert np.all(got[:, k:] == 0.0) and not np.any(np.signbit(got[:, k:])), ("padding", reg, k)
        for i, u in enumerate(U):
            assert same_value(e0[i], device_eval(reg, u)), ("evaluate", reg, k, i, u, e0[i], device_eval(reg, u))
            # fixed_last feeds the base u[nfix:], which reaches into the pinned region: a NaN / inf there goes through the base's prox, and
            # the element-wise kinds treat a NaN differently from numpy's maximum / minimum (as they do without a wrapper).  Those vectors
            # are held on evaluate above and on the pinned entries of the result; the rest of the result is compared for Zero / Quad bases.
            pinned = got[i, nsub:k] if last else got[i, :nfix]
            assert same_bits(pinned, y), ("pinned entries", reg, k, i, pinned, y)
            if last and not finite[i] and not isinstance(base, (L.ZeroReg, L.QuadReg)):
                continue
            want = mirror_prox(reg, u, alpha)
            body_g, body_w = (got[i, :nsub], want[:nsub]) if last else (got[i, nfix:k], want[nfix:])
            assert np.array_equal(body_g, body_w, equal_nan=True), ("prox", reg, k, i, u, got[i, :k], want)
            assert same_value(e1[i], device_eval(reg, got[i, :k])), ("evaluate(prox)", reg, k, i, got[i, :k], e1[i])


FIXED_SHAPES = sorted({(k, nfix) for k in (2, 5, 33, 64) for nfix in (1, k - 1, k)} | {(33, 11), (33, 20)})   # (5, 1) / (5, 4): both overlap cases too


@pytest.mark.parametrize("last", [False, True], ids=["fixed_latent_features", "fixed_last_latent_features"])
@pytest.mark.parametrize("shape", FIXED_SHAPES, ids=lambda s: f"k{s[0]}-nfix{s[1]}")
def test_hook_fixed_wrappers_match_the_mirrors(shape, last):
    check_fixed(shape[0], shape[1], last)


@pytest.mark.parametrize("k", [2, 5, 33, 64])
def test_hook_rem_quad_reg_matches_the_mirror(k):
    rng = np.random.default_rng(k)
    m = rng.standard_normal(k)
    m[0] = -0.0
    reg, alpha = L.RemQuadReg(0.7, m), 0.37
    U = [rng.standard_normal(k) * s for s in (1.0, 0.01, 30.0)] + [m.copy(), np.zeros(k), -np.zeros(k)]
    for bad in (np.nan, INF, -INF):
        v = rng.standard_normal(k); v[rng.integers(k)] = bad
        U.append(v)
    ulp = m.copy(); ulp[k - 1] = np.nextafter(ulp[k - 1], INF)
    U = np.array(U + [ulp])
    got, e0, e1 = hook(reg, k, alpha, U)
    assert np.all(got[:, k:] == 0.0) and not np.any(np.signbit(got[:, k:]))
    for i, u in enumerate(U):
        assert same_bits(got[i, :k], reg.prox(u, alpha)), (k, i, u, got[i, :k], reg.prox(u, alpha))
        assert same_value(e0[i], device_eval(reg, u)) and same_value(e1[i], device_eval(reg, got[i, :k])), (k, i)
    assert e0[3] == 0.0 and e0[-1] > 0.0                      # at the mean / one ulp off it


# ------------------------------------------------------------------------------------------------ 2. fits

@functools.lru_cache(maxsize=None)
def reference(key):
    name, k, inner = key
    mdl = RV.model(name, k, RV.FITS[key], inner)
    A, losses, rx, ry, feats, exs, X0, Y0, p = mdl
    Xn, Yn, chn, _, _ = numpy_proxgrad(A, losses, rx, ry, feats, exs, X0, Y0, p)
    for a in (Xn, Yn):
        a.setflags(write=False)
    return mdl, Xn, Yn, tuple(chn)


def against_numpy(obj, X, Y, ref, what):
    _, Xn, Yn, chn = ref
    assert len(obj) == len(chn), (what, len(obj), len(chn))
    e = (cases.rel_err(obj, chn), cases.fro_err(X, Xn), cases.fro_err(Y, Yn))
    print(what, "rel err objective / X / Y:", e)
    assert max(e) < TOL, (what, e)


@pytest.mark.parametrize("key", list(RV.FITS), ids=lambda k: f"{k[0]}-k{k[1]}-inner{k[2]}")
def test_fits_against_numpy_through_capi_and_fit_b(key):
    ref = reference(key)
    mdl, (name, k, _) = ref[0], key
    p = mdl[8]
    api = _capi.hip_api()
    obj, X, Y, st = RV.run_capi(api, RV.glrm_of(mdl, k), p)
    assert st["tiled"] & 8, st["tiled"]                       # the general sweeps
    against_numpy(obj, X, Y, ref, (key, "_capi"))
    assert (obj[0] == INF) == (name in RV.INF_START) and np.all(np.isfinite(obj[1:]))
    assert RV.pinned_ok(mdl[2], mdl[3], X, Y)
    g = RV.glrm_of(mdl, k)
    try:
        Xf, Yf, ch = L.fit_b(g, p, verbose=False)
        assert np.array_equal(ch.objective, obj) and np.array_equal(Xf, X) and np.array_equal(Yf, Y)
        assert RV.pinned_ok(g.rx, g.ry, g.X, g.Y)
    finally:
        g.close()


@pytest.mark.parametrize("key", [k for k in RV.FITS if k[2] == 1], ids=lambda k: f"{k[0]}-k{k[1]}")
def test_fixed_step_half_steps(key):
    """The SparseProxGradParams step (glrm_hip_gradstep_x / _y: one global step size, no line search), mode 2 of the general sweeps."""
    mdl = reference(key)[0]
    A, losses, rx, ry, feats, exs, X0, Y0, p = mdl
    alpha = 0.8
    Xn, Yn = RX.numpy_gradstep(A, losses, rx, ry, feats, exs, X0, Y0, alpha)
    api, dev = _capi.hip_api(), torch.device("cuda", 0)
    g = RV.glrm_of(mdl, key[1])
    pa = g.problem_arrays()
    h = RV.create_with_vectors(api, g)
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
    print(key, "fixed step rel err X / Y:", e)
    assert max(e) < TOL, (key, e)
    assert RV.pinned_ok(rx, ry, X, Y)


@pytest.mark.parametrize("key", [k for k in RV.FITS if k[2] == 1], ids=lambda k: f"{k[0]}-k{k[1]}")
def test_objective_with_regularization_against_the_mirrors(key):
    """L.objective(..., include_regularization=True): multi_penalty_kernel's evaluate, at the fitted point and (pins violated: inf) at the start."""
    mdl, Xn, Yn, _ = reference(key)
    A, losses, rx, ry, feats, exs, X0, Y0, p = mdl
    g = RV.glrm_of(mdl, key[1])

    def numpy_objective(X, Y, reg):
        err = sum(losses[j].evaluate(float(X[:, i] @ Y[:, j]), A[i, j]) for i in range(len(feats)) for j in feats[i])
        if reg:
            err += sum(rx[i].evaluate(X[:, i]) for i in range(X.shape[1])) + sum(ry[j].evaluate(Y[:, j]) for j in range(Y.shape[1]))
        return err
    try:
        for reg in (True, False):
            got, want = L.objective(g, Xn, Yn, include_regularization=reg), numpy_objective(Xn, Yn, reg)
            assert np.isfinite(want) and abs(got - want) <= 1e-11 * abs(want), (key, reg, got, want)
        got0, want0 = L.objective(g, X0, Y0, include_regularization=True), numpy_objective(X0, Y0, True)
        assert (got0 == want0 == INF) if key[0] in RV.INF_START else abs(got0 - want0) <= 1e-11 * abs(want0), (key, got0, want0)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ 3. the reference's scripts

@pytest.mark.parametrize("last", [False, True], ids=["fixed_latent_features", "fixed_last_latent_features"])
def test_reference_script_fixedfeatures(last):
    """test/fixedfeatures_test.jl: Yp[1:k, :] == Y, respectively Yp[2:end, :] == Y -- exactly."""
    mdl, Yfix = RV.fixedfeatures_script(last)
    A, losses, rx, ry, feats, exs, X0, Y0, p = mdl
    g = L.GLRM(A, losses, rx, ry, 4, X=X0, Y=Y0)
    try:
        X, Y, ch = L.fit_b(g, p, verbose=False)
    finally:
        g.close()
    assert np.array_equal(Y[1:] if last else Y[:3], Yfix)
    Xn, Yn, chn, _, _ = numpy_proxgrad(A, losses, rx, ry, feats, exs, X0, Y0, p)
    against_numpy(np.array(ch.objective), X, Y, (None, Xn, Yn, chn), ("fixedfeatures", last))
    assert np.all(X >= 0) and np.allclose(X.sum(axis=0), 1, rtol=0, atol=1e-14)


def test_reference_script_mult_reg():
    """test/mult_reg.jl at its size: mseU < 1e-3 and mseV < 1e-3 (the numpy run gives 4.3e-4 and 5.6e-4 in 18 iterations)."""
    mdl, (U, V) = RV.mult_reg_script()
    A, losses, rx, ry, feats, exs, X0, Y0, p = mdl
    g = L.GLRM(A, losses, rx, ry, 5, X=X0, Y=Y0)
    try:
        Uh, Vh, ch = L.fit_b(g, p, verbose=False)
    finally:
        g.close()
    mseU, mseV = float(np.mean((U - Uh) ** 2)), float(np.mean((V - Vh) ** 2))
    print("mult_reg: MSE(U), MSE(V), iterations:", mseU, mseV, len(ch.objective) - 1)
    assert mseU < 1e-3 and mseV < 1e-3
    Xn, Yn, chn, _, _ = numpy_proxgrad(A, losses, rx, ry, feats, exs, X0, Y0, p)
    against_numpy(np.array(ch.objective), Uh, Vh, (None, Xn, Yn, chn), "mult_reg")


# ------------------------------------------------------------------------------------------------ 4. shards

def multi_fit_with_vectors(api, g, p, ns, rx=None, ry=None):
    """glrm_hip_multi_create on device 0 (placeholder descriptors), glrm_hip_multi_set_regularizers_vec, glrm_hip_multi_fit."""
    mh = api.multi_create(g.problem_arrays(), ns, device_ids=[0] * ns)
    try:
        info = api.multi_info(mh, ns)
        if rx is not None:
            g.rx, g.ry = rx(info), ry(info)
        api.multi_set_regularizers_vec(mh, *RV.vec_args(g.rx, g.ry, g.k))
        X, Y = np.array(g.X, order="F"), np.array(g.Y, order="F")
        obj, _ = api.multi_fit(mh, p, X, Y)
    finally:
        api.multi_destroy(mh)
    return obj, X, Y, info


@pytest.mark.parametrize("ns", [2, 3])
@pytest.mark.parametrize("name", ["mixed_rows", "remquad_both", "fixlast_ry"])
def test_shards_equal_the_single_handle_bit_for_bit(name, ns):
    mdl = RV.model(name, 5, 1)
    p = mdl[8]
    api = _capi.hip_api()
    obj, X, Y, _ = RV.run_capi(api, RV.glrm_of(mdl, 5), p)
    objs, Xs, Ys, info = multi_fit_with_vectors(api, RV.glrm_of(mdl, 5), p, ns)
    assert len(info["row_bounds"]) == ns + 1
    assert np.array_equal(objs, obj) and np.array_equal(Xs, X) and np.array_equal(Ys, Y)
    assert RV.pinned_ok(mdl[2], mdl[3], Xs, Ys)


@pytest.mark.parametrize("ns", [2, 3])
def test_only_one_shard_holds_a_vector(ns):
    """Vector-carrying descriptors on some rows and columns of the LAST shard only: that shard gets tables, the others none."""
    A, losses, _, _, feats, exs, X0, Y0, p = RV.model("remquad_both", 5, 1)
    rng = np.random.default_rng(77)
    P = rng.standard_normal((5, max(RX.M, RX.N)))

    def rows(info):
        lo = info["row_bounds"][-2]
        assert lo + 2 < RX.M
        return [L.fixed_latent_features(L.OneReg(0.1), P[:2, i]) if i >= lo + 1 and i % 2 else L.QuadReg(0.1) for i in range(RX.M)]

    def cols(info):
        lo = info["col_bounds"][-2]
        assert lo + 1 < RX.N
        return [L.RemQuadReg(0.4, P[:, j]) if j > lo else L.QuadReg(0.1) for j in range(RX.N)]
    make = lambda: L.GLRM(A, losses, [L.QuadReg(0.1)] * RX.M, [L.QuadReg(0.1)] * RX.N, 5, observed_features=feats, observed_examples=exs, X=X0, Y=Y0)   # noqa: E731
    api = _capi.hip_api()
    gm = make()
    gm.rx, gm.ry = [L.QuadReg(0.1 + 1e-3 * i) for i in range(RX.M)], [L.QuadReg(0.1 + 1e-3 * j) for j in range(RX.N)]   # per-entry counts at create
    objs, Xs, Ys, info = multi_fit_with_vectors(api, gm, p, ns, rows, cols)
    gs = make()
    gs.rx, gs.ry = rows(info), cols(info)
    obj, X, Y, _ = RV.run_capi(api, gs, p)
    assert np.array_equal(objs, obj) and np.array_equal(Xs, X) and np.array_equal(Ys, Y)
    assert RV.pinned_ok(gs.rx, gs.ry, Xs, Ys) and np.all(np.isfinite(obj[1:]))


# ------------------------------------------------------------------------------------------------ 5. live handles

def plain_model(mdl, k):
    A, losses, _, _, feats, exs, X0, Y0, _ = mdl
    return L.GLRM(A, losses, [L.QuadReg(0.1 + 1e-3 * i) for i in range(RX.M)], [L.QuadReg(0.1 + 1e-3 * j) for j in range(RX.N)], k,
                  observed_features=feats, observed_examples=exs, X=X0, Y=Y0)


@pytest.mark.parametrize("name", ["mixed_rows", "remquad_both"])
def test_installing_and_replacing_on_a_live_handle_matches_fresh_handles(name):
    mdl = RV.model(name, 5, 1)
    other = RV.model(name, 5, 2)                               # other vectors (and data: only its regularizers are used)
    p = mdl[8]
    api = _capi.hip_api()
    plain = plain_model(mdl, 5)
    g1 = RV.glrm_of(mdl, 5)
    g2 = RV.glrm_of(mdl, 5)
    g2.rx, g2.ry = other[2], other[3]
    X0, Y0 = np.asfortranarray(mdl[6]), np.asfortranarray(mdl[7])
    h = api.create(plain.problem_arrays())
    try:
        api.fit(h, p, X0.copy(order="F"), Y0.copy(order="F"))                 # a handle that has run on the fast families
        for g in (g1, g2, g1):                                               # install, replace only the vectors, and back
            api.set_regularizers_vec(h, *RV.vec_args(g.rx, g.ry, 5))
            X, Y = X0.copy(order="F"), Y0.copy(order="F")
            obj, _ = api.fit(h, p, X, Y)
            objf, Xf, Yf, _ = RV.run_capi(api, g, p)
            assert np.array_equal(obj, objf) and np.array_equal(X, Xf) and np.array_equal(Y, Yf)
            assert RV.pinned_ok(g.rx, g.ry, X, Y)
        # a plain glrm_hip_set_regularizers afterwards: as if the vectors had never been set.  Compared with a handle that reached the
        # general sweeps through a wrapper instead and then got the same plain descriptors.
        pa = plain.problem_arrays()
        api.set_regularizers(h, pa.rx, pa.ry)
        X, Y = X0.copy(order="F"), Y0.copy(order="F")
        obj, _ = api.fit(h, p, X, Y)
        h2 = api.create(pa)
        try:
            wrapped = pa.ry.copy()
            wrapped["wrap"] = R.WRAP_LASTENTRY_UNPENALIZED
            api.set_regularizers(h2, pa.rx, wrapped)
            api.set_regularizers(h2, pa.rx, pa.ry)
            X2, Y2 = X0.copy(order="F"), Y0.copy(order="F")
            obj2, _ = api.fit(h2, p, X2, Y2)
        finally:
            api.destroy(h2)
        assert np.array_equal(obj, obj2) and np.array_equal(X, X2) and np.array_equal(Y, Y2)
        A, losses, _, _, feats, exs = mdl[:6]
        Xn, Yn, chn, _, _ = numpy_proxgrad(A, losses, list(plain.rx), list(plain.ry), feats, exs, mdl[6], mdl[7], p)
        against_numpy(obj, X, Y, (None, Xn, Yn, chn), (name, "plain after vectors"))
    finally:
        api.destroy(h)


def test_a_table_of_zero_lengths_moves_the_handle_to_the_general_sweeps():
    """How the shards of one problem stay on one family (include/glrm_hip_regvec.h): a handle that is given a table runs the general sweeps even
    when its own slice holds no vector; with neither vector nor table the call is the plain one."""
    g, p = quad_model()
    api = _capi.hip_api()
    h = api.create(g.problem_arrays())
    try:
        fit_of(api, h, g, p)
        assert not api.kernel_stats(h)["tiled"] & 8
        api.set_regularizers_vec(h, QUAD1, None, QUAD1, None)
        fit_of(api, h, g, p)
        assert not api.kernel_stats(h)["tiled"] & 8
        api.set_regularizers_vec(h, QUAD1, (np.zeros(K), np.zeros(1, dtype=np.int32)), QUAD1, None)
        obj, X, Y = fit_of(api, h, g, p)
        assert api.kernel_stats(h)["tiled"] & 8
        A, losses, _, _, feats, exs = RV.model("remquad_both", 5, 1)[:6]
        Xn, Yn, chn, _, _ = numpy_proxgrad(A, losses, list(g.rx), list(g.ry), feats, exs, g.X, g.Y, p)
        against_numpy(obj, X, Y, (None, Xn, Yn, chn), "zero-length table")
    finally:
        api.destroy(h)


def test_a_changed_vector_reaches_the_warm_handle_of_a_model():
    """Through L: assigning a new vector changes the soft key; the SAME handle gets it (glrm_hip_set_regularizers_vec) and fits like a fresh model."""
    mdl = RV.model("fixfirst_ry", 5, 1)
    p = mdl[8]
    g = RV.glrm_of(mdl, 5)
    try:
        L.fit_b(g, p, verbose=False)
        h0 = g._handle_cache[1].value
        newy = [r.y + 0.25 for r in g.ry]
        for r, y in zip(g.ry, newy):
            r.y = y
        g.X[...], g.Y[...] = mdl[6], mdl[7]
        X, Y, ch = L.fit_b(g, p, verbose=False)
        assert g._handle_cache[1].value == h0
        fresh = RV.glrm_of(mdl, 5)
        fresh.ry = [L.fixed_latent_features(L.QuadReg(0.2), y) for y in newy]
        try:
            Xf, Yf, chf = L.fit_b(fresh, p, verbose=False)
        finally:
            fresh.close()
        assert np.array_equal(ch.objective, chf.objective) and np.array_equal(X, Xf) and np.array_equal(Y, Yf)
        assert np.array_equal(Y[:len(newy[0])], np.array(newy).T)
    finally:
        g.close()


@pytest.mark.parametrize("name", ["fixfirst_ry", "remquad_both"])
def test_two_point_regularization_path_matches_fresh_models(name):
    """Only the scales change (scale_regularizer!: forwarded to the base of a fixed wrapper, set on RemQuadReg); the vectors stay."""
    mdl = RV.model(name, 5, 1)
    A, losses, rx, ry, feats, exs, X0, Y0, _ = mdl
    p = L.ProxGradParams(max_iter=6)
    import copy

    def make(s, X, Y):
        g = L.GLRM(A, losses, copy.deepcopy(rx), copy.deepcopy(ry), 5, observed_features=feats, observed_examples=exs, X=X.copy(), Y=Y.copy())
        return L.scale_regularizer_(g, s) if s is not None else g
    train, test = make(None, X0, Y0), make(None, X0, Y0)
    tr, te, _, _ = L.regularization_path(train, test, params=p, reg_params=[1.0, 0.1], verbose=False)
    train.close(), test.close()
    X, Y = X0, Y0
    nobs = sum(len(f) for f in feats)
    for i, s in enumerate((1.0, 0.1)):
        g = make(s, X, Y)
        try:
            X, Y, _ = L.fit_b(g, p, verbose=False)
            assert tr[i] == L.objective(g, X, Y, include_regularization=False) / nobs and te[i] == tr[i]
        finally:
            g.close()
        X, Y = X.copy(), Y.copy()
    assert np.array_equal(train.X, X) and np.array_equal(train.Y, Y)


def test_cross_validate_children_inherit_the_vectors():
    """cross_validate on a fix_latent_features! model: the folds' handles are glrm_hip_subset children of the parent's.  They equal the
    same folds fitted as fresh models (fused=False: every fold creates its own handle and installs its own vectors)."""
    mdl = RV.model("remquad_both", 5, 1)
    A, losses, _, _, feats, exs, X0, Y0, _ = mdl
    p = L.ProxGradParams(max_iter=5)
    nobs = sum(len(f) for f in feats)
    groups = np.random.default_rng(9).integers(0, 2, nobs)

    def run(fused):
        g = L.GLRM(A, losses, [L.QuadReg(0.1)] * RX.M, [L.QuadReg(0.2)] * RX.N, 5, observed_features=feats, observed_examples=exs, X=X0.copy(), Y=Y0.copy())
        L.fix_latent_features_(g, 2)
        try:
            tre, tee, trg, teg = L.cross_validate(g, nfolds=2, params=p, verbose=False, groups=groups, fused=fused)
            out = (tre, tee, [t.X.copy() for t in trg], [t.Y.copy() for t in trg])
            for t in trg + teg:
                t.close()
        finally:
            g.close()
        return out, g
    (tre, tee, Xs, Ys), g = run(True)
    assert g._split_cache.canonical                           # the fused path was taken: the folds' handles were subsets
    (tre2, tee2, Xs2, Ys2), _ = run(False)
    assert np.array_equal(tre, tre2) and np.array_equal(tee, tee2) and np.all(np.isfinite(tre)) and np.all(np.isfinite(tee))
    for X, X2, Y, Y2 in zip(Xs, Xs2, Ys, Ys2):
        assert np.array_equal(X, X2) and np.array_equal(Y, Y2)
        assert np.array_equal(Y[:2], Y0[:2])                  # the first two latent features of every column stayed where they were


# ------------------------------------------------------------------------------------------------ 6. refusals

INVALID, UNSUPPORTED, NONFINITE = _capi.ERR_INVALID, _capi.ERR_UNSUPPORTED, _capi.ERR_NONFINITE
K = 5


def one(desc):
    return np.array([desc], dtype=_capi.REG_DTYPE)


def vec(values, n, k=K):
    t = np.zeros(k)
    t[:len(values)] = values
    return t, np.array([n], dtype=np.int32)


QUAD1 = one((R.QUAD, 0, 0.1))
REFUSALS = {
    "nfix = 0": (one((R.QUAD, R.WRAP_FIXED_FIRST, 0.1)), vec([], 0), INVALID),
    "nfix = k + 1": (one((R.QUAD, R.WRAP_FIXED_LAST, 0.1)), vec([1.0] * K, K + 1), INVALID),
    "RemQuadReg length != k": (one((R.REM_QUAD, 0, 1.0)), vec([1.0] * (K - 1), K - 1), INVALID),
    "KSparseConstraint r > k - nfix": (one((R.K_SPARSE, R.WRAP_FIXED_FIRST, 4.0)), vec([1.0, 2.0], 2), INVALID),
    "argmax base with nfix = k": (one((R.ONE_SPARSE, R.WRAP_FIXED_FIRST, 1.0)), vec([1.0] * K, K), INVALID),
    "no vector given": (one((R.REM_QUAD, 0, 1.0)), None, INVALID),
    "a length on a descriptor without a vector": (QUAD1, vec([1.0], 1), INVALID),
    "NaN in a vector": (one((R.QUAD, R.WRAP_FIXED_FIRST, 0.1)), vec([1.0, np.nan], 2), NONFINITE),
    "inf in a vector": (one((R.REM_QUAD, 0, 1.0)), vec([1.0, 2.0, INF, 0.0, 0.0], K), NONFINITE),
    "new flag with lastentry1": (one((R.QUAD, R.WRAP_FIXED_FIRST | R.WRAP_LASTENTRY1, 0.1)), vec([1.0], 1), UNSUPPORTED),
    "both new flags": (one((R.QUAD, R.WRAP_FIXED_FIRST | R.WRAP_FIXED_LAST, 0.1)), vec([1.0], 1), UNSUPPORTED),
    "RemQuadReg under a fixed wrapper": (one((R.REM_QUAD, R.WRAP_FIXED_LAST, 1.0)), vec([1.0], 1), UNSUPPORTED),
    "RemQuadReg under lastentry_unpenalized": (one((R.REM_QUAD, R.WRAP_LASTENTRY_UNPENALIZED, 1.0)), vec([1.0] * K, K), UNSUPPORTED),
}


def quad_model(k=K, **kw):
    A, losses, _, _, feats, exs, _, _, p = RV.model("remquad_both", 5, 1)
    rng = np.random.default_rng(4)
    X0, Y0 = rng.standard_normal((k, RX.M)), rng.standard_normal((k, RX.N))
    return L.GLRM(A, losses, L.QuadReg(0.1), L.QuadReg(0.1), k, observed_features=feats, observed_examples=exs, X=X0, Y=Y0, **kw), L.ProxGradParams(max_iter=4)


def fit_of(api, h, g, p):
    X, Y = np.array(g.X, order="F"), np.array(g.Y, order="F")
    obj, _ = api.fit(h, p, X, Y)
    return obj, X, Y


def expect_refusal(api, h, g, p, code, call, word=None):
    """The call is refused with `code`; the fit after the refusal equals the fit before it."""
    before = fit_of(api, h, g, p)
    with pytest.raises(L.GLRMError) as ei:
        call()
    assert ei.value.code == code, (code, str(ei.value))
    if word:
        assert word in ei.value.message, ei.value.message
    after = fit_of(api, h, g, p)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("side", ["rx", "ry"])
@pytest.mark.parametrize("case", list(REFUSALS))
def test_refused_descriptors_and_vectors(case, side):
    bad, v, code = REFUSALS[case]
    g, p = quad_model()
    api = _capi.hip_api()
    h = api.create(g.problem_arrays())
    try:
        args = (bad, v, QUAD1, None) if side == "rx" else (QUAD1, None, bad, v)
        expect_refusal(api, h, g, p, code, lambda: api.set_regularizers_vec(h, *args))
    finally:
        api.destroy(h)


def test_a_failed_call_keeps_the_vectors_that_were_installed():
    mdl = RV.model("mixed_rows", 5, 1)
    g, p = RV.glrm_of(mdl, 5), mdl[8]
    api = _capi.hip_api()
    h = RV.create_with_vectors(api, g)
    try:
        rx, vx, ry, vy = RV.vec_args(g.rx, g.ry, 5)
        broken = vy[0].copy()
        broken[5 * (RX.N - 1)] = np.nan                       # the last column's pin
        expect_refusal(api, h, g, p, NONFINITE, lambda: api.set_regularizers_vec(h, rx, vx, ry, (broken, vy[1])))
        obj, X, Y = fit_of(api, h, g, p)
        assert RV.pinned_ok(g.rx, g.ry, X, Y)
    finally:
        api.destroy(h)


def test_the_plain_entry_points_keep_refusing_the_new_codes():
    """glrm_hip_create / glrm_hip_set_regularizers: kind 10 stays GLRM_ERR_UNSUPPORTED, the new flags GLRM_ERR_INVALID -- a descriptor that
    needs a vector and arrives without one is never accepted."""
    g, p = quad_model()
    api = _capi.hip_api()
    pa = g.problem_arrays()
    h = api.create(pa)
    try:
        for desc, code in (((R.REM_QUAD, 0, 1.0), UNSUPPORTED), ((R.QUAD, R.WRAP_FIXED_FIRST, 0.1), INVALID), ((R.QUAD, R.WRAP_FIXED_LAST, 0.1), INVALID)):
            for side in ("rx", "ry"):
                expect_refusal(api, h, g, p, code, lambda: api.set_regularizers(h, one(desc) if side == "rx" else pa.rx, one(desc) if side == "ry" else pa.ry))
                setattr(pa, side, one(desc))
                with pytest.raises(L.GLRMError) as ei:
                    api.destroy(api.create(pa))
                assert ei.value.code == code
                setattr(pa, side, QUAD1)
    finally:
        api.destroy(h)


def test_handles_that_cannot_run_the_general_sweeps_refuse():
    api = _capi.hip_api()
    good = (one((R.REM_QUAD, 0, 1.0)), None)
    # k = 65
    g, p = quad_model(k=65)
    h = api.create(g.problem_arrays())
    try:
        expect_refusal(api, h, g, p, UNSUPPORTED, lambda: api.set_regularizers_vec(h, good[0], vec(np.ones(65), 65, 65), QUAD1, None), "k <= 64")
    finally:
        api.destroy(h)
    # storage = f32, sum_order = 1: the message names the mode
    for kw, word in ((dict(storage=1), "storage = f32"), (dict(sum_order=1), "sum_order = 1")):
        g, p = quad_model()
        h = api.create(g.problem_arrays(), **kw)
        try:
            expect_refusal(api, h, g, p, UNSUPPORTED, lambda: api.set_regularizers_vec(h, good[0], vec(np.ones(K), K), QUAD1, None), word)
            expect_refusal(api, h, g, p, UNSUPPORTED, lambda: api.set_regularizers_vec(h, QUAD1, None, one((R.QUAD, R.WRAP_FIXED_FIRST, 0.1)), vec([1.0], 1)), word)
        finally:
            api.destroy(h)
    # the dense hand-over
    rng = np.random.default_rng(6)
    gd = L.GLRM(rng.standard_normal((40, 24)), L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.1), 9, rng=rng)
    assert gd.dense_eligible()
    h = api.create(gd.problem_arrays(dense=True))
    try:
        expect_refusal(api, h, gd, L.ProxGradParams(max_iter=4), UNSUPPORTED,
                       lambda: api.set_regularizers_vec(h, good[0], vec(np.ones(9), 9, 9), QUAD1, None), "sparse-view")
    finally:
        api.destroy(h)


def test_a_multinomial_column_refuses_a_vector_carrying_regularizer():
    """On a column whose loss has dim > 1: the rule and the wording of the vector kinds."""
    kw = GX.multinomial_model()
    g = L.GLRM(**dict(kw, ry=[L.QuadReg(0.2 + 0.01 * j) for j in range(7)]))      # one descriptor per column
    k, n = g.k, len(g.ry)
    api = _capi.hip_api()
    pa = g.problem_arrays()
    h = api.create(pa)
    p = L.ProxGradParams(max_iter=4)
    try:
        rx = pa.rx
        for desc, ln, name in (((R.REM_QUAD, 0, 1.0), k, "RemQuadReg"), ((R.QUAD, R.WRAP_FIXED_FIRST, 0.2), 1, "fixed_latent_features"),
                               ((R.QUAD, R.WRAP_FIXED_LAST, 0.2), 1, "fixed_last_latent_features")):
            ry = np.array([desc] + [(R.QUAD, 0, 0.2)] * (n - 1), dtype=_capi.REG_DTYPE)
            lens = np.array([ln] + [0] * (n - 1), dtype=np.int32)
            expect_refusal(api, h, g, p, UNSUPPORTED, lambda: api.set_regularizers_vec(h, rx, None, ry, (np.ones(k * n), lens)),
                           f"{name} is a vector regularizer and cannot regularize the 4-column block of column 0")
        ry = np.array([(R.QUAD, 0, 0.2)] + [(R.REM_QUAD, 0, 1.0)] * (n - 1), dtype=_capi.REG_DTYPE)     # fine on the scalar-loss columns
        api.set_regularizers_vec(h, rx, None, ry, (np.ones(k * n), np.array([0] + [k] * (n - 1), dtype=np.int32)))
        obj, _, _ = fit_of(api, h, g, p)
        assert np.all(np.isfinite(obj[1:]))
    finally:
        api.destroy(h)


def test_multi_handle_checks_every_shard_before_changing_any():
    """A vector the LAST shard refuses must leave the first shards as they were: the fit after the refusal equals the fit before it."""
    mdl = RV.model("remquad_both", 5, 1)
    g, p = RV.glrm_of(mdl, 5), mdl[8]
    api = _capi.hip_api()
    mh = api.multi_create(g.problem_arrays(), 3, device_ids=[0, 0, 0])
    try:
        X0, Y0 = np.asfortranarray(mdl[6]), np.asfortranarray(mdl[7])
        before = api.multi_fit(mh, p, X0.copy(order="F"), Y0.copy(order="F"))[0]
        rx, vx, ry, vy = RV.vec_args(g.rx, g.ry, 5)
        bad = vx[0].copy()
        bad[5 * (RX.M - 1) + 2] = np.nan                      # in the last row's mean, i.e. in the last shard
        with pytest.raises(L.GLRMError) as ei:
            api.multi_set_regularizers_vec(mh, rx, (bad, vx[1]), ry, vy)
        assert ei.value.code == NONFINITE
        after = api.multi_fit(mh, p, X0.copy(order="F"), Y0.copy(order="F"))[0]
        assert np.array_equal(before, after)
        with pytest.raises(L.GLRMError) as ei:                # the plain multi entry point refuses the new codes as well
            api.multi_set_regularizers(mh, rx, ry)
        assert ei.value.code == UNSUPPORTED
        assert np.array_equal(before, api.multi_fit(mh, p, X0.copy(order="F"), Y0.copy(order="F"))[0])
    finally:
        api.multi_destroy(mh)


# ------------------------------------------------------------------------------------------------ 7. leaks

def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def cycle(rng, mdl, other):
    api = _capi.hip_api()
    g = RV.glrm_of(mdl, 5)
    L.fit_b(g, L.HipProxGradParams(max_iter=2), verbose=False)                 # create + install
    g.rx, g.ry = other[2], other[3]
    L.fit_b(g, L.HipProxGradParams(max_iter=2), verbose=False)                 # replace on the live handle
    h = g._handle_cache[1]
    tags = rng.integers(0, 2, len(g._colidx)).astype(np.uint8)
    ctags = rng.integers(0, 2, len(g._rowidx)).astype(np.uint8)
    api.destroy(api.subset(h, tags, ctags, 1, False))                          # a child with inherited tables
    pa = g.problem_arrays()
    api.set_regularizers(h, pa.rx, pa.ry)                                      # the plain call drops them
    g.close()


def test_no_device_memory_leak():
    rng = np.random.default_rng(0)
    mdl, other = RV.model("mixed_rows", 5, 1), RV.model("mixed_rows", 5, 2)
    cycle(rng, mdl, other)
    cycle(rng, mdl, other)
    levels = [free_bytes()]                                                    # windows as in tests/test_gpu_leaks.py
    for _ in range(3):
        for _ in range(8):
            cycle(rng, mdl, other)
        levels.append(free_bytes())
    lost = [levels[i] - levels[i + 1] for i in range(3)]
    assert min(lost) < 4 << 20, f"device memory lost per window of 8 cycles (MiB): {[round(x / 2**20, 1) for x in lost]}"
