"""Models, seeds and helpers shared by tests/test_regularizers_vec.py (CPU) and tests/test_gpu_regularizers_vec.py (-m gpu): the regularizers
that carry a vector, fixed_latent_features, fixed_last_latent_features and RemQuadReg (src/regularizers.jl:193-231,412-423;
include/glrm_hip_regvec.h).

The fits are held against numpy_proxgrad / numpy_gradstep (tests/test_oracle_vs_numpy.py, tests/regs_extra.py, imported unchanged) driven
by the mirror classes; the CPU oracle does not know these regularizers.  Shapes are those of tests/regs_extra.py (37 x 23, density 0.6,
12 iterations).  Seed discipline as there: for every entry of FITS numpy_proxgrad run in its two summation orders (plain and SeqArray)
agrees to 1e-9 on objectives, factors and step sizes -- the CPU test asserts it; a seed that forks is replaced here, never tolerated."""
import numpy as np

import lowrankmodels.jl_amd as L
from lowrankmodels.jl_amd.regularizers import pack_reg_vectors, pack_regs
from regs_extra import DENSITY, ITERS, M, N

MODEL_NAMES = ["fixfirst_ry", "fixlast_ry", "fixfirst_rx", "fixlast_rx", "remquad_both", "mixed_rows"]
#: the models whose random start does not satisfy a pin: the initial objective is inf, every later one finite
INF_START = {"fixfirst_ry", "fixlast_ry", "fixfirst_rx", "fixlast_rx", "mixed_rows"}


def nfix_of(k):
    return max(1, k // 3)


def model(name, k, seed, inner_iter=1):
    """Returns A, losses, rx, ry, feats, exs, X0, Y0, params (the tuple of tests/regs_extra.py: model)."""
    rng = np.random.default_rng(seed)
    kz = min(k, 4)
    Z = rng.standard_normal((M, kz)) @ rng.standard_normal((kz, N)) / np.sqrt(kz)
    A, losses = Z + 0.1 * rng.standard_normal((M, N)), [L.QuadLoss() for _ in range(N)]
    mask = rng.random((M, N)) < DENSITY
    feats = [list(np.flatnonzero(mask[i])) for i in range(M)]
    exs = [list(np.flatnonzero(mask[:, j])) for j in range(N)]
    X0, Y0 = rng.standard_normal((k, M)), rng.standard_normal((k, N))
    nf = nfix_of(k)
    PX, PY = rng.standard_normal((k, M)), rng.standard_normal((k, N))   # pins / means, one column per row / column of A
    quad_x, quad_y = [L.QuadReg(0.1)] * M, [L.QuadReg(0.1)] * N
    if name == "fixfirst_ry":
        rx, ry = quad_x, [L.fixed_latent_features(L.QuadReg(0.2), PY[:nf, j]) for j in range(N)]
    elif name == "fixlast_ry":
        rx, ry = quad_x, [L.fixed_last_latent_features(L.OneReg(0.2), PY[:nf, j]) for j in range(N)]
    elif name == "fixfirst_rx":
        rx, ry = [L.fixed_latent_features(L.KSparseConstraint(2), PX[:nf, i]) for i in range(M)], quad_y
    elif name == "fixlast_rx":
        rx, ry = [L.fixed_last_latent_features(L.NonNegConstraint(), PX[:nf, i]) for i in range(M)], quad_y
    elif name == "remquad_both":
        rx, ry = [L.RemQuadReg(0.7, PX[:, i]) for i in range(M)], [L.RemQuadReg(1.3, PY[:, j]) for j in range(N)]
    elif name == "mixed_rows":
        kinds = [lambda i: L.RemQuadReg(0.7, PX[:, i]), lambda i: L.fixed_latent_features(L.SimplexConstraint(), PX[:nf, i]),
                 lambda i: L.QuadReg(0.1), lambda i: L.fixed_last_latent_features(L.ZeroReg(), PX[:nf, i])]
        rx = [kinds[i % 4](i) for i in range(M)]
        ry = [L.fixed_latent_features(L.QuadReg(0.2), PY[:1, j]) for j in range(N)]
    else:
        raise KeyError(name)
    return A, losses, rx, ry, feats, exs, X0, Y0, L.ProxGradParams(max_iter=ITERS, inner_iter=inner_iter)


#: (model, k, inner_iter) -> seed.  Seeds start at 1; one that forked between the two summation orders is bumped by 100 (see module docstring).
FITS = {(name, k, 1): 1 for name in MODEL_NAMES for k in (5, 33)}
FITS[("fixfirst_rx", 5, 4)] = 1   # the one inner_iter = 4 case


def glrm_of(mdl, k, X=None, Y=None):
    A, losses, rx, ry, feats, exs, X0, Y0, p = mdl
    return L.GLRM(A, losses, rx, ry, k, observed_features=feats, observed_examples=exs, X=X0 if X is None else X, Y=Y0 if Y is None else Y)


def pinned_ok(rx, ry, X, Y):
    """After a fit every pinned entry equals its y exactly (first / last nfix entries of the row's / column's vector)."""
    for regs, F in ((rx, X), (ry, Y)):
        for i, r in enumerate(regs):
            if isinstance(r, L.fixed_latent_features) and not np.array_equal(F[:r.n, i], r.y):
                return False
            if isinstance(r, L.fixed_last_latent_features) and not np.array_equal(F[F.shape[0] - r.n:, i], r.y):
                return False
    return True


def vec_args(rx, ry, k):
    """(rx descriptors, vx, ry descriptors, vy) of Api.set_regularizers_vec for the regularizer lists of one handle (or one shard)."""
    vx, vy = pack_reg_vectors(rx, k), pack_reg_vectors(ry, k)
    return (vx[0] if vx is not None else pack_regs(rx), None if vx is None else vx[1:],
            vy[0] if vy is not None else pack_regs(ry), None if vy is None else vy[1:])


def create_with_vectors(api, g, **create_kw):
    """A handle for model g straight through _capi: created from the placeholder descriptors, then glrm_hip_set_regularizers_vec."""
    h = api.create(g.problem_arrays(), **create_kw)
    try:
        api.set_regularizers_vec(h, *vec_args(g.rx, g.ry, g.k))
    except Exception:
        api.destroy(h)
        raise
    return h


def run_capi(api, g, p, X0=None, Y0=None, **create_kw):
    """fit of model g through _capi alone; returns objective, X, Y, kernel stats."""
    h = create_with_vectors(api, g, **create_kw)
    try:
        X, Y = np.array(g.X if X0 is None else X0, order="F"), np.array(g.Y if Y0 is None else Y0, order="F")
        obj, _ = api.fit(h, p, X, Y)
        st = api.kernel_stats(h)
    finally:
        api.destroy(h)
    return obj, X, Y, st


# ------------------------------------------------------------------------------------------------ the reference's scripts
# test/fixedfeatures_test.jl (both halves) and test/mult_reg.jl, with numpy's generator in place of Julia's rand / randn.

def fixedfeatures_script(last, seed=1):
    """10 x 20, k + 1 = 4, SimplexConstraint rows, every column's first (or last) 3 latent features fixed to rand(3).  Returns the model
    tuple of `model` plus Yfix."""
    rng = np.random.default_rng(seed)
    m, n, k = 10, 20, 3
    Yfix, A = rng.random((k, n)), rng.random((m, n))
    make = L.FixedLastLatentFeaturesConstraint if last else L.FixedLatentFeaturesConstraint
    ry = [make(Yfix[:, j]) for j in range(n)]
    X0, Y0 = rng.standard_normal((k + 1, m)), rng.standard_normal((k + 1, n))
    feats, exs = [list(range(n))] * m, [list(range(m))] * n
    return (A, [L.QuadLoss() for _ in range(n)], [L.SimplexConstraint()] * m, ry, feats, exs, X0, Y0, L.ProxGradParams()), Yfix


def mult_reg_script(seed=1):
    """200 x 200, rank 5, RemQuadReg(50, .) on both sides, default params.  Returns the model tuple plus (U, V)."""
    rng = np.random.default_rng(seed)
    n = m = 200
    r, eta, delta = 5, 0.01, 1e-3
    Um, Vm = rng.standard_normal((r, n)), rng.standard_normal((r, m))
    U, V = Um + np.sqrt(eta) * rng.standard_normal((r, n)), Vm + np.sqrt(eta) * rng.standard_normal((r, m))
    Y = U.T @ V + np.sqrt(delta) * rng.standard_normal((n, m))
    X0, Y0 = rng.standard_normal((r, n)), rng.standard_normal((r, m))
    rx, ry = [L.RemQuadReg(50, Um[:, i]) for i in range(n)], [L.RemQuadReg(50, Vm[:, j]) for j in range(m)]
    feats, exs = [list(range(m))] * n, [list(range(n))] * m
    return (Y, [L.QuadLoss() for _ in range(m)], rx, ry, feats, exs, X0, Y0, L.ProxGradParams()), (U, V)
