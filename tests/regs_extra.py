"""Models, seeds and numpy restatements shared by tests/test_regularizers_extra.py (CPU) and tests/test_gpu_regularizers_extra.py (-m gpu):
the vector regularizers QuadConstraint, NonNegOneReg, OneSparseConstraint, KSparseConstraint and SimplexConstraint
(src/regularizers.jl:68-76,118-138,235-291,323-348).

The GPU fits are held against numpy_proxgrad (tests/test_oracle_vs_numpy.py, imported unchanged).  Three of the five prox operators select
entries, so a trajectory can fork where two candidates are within rounding of each other: every (model, k) below uses a seed for which
numpy_proxgrad run in two summation orders -- as written (dense BLAS products) and with every product accumulated one term per step in
component order (SeqArray) -- agrees to 1e-9 on objectives, factors and step sizes.  The CPU test asserts that for each entry of FITS;
a seed that forked was replaced here, never tolerated."""
import numpy as np

import lowrankmodels.jl_amd as L

M, N, DENSITY, ITERS = 37, 23, 0.6, 12
NEW_KINDS = {
    "quadconstraint": lambda: L.QuadConstraint(1.5),
    "nonnegone": lambda: L.NonNegOneReg(0.3),
    "onesparse": lambda: L.OneSparseConstraint(),
    "ksparse": lambda: L.KSparseConstraint(2),
    "simplex": lambda: L.SimplexConstraint(),
}


def hello_world_rx(m):
    """The per-row list of test/hello_world.jl:30, cycled over the rows."""
    kinds = [L.QuadReg(), L.OneReg(5), L.NonNegConstraint(), L.KSparseConstraint(2)]
    return [kinds[i % 4] for i in range(m)]


def _mixed_columns(rng, Z):
    """Losses and data per column as in mixed_losses_per_row_regs (tests/test_oracle_vs_numpy.py)."""
    m, n = Z.shape
    A, losses = np.zeros((m, n)), []
    for f in range(n):
        kind = f % 5
        if kind == 0:
            A[:, f] = Z[:, f]; losses.append(L.QuadLoss(0.8))
        elif kind == 1:
            A[:, f] = rng.random(m) < 0.5; losses.append(L.LogisticLoss(1.2))
        elif kind == 2:
            A[:, f] = np.clip(np.round(3 + Z[:, f]), 1, 5); losses.append(L.OrdinalHingeLoss(1, 5))
        elif kind == 3:
            A[:, f] = Z[:, f]; losses.append(L.HuberLoss(1.0, crossover=0.7))
        else:
            A[:, f] = rng.random(m) < 0.4; losses.append(L.WeightedHingeLoss(1.0, case_weight_ratio=1.5))
    return A, losses


def model(name, k, seed, inner_iter=1):
    """name: '<kind>_rx', '<kind>_ry', 'hello_world', 'mixed', 'offset'.  Returns A, losses, rx, ry, feats, exs, X0, Y0, params."""
    rng = np.random.default_rng(seed)
    kz = min(k, 4)
    Z = rng.standard_normal((M, kz)) @ rng.standard_normal((kz, N)) / np.sqrt(kz)
    if name == "mixed":
        A, losses = _mixed_columns(rng, Z)
        rx, ry = hello_world_rx(M), [L.SimplexConstraint() if f % 3 == 0 else L.QuadReg(0.2) for f in range(N)]
    else:
        A, losses = Z + 0.1 * rng.standard_normal((M, N)), [L.QuadLoss() for _ in range(N)]
        if name == "hello_world":
            rx, ry = hello_world_rx(M), [L.QuadReg(0.1)] * N
        elif name == "offset":   # add_offset! with a simplex on the first k - 1 entries of every row (general sweeps)
            rx, ry = [L.lastentry1(L.SimplexConstraint())] * M, [L.lastentry_unpenalized(L.QuadReg(0.1))] * N
        else:
            kind, side = name.rsplit("_", 1)
            r = NEW_KINDS[kind]()
            rx, ry = ([r] * M, [L.QuadReg(0.1)] * N) if side == "rx" else ([L.QuadReg(0.1)] * M, [r] * N)
    mask = rng.random((M, N)) < DENSITY
    feats = [list(np.flatnonzero(mask[i])) for i in range(M)]
    exs = [list(np.flatnonzero(mask[:, j])) for j in range(N)]
    X0, Y0 = rng.standard_normal((k, M)), rng.standard_normal((k, N))
    return A, losses, rx, ry, feats, exs, X0, Y0, L.ProxGradParams(max_iter=ITERS, inner_iter=inner_iter)


MODEL_NAMES = [f"{kind}_{side}" for kind in NEW_KINDS for side in ("rx", "ry")] + ["hello_world", "mixed"]
#: (model, k, inner_iter) -> seed.  Seeds start at 1; one that forked between the two summation orders is bumped by 100 (see module docstring).
FITS = {(name, k, 1): 1 for name in MODEL_NAMES for k in (5, 33)}
FITS[("ksparse_rx", 5, 4)] = 1   # the one inner_iter = 4 case
FITS[("simplex_ry", 32, 1)] = 1  # padded rank 32: the lane-per-segment family (layout (2, 16)) and the cached sweeps at (4, 8)
FITS[("mixed", 32, 1)] = 1
FITS[("offset", 4, 1)] = 1       # lastentry1(SimplexConstraint()) / lastentry_unpenalized(QuadReg): the general sweeps


def glrm_of(mdl, k):
    A, losses, rx, ry, feats, exs, X0, Y0, p = mdl
    return L.GLRM(A, losses, rx, ry, k, observed_features=feats, observed_examples=exs, X=X0, Y=Y0)


class SeqArray(np.ndarray):
    """ndarray whose matrix products add one term per step in component order (multiply, then add): what a sequential dot product over
    the k components gives for every entry, observed ones included -- the second summation order of the seed check."""

    @staticmethod
    def _mm(a, b):
        a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
        a2, b2 = np.atleast_2d(a), (b[:, None] if b.ndim == 1 else b)
        acc = np.zeros((a2.shape[0], b2.shape[1]))
        for c in range(a2.shape[1]):
            acc = acc + np.outer(a2[:, c], b2[c, :])
        if a.ndim == 1:
            acc = acc[0]
        if b.ndim == 1:
            acc = acc[..., 0]
        return acc

    def __matmul__(self, other):
        return SeqArray._mm(self, other)

    def __rmatmul__(self, other):
        return SeqArray._mm(other, self)


def numpy_gradstep(A, losses, rx, ry, feats, exs, X, Y, alpha):
    """One global-step-size prox-gradient step of the rows, then of the columns (src/algorithms/sparse_proxgrad.jl:59-77 / :81-99)."""
    X, Y = X.copy(), Y.copy()
    for e in range(X.shape[1]):
        g = np.zeros(X.shape[0])
        for f in feats[e]:
            g += losses[f].grad(float(X[:, e] @ Y[:, f]), A[e, f]) * Y[:, f]
        l = len(feats[e]) + 1
        X[:, e] = rx[e].prox(X[:, e] + g * (-alpha / l), alpha / l)
    for f in range(Y.shape[1]):
        g = np.zeros(Y.shape[0])
        for e in exs[f]:
            g += losses[f].grad(float(X[:, e] @ Y[:, f]), A[e, f]) * X[:, e]
        l = len(exs[f]) + 1
        Y[:, f] = ry[f].prox(Y[:, f] + g * (-alpha / l), alpha / l)
    return X, Y
