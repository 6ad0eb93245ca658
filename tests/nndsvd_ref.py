"""init_nndsvd! (reference: src/initialize_nmf.jl) in dense numpy, written from the contract in include/glrm_hip_nmf.h -- NMF.jl, whose
`nndsvd` the reference calls, is not part of its tree.  Everything m x n is explicit here: the matrix of a round is built entry by entry
and decomposed with np.linalg.svd.

    B_0[i, j] = s_j A[i, j] on the observed pairs, 0 elsewhere        (s_j = losses[j].scale with `scale`, else 1)
    (U, sigma, V) = the top-k singular triplets of B_t
    per component j, all alike:  xp = |max(u_j, 0)|, xn = |max(-u_j, 0)|, yp, yn from v_j, mp = xp yp, mn = xn yn
        mp >= mn:  c = sqrt(sigma_j mp),  W[:, j] = u_j c / xp where u_j > 0, else v0;  H[j, :] = v_j c / yp where v_j > 0, else v0
        else:      c = sqrt(sigma_j mn),  W[:, j] = -u_j c / xn where u_j < 0, else v0;  H[j, :] likewise with yn
    v0 = 0 (variant "std") or mean(B_t) over all m n entries (variant "a");  zeroh: H = 0 after the split
    X = W', Y = H;  round t >= 1:  B_t = s_j A on the observed pairs and (X'Y)[i, j] elsewhere, then SVD and split again

Also here: the fixtures of tests/test_gpu_nndsvd.py and the three conditions every fixture has to meet in every round, so that the CPU
suite and the GPU suite check the same matrices."""
import functools

import numpy as np


def split_factors(U, s, V, v0=0.0, zeroh=False):
    """(W, H, mp, mn) from singular triplets: U m x k, s k, V n x k."""
    m, k = U.shape
    n = V.shape[0]
    W, H = np.empty((m, k)), np.empty((k, n))
    mp, mn = np.zeros(k), np.zeros(k)
    for j in range(k):
        u, v = U[:, j], V[:, j]
        xp, xn = np.linalg.norm(np.maximum(u, 0.0)), np.linalg.norm(np.maximum(-u, 0.0))
        yp, yn = np.linalg.norm(np.maximum(v, 0.0)), np.linalg.norm(np.maximum(-v, 0.0))
        mp[j], mn[j] = xp * yp, xn * yn
        with np.errstate(divide="ignore", invalid="ignore"):     # a part without entries has norm 0 and no entry that divides by it
            if mp[j] >= mn[j]:
                c = np.sqrt(s[j] * mp[j])
                W[:, j] = np.where(u > 0, u * c / xp, v0)
                H[j] = np.where(v > 0, v * c / yp, v0)
            else:
                c = np.sqrt(s[j] * mn[j])
                W[:, j] = np.where(u < 0, -u * c / xn, v0)
                H[j] = np.where(v < 0, -v * c / yn, v0)
    if zeroh:
        H[...] = 0.0
    return W, H, mp, mn


def nndsvd(B, k, variant="std", zeroh=False):
    """(W, H, info) of a dense matrix; info: all singular values of B and (mp, mn) per component."""
    if variant not in ("std", "a"):
        raise NotImplementedError("variant ar draws NMF.jl's own random numbers")
    U, s, Vt = np.linalg.svd(B, full_matrices=False)
    v0 = float(B.mean()) if variant == "a" else 0.0
    W, H, mp, mn = split_factors(U[:, :k], s[:k], Vt[:k].T, v0, zeroh)
    return W, H, dict(sigma=s, mp=mp, mn=mn, v0=v0)


def init_nndsvd(A, mask, scales, k, scale=True, zeroh=False, variant="std", max_iters=0):
    """A m x n, mask m x n bool (the observed pairs), scales n.  Returns X (k x m), Y (k x n), the singular values and the (larger,
    smaller) split products of the last round, and every round's info."""
    sA = A * (np.asarray(scales, dtype=np.float64)[None, :] if scale else 1.0)
    B = np.where(mask, sA, 0.0)
    rounds = []
    for t in range(max_iters + 1):
        if t > 0:
            B = np.where(mask, sA, W @ H)
        W, H, info = nndsvd(B, k, variant, zeroh)
        rounds.append(info)
    last = rounds[-1]
    spl = np.column_stack([np.maximum(last["mp"], last["mn"]), np.minimum(last["mp"], last["mn"])])
    return dict(X=np.asfortranarray(W.T), Y=np.asfortranarray(H), singular_values=last["sigma"][:k].copy(), split=spl, rounds=rounds)


# ---- the fixtures: A = 4 + sqrt(m n) Q_m diag(decay^i) Q_n', rank r, under a Bernoulli mask; k = r + 1
#            m     n    k  r  density seed decay
FIXTURES = ((300, 200, 4, 3, 0.95, 1, 0.5),
            (97, 130, 3, 2, 0.9, 2, 0.5),
            (2000, 48, 3, 2, 0.9, 3, 0.5),
            (64, 1500, 4, 3, 1.0, 4, 0.5),
            (513, 257, 5, 4, 0.97, 5, 0.6))
ROUNDS = (0, 1, 2)
MIN_GAP, MAX_TAIL, MIN_MARGIN = 0.03, 0.45, 5e-3


@functools.lru_cache(maxsize=None)
def fixture(m, n, k, r, density, seed, decay):
    """(A, mask): computed once and shared; callers do not write to them."""
    rng = np.random.default_rng(seed)
    Qm = np.linalg.qr(rng.standard_normal((m, r)))[0]
    Qn = np.linalg.qr(rng.standard_normal((n, r)))[0]
    A = 4.0 + np.sqrt(m * n) * (Qm * decay ** np.arange(r)) @ Qn.T
    mask = rng.random((m, n)) < density
    A.setflags(write=False)
    mask.setflags(write=False)
    return A, mask


@functools.lru_cache(maxsize=None)
def fixture_reference(fx, max_iters, variant="std", zeroh=False):
    A, mask = fixture(*fx)
    return init_nndsvd(A, mask, np.ones(fx[1]), fx[2], scale=False, zeroh=zeroh, variant=variant, max_iters=max_iters)


# ---- further problems of the GPU suite, (A, mask, k, scales); the CPU suite asserts the conditions for them as well
def scaled_case():
    """Fixture 0 with a loss scale per column."""
    fx = FIXTURES[0]
    A, mask = fixture(*fx)
    return A, mask, fx[2], 0.8 + 0.4 * np.random.default_rng(11).random(fx[1])


def empty_case():
    """Fixture 4 with a row and a column without observations."""
    fx = FIXTURES[4]
    A, mask = fixture(*fx)
    mask = mask.copy()
    mask[5, :] = False
    mask[:, 7] = False
    return A, mask, fx[2], np.ones(fx[1])


def long_case():
    """40000 x 12, fully observed: every column list spans three 16384-entry chunks."""
    A, mask = fixture(40000, 12, 3, 2, 1.0, 6, 0.5)
    return A, mask, 3, np.ones(12)


def conditions(info, k, l):
    """(smallest gap among the first k + 1 singular values / sigma_1, sigma_l / sigma_k, smallest |mp - mn| / max(mp, mn))."""
    s = info["sigma"]
    gap = float(np.min(s[:k] - s[1:k + 1]) / s[0])
    tail = float(s[l - 1] / s[k - 1])
    margin = float(np.min(np.abs(info["mp"] - info["mn"]) / np.maximum(info["mp"], info["mn"])))
    return gap, tail, margin


def check_conditions(ref, k, l):
    """Asserts the three conditions for every round of a reference run; returns the figures."""
    out = []
    for t, info in enumerate(ref["rounds"]):
        gap, tail, margin = conditions(info, k, l)
        out.append((gap, tail, margin))
        assert gap >= MIN_GAP, f"round {t}: smallest gap {gap:.4f} sigma_1"
        assert tail <= MAX_TAIL, f"round {t}: sigma_l / sigma_k = {tail:.4f}"
        assert margin >= MIN_MARGIN, f"round {t}: split margin {margin:.2e}"
    return out
