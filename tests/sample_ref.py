"""A numpy restatement of include/glrm_hip_sample.h: Philox4x32-10 and the two uniforms of a (row, column), the Gaussian z, the rules
S1 .. S4 with wsample, the deterministic rules through ``domains.impute_entry``, and v_j.  u comes from ``precision_ref.xy_chain`` (the
bits of the device chain wherever the products are exact).

For every discrete draw the restatement also returns the MARGIN: the distance of U0 (for S3 and S4: of t / sum) to the nearest
cumulative boundary -- a draw whose margin exceeds the error of the exponentials cannot differ between this file and the device.
Deterministic and Gaussian entries carry margin +Inf."""
import math

import numpy as np

import lowrankmodels.jl_amd as L
from kmeanspp_ref import wsample

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TWO_PI = 6.283185307179586


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of 32-bit words, key: 2 -> 4 uint64 arrays holding 32-bit words."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & MASK for x in ctr]
    k = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & MASK for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]           # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return c


def words_to_uniforms(w):
    """U0 = (((w1 << 32) | w0) >> 11) * 2^-53, U1 likewise from w3, w2: exact conversions."""
    u0 = (((w[1] << np.uint64(32)) | w[0]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    u1 = (((w[3] << np.uint64(32)) | w[2]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return u0, u1


def uniforms(seed, rows, cols):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rows, cols = np.asarray(rows, dtype=np.uint64), np.asarray(cols, dtype=np.uint64)
    z = np.zeros_like(rows)
    return words_to_uniforms(philox4x32_10((rows, cols, z, z), (seed & 0xFFFFFFFF, seed >> 32)))


def gauss(U0, U1):
    """z of S1: plain multiplies, nothing contracted."""
    return np.sqrt(-2.0 * np.log(1.0 - U0)) * np.cos(TWO_PI * U1)


def rule(D, l):
    """"S1" .. "S4", "impute", or "refused" -- what Julia dispatch selects (src/sample.jl:159)."""
    if l.embedding_dim <= 1:
        if isinstance(D, L.RealDomain) and isinstance(l, L.QuadLoss):
            return "S1"
        if isinstance(D, L.BoolDomain) and isinstance(l, L.LogisticLoss):
            return "S2"
        return "impute"
    if isinstance(D, L.CategoricalDomain) and isinstance(l, L.MultinomialLoss):
        return "S3"
    if isinstance(D, (L.OrdinalDomain, L.CategoricalDomain)):
        return "S4"
    return "refused" if isinstance(D, L.BoolDomain) else "impute"


def level_weights(D, l, u):
    """(first level, weights) of S3 / S4."""
    if rule(D, l) == "S3":
        return 1, [math.exp(float(x)) for x in u]
    return D.min, [math.exp(-float(l.evaluate(np.array(u, dtype=float), lev))) for lev in range(D.min, D.max + 1)]


def draw_entry(D, l, u, U0, U1, sd=math.nan):
    """-> (value, margin) of one entry; u a float or the vector of embedding_dim(l) floats."""
    r = rule(D, l)
    if r == "S1":
        return float(u) + float(gauss(np.float64(U0), np.float64(U1))) * sd, math.inf
    if r == "S2":
        p = 1.0 / (1.0 + math.exp(-float(u)))
        return (1.0 if U0 <= p else 0.0), abs(U0 - p)
    if r in ("S3", "S4"):
        first, w = level_weights(D, l, u)
        i, margin = wsample(w, float(U0))
        return float(first + i), margin
    if r == "refused":
        raise TypeError(f"({D!r}, {l!r}) cannot be sampled")
    return float(L.impute_entry(D, l, u)), math.inf


def draws(domains, losses, U, rows, cols, seed, sd=None):
    """The draws at the pairs (rows[t], cols[t]); U = X'Y over the d vectors of Y; sd: n values (read at the S1 columns).
    -> (out, margin)."""
    spans = L.get_yidxs(losses)
    U0, U1 = uniforms(seed, rows, cols)
    out, margin = np.empty(len(rows)), np.empty(len(rows))
    for t, (i, j) in enumerate(zip(rows, cols)):
        y0, y1 = spans[j]
        u = U[i, y0:y1] if losses[j].embedding_dim > 1 else float(U[i, y0])
        out[t], margin[t] = draw_entry(domains[j], losses[j], u, float(U0[t]), float(U1[t]), math.nan if sd is None else float(sd[j]))
    return out, margin


def column_variance(U, colptr, rowidx, colvals, j, y0):
    """v_j = mean over the column-view list of column j of (u_ej - A_ej)^2 (NaN for an empty list); y0: the column's vector of Y."""
    b, e = int(colptr[j]), int(colptr[j + 1])
    if e == b:
        return math.nan
    res = U[np.asarray(rowidx[b:e], dtype=np.int64), y0] - np.asarray(colvals[b:e], dtype=np.float64)
    return float(np.sum(res * res)) / (e - b)


def noise_sd(v, noise):
    """sd_j of the rules "residual" (sqrt(v)) and "reference" (1 / sqrt(v))."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(v) if noise == "residual" else 1.0 / np.sqrt(v)
