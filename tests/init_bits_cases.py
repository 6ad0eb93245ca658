"""The cases of tests/golden/init_bits.npz: glrm_hip_init_svd (S*) and glrm_hip_init_nndsvd (N*) at shapes where the column product,
its chunk reduce and the subspace iteration take every path (a block clipped to d, a ragged last workgroup, empty segments, d > 1
expansion, l > 64, three chunks with a short last one).  Inputs are seeded standard normal draws, so a reordered sum changes bits; every
case runs exactly FIXED_ITERS subspace iterations (a tolerance no run reaches).  Shared by tests/golden/make_init_bits.py, which records,
and tests/test_gpu_init_bits.py, which compares.

S1's mask has column 7 empty, so a row holds at most 8 entries: the row lengths cover 0 ... 8, every length the mask allows."""
import functools
import hashlib

import numpy as np

import lowrankmodels.jl_amd as L
from test_init_svd import model_of

FIXED_ITERS = 5
NEVER = 1e-300                # a relative change of the singular values no iteration reaches
FULL_BYTES = 64 << 10         # a case whose arrays are smaller together is stored in full, otherwise as SHA-256 (singular values in full)
LONG_M = 2 * 16384 + 5        # three chunks of the column product, the last of 5 entries

CASES = ("S1", "S2_categorical_mix", "S2_ordinal_offsets", "S2_mnl", "S3", "S4", "N1", "N2", "N3", "N4")


@functools.lru_cache(maxsize=None)
def s1_mask():
    """130 x 9, about 60 % observed, row 5 and column 7 empty, rows 10 ... 18 with 0 ... 8 entries."""
    rng = np.random.default_rng(101)
    mask = rng.random((130, 9)) < 0.68  # 0.6 of the whole once the empty row and column are out
    open_cols = [c for c in range(9) if c != 7]
    for length in range(9):
        mask[10 + length] = False
        mask[10 + length, open_cols[:length]] = True
    mask[5] = False
    mask[:, 7] = False
    mask.setflags(write=False)
    return mask


def _quad(A, k, mask=None, scales=None):
    losses = L.QuadLoss() if scales is None else [L.QuadLoss(float(s)) for s in scales]
    obs = {} if mask is None else dict(obs=np.nonzero(mask))
    return L.GLRM(A, losses, L.ZeroReg(), L.ZeroReg(), k, **obs)


def build(name):
    """-> (model, "svd" | "nndsvd", keyword arguments of the initialization)."""
    svd = dict(max_iter=FIXED_ITERS, tol=NEVER)
    nmf = dict(svd_max_iter=FIXED_ITERS, svd_tol=NEVER)
    if name == "S1":
        return _quad(np.random.default_rng(102).standard_normal((130, 9)), 3, s1_mask()), "svd", svd
    if name.startswith("S2_"):
        return model_of(name[3:]), "svd", svd
    if name == "S3":
        return _quad(np.random.default_rng(103).standard_normal((140, 80)), 60), "svd", svd
    if name == "S4":
        rng = np.random.default_rng(104)
        A = rng.standard_normal((LONG_M, 3))
        A[:, 0] = rng.integers(1, 4, LONG_M)
        return L.GLRM(A, [L.MultinomialLoss(3), L.QuadLoss(), L.QuadLoss()], L.ZeroReg(), L.ZeroReg(), 2), "svd", svd
    if name == "N1":
        scales = 0.8 + 0.4 * np.random.default_rng(106).random(9)
        return (_quad(np.random.default_rng(105).standard_normal((130, 9)), 3, s1_mask(), scales), "nndsvd",
                dict(nmf, scale=True, variant="std", max_iters=2))
    if name == "N2":
        return _quad(np.random.default_rng(107).standard_normal((130, 9)), 4, s1_mask()), "nndsvd", dict(nmf, variant="a", max_iters=1)
    if name == "N3":
        return _quad(np.random.default_rng(108).standard_normal((140, 80)), 60), "nndsvd", dict(nmf, max_iters=1)
    if name == "N4":
        return _quad(np.random.default_rng(109).standard_normal((LONG_M, 3)), 2), "nndsvd", dict(nmf, max_iters=1)
    raise KeyError(name)


def run_twice(name, api):
    """Two calls on one model (the second on the handle the first left behind) -> two dicts of arrays."""
    g, kind, kw = build(name)
    outs = []
    try:
        for _ in range(2):
            if kind == "svd":
                L.init_svd_(g, engine=api, **kw)
                info = g._init_svd_info
                out = dict(iters=np.array([info["iterations"]], dtype=np.int32))
            else:
                L.init_nndsvd_(g, engine=api, **kw)
                info = g._init_nndsvd_info
                out = dict(iters=np.array(info["iterations"], dtype=np.int32), split=np.array(info["split"]))
            out.update(X=np.array(g.X), Y=np.array(g.Y), sv=np.array(info["singular_values"]))
            outs.append(out)
    finally:
        g.close()
    return outs


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def record(out):
    """What the fixture keeps of one call's arrays."""
    if sum(a.nbytes for a in out.values()) < FULL_BYTES:
        return dict(out)
    return {key: a if key in ("sv", "iters") else np.array(hashlib.sha256(raw(a)).hexdigest()) for key, a in out.items()}
