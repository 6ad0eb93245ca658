"""Problems of explicit shape for the edge-case tests (tests/test_gpu_edge_shapes.py): chosen rows and columns get exactly the number of
observations asked for, placed where asked inside the tile windows of the opposing factor, and everything else gets filler.

A listed column takes its rows from the rows nobody listed, a listed row its columns from the columns nobody listed, and the filler
joins unlisted rows to unlisted columns only -- so every listed length is exact whatever else the problem holds.  Lists come out sorted
(ascending index, duplicates adjacent): in tile order for every window size.  Values and losses are restricted to the formulas the
engine and the oracle evaluate with the same instructions (no exp / log / sin)."""
from dataclasses import dataclass, field

import numpy as np

import lowrankmodels.jl_amd as L
from lowrankmodels.jl_amd import _capi

# the losses of test_gpu_fuzz.EXACT_KINDS, in the order a loss per column cycles through them
EXACT_KINDS = ("quad", "l1", "huber", "quantile", "ordhinge", "whinge")
REGS = {"quad": lambda: L.QuadReg(0.1), "nonneg": L.NonNegConstraint, "one": lambda: L.OneReg(0.05), "zero": L.ZeroReg}


def tile_rows(kp):
    """glrm_tile_rows (csrc/glrm_engine.hpp): vectors of the opposing factor per staged tile at padded rank kp."""
    return ((150 * 1024) // (kp * 8 + 16)) // 16 * 16


def padded_rank(k):
    """pick_layout (csrc/glrm_hip.hip): (kp, lanes of the gather layout)."""
    for kp, G in ((8, 4), (16, 4), (32, 4), (64, 8), (128, 16)):
        if k <= kp:
            return kp, G
    raise ValueError(k)


@dataclass
class Seg:
    """One listed segment.  view: "row" / "col"; place: "uniform" | "window" (inside tile window `arg`) | "last_tile" | "range" (indices
    [arg[0], arg[1])) | "straddle" (nearest the window edge at index `arg`: arg - 1, arg, arg - 2, arg + 1, ...) | "dups" (uniform,
    every index twice in a row); intent: the per-segment class the test expects the engine to run it on."""
    name: str
    view: str
    index: int
    length: int
    place: str = "uniform"
    arg: object = None
    intent: str = ""


@dataclass
class Shape:
    pa: object
    X0: np.ndarray
    Y0: np.ndarray
    segs: list
    T: int
    lists: dict = field(default_factory=dict)   # (view, index) -> sorted opposing indices

    def seg(self, name):
        return next(s for s in self.segs if s.name == name)

    def indices(self, view, i):
        ptr, idx = (self.pa.rowptr, self.pa.colidx) if view == "row" else (self.pa.colptr, self.pa.rowidx)
        return idx[ptr[i]:ptr[i + 1]]


def _pick(free, count):
    """`count` distinct entries of the sorted array `free`, spread evenly over it."""
    if count > len(free):
        raise ValueError(f"{count} observations asked for among {len(free)} free indices")
    return free[(np.arange(count, dtype=np.int64) * len(free)) // max(count, 1)] if count else free[:0]


def place(seg, free, size, T):
    """The opposing indices of a listed segment (sorted, duplicates adjacent)."""
    L_ = seg.length
    if seg.place == "uniform":
        return _pick(free, L_)
    if seg.place == "dups":
        base = _pick(free, (L_ + 1) // 2)
        return np.repeat(base, 2)[:L_]
    if seg.place in ("window", "last_tile", "range"):
        if seg.place == "range":
            lo, hi = seg.arg
        else:
            w = (size - 1) // T if seg.place == "last_tile" else int(seg.arg)
            lo, hi = w * T, min(size, (w + 1) * T)
        return _pick(free[(free >= lo) & (free < hi)], L_)
    if seg.place == "straddle":
        e = int(seg.arg)
        below, above = free[free < e][::-1], free[free >= e]
        out = []
        for a, b in zip(below, above):
            out += [a, b]
        if len(out) < L_:
            raise ValueError("not enough free indices around the edge")
        return np.sort(np.array(out[:L_], dtype=np.int64))
    raise ValueError(seg.place)


def column_loss(kind, f, distinct=None):
    s = 0.9 if distinct is None else 0.5 + (f % distinct) / distinct   # `distinct` different descriptors: the scale tells them apart
    return {"quad": lambda: L.QuadLoss(s), "l1": lambda: L.L1Loss(s), "huber": lambda: L.HuberLoss(s, crossover=0.7),
            "quantile": lambda: L.QuantileLoss(s, quantile=0.3), "ordhinge": lambda: L.OrdinalHingeLoss(1, 5, s),
            "whinge": lambda: L.WeightedHingeLoss(s, case_weight_ratio=1.5)}[kind]()


def value_of(kind, z):
    if kind == "ordhinge":
        return np.clip(np.round(3 + 1.5 * z), 1, 5)
    if kind == "whinge":
        return (z > 0).astype(np.float64)
    return z


def build(m, n, k, segs, fill=4, losses="quad", reg="quad", rx_per_row=False, seed=1, start=0.3, distinct=None):
    """losses: "quad" / one kind of EXACT_KINDS for the whole model (one descriptor), "per_column" (a descriptor per column, the kinds
    in turn), or "distinct" (QuadLoss with `distinct` different scales, column f taking scale number f mod distinct).  reg: a key of
    REGS for rx and ry; rx_per_row: rx cycles through every key of REGS by row.  fill: observations of every unlisted row (among the
    unlisted columns)."""
    kp, _ = padded_rank(k)
    T = tile_rows(kp)
    rng = np.random.default_rng(seed)
    listed_r = {s.index for s in segs if s.view == "row"}
    listed_c = {s.index for s in segs if s.view == "col"}
    assert len(listed_r) == sum(s.view == "row" for s in segs) and len(listed_c) == sum(s.view == "col" for s in segs), "a segment listed twice"
    free_r = np.array(sorted(set(range(m)) - listed_r), dtype=np.int64)
    free_c = np.array(sorted(set(range(n)) - listed_c), dtype=np.int64)
    I, J = [], []
    lists = {}
    for s in segs:
        if s.view == "col":
            rows = place(s, free_r, m, T)
            I.append(rows)
            J.append(np.full(len(rows), s.index, np.int64))
            lists[("col", s.index)] = rows
        else:
            cols = place(s, free_c, n, T)
            I.append(np.full(len(cols), s.index, np.int64))
            J.append(cols)
            lists[("row", s.index)] = cols
    if fill > 0 and len(free_c) and len(free_r):
        # q distinct columns per row: a random start, then strides of len(free_c) // q (ascending after the sort)
        q = min(fill, len(free_c))
        first = rng.integers(0, len(free_c), len(free_r))
        cols = np.sort(free_c[(first[:, None] + np.arange(q)[None, :] * (len(free_c) // q)) % len(free_c)], axis=1)
        I.append(np.repeat(free_r, q))
        J.append(cols.ravel())
    I = np.concatenate(I) if I else np.zeros(0, np.int64)
    J = np.concatenate(J) if J else np.zeros(0, np.int64)
    # values: one per observation, duplicates included (the two views carry the same (i, j, value) triples)
    if losses == "per_column":
        kinds = [EXACT_KINDS[f % len(EXACT_KINDS)] for f in range(n)]
        objs = [column_loss(kd, f) for f, kd in enumerate(kinds)]
    elif losses == "distinct":
        kinds = ["quad"] * n
        objs = [column_loss("quad", f, distinct) for f in range(n)]
    else:
        kinds = [losses] * n
        objs = [column_loss(losses, 0)]
    z = rng.standard_normal(len(I))
    vals = np.empty(len(I))
    kind_of = np.array([EXACT_KINDS.index(kd) for kd in kinds])[J] if len(I) else np.zeros(0, np.int64)
    for kd in set(kinds):
        sel = kind_of == EXACT_KINDS.index(kd)
        vals[sel] = value_of(kd, z[sel])
    # both views, stably sorted: equal (i, j) keep their order, so duplicates sit next to each other in both
    o_r = np.lexsort((J, I))
    o_c = np.lexsort((I, J))
    rowptr = np.zeros(m + 1, np.int64)
    np.add.at(rowptr, I + 1, 1)
    rowptr = np.cumsum(rowptr)
    colptr = np.zeros(n + 1, np.int64)
    np.add.at(colptr, J + 1, 1)
    colptr = np.cumsum(colptr)
    loss_arr = np.array([o.descriptor() for o in objs], dtype=_capi.LOSS_DTYPE)
    if rx_per_row:
        names = sorted(REGS)
        rx = np.array([REGS[names[i % len(names)]]().descriptor() for i in range(m)], dtype=_capi.REG_DTYPE)
    else:
        rx = np.array([REGS[reg]().descriptor()], dtype=_capi.REG_DTYPE)
    ry = np.array([REGS[reg]().descriptor()], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, np.ascontiguousarray(J[o_r], dtype=np.int32), np.ascontiguousarray(vals[o_r]), colptr,
                             np.ascontiguousarray(I[o_c], dtype=np.int32), np.ascontiguousarray(vals[o_c]), loss_arr, rx, ry)
    X0 = start * rng.standard_normal((k, m)) / k ** 0.25
    Y0 = start * rng.standard_normal((k, n)) / k ** 0.25
    if reg == "nonneg" or rx_per_row:
        X0 = np.abs(X0)
    if reg == "nonneg":
        Y0 = np.abs(Y0)
    return Shape(pa, np.asfortranarray(X0), np.asfortranarray(Y0), list(segs), T, lists)
