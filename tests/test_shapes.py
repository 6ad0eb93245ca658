"""tests/shapes.py (the builder of the edge-case GPU tests) yields exactly the lengths and placements asked for, lists in range and in tile
order, and the same observations in both views."""
import numpy as np
import pytest

import shapes
from shapes import Seg


def check_views(pa):
    for ptr, idx, vals, size, other in ((pa.rowptr, pa.colidx, pa.rowvals, pa.m, pa.n), (pa.colptr, pa.rowidx, pa.colvals, pa.n, pa.m)):
        assert ptr[0] == 0 and np.all(np.diff(ptr) >= 0) and len(ptr) == size + 1 and ptr[-1] == len(idx) == len(vals)
        assert idx.dtype == np.int32 and (len(idx) == 0 or (idx.min() >= 0 and idx.max() < other))
        for s in range(size):
            assert np.all(np.diff(idx[ptr[s]:ptr[s + 1]]) >= 0)   # sorted: in tile order for every window size
    rows = np.repeat(np.arange(pa.m), np.diff(pa.rowptr))
    cols = np.repeat(np.arange(pa.n), np.diff(pa.colptr))
    a = sorted(zip(rows.tolist(), pa.colidx.tolist(), pa.rowvals.tolist()))
    b = sorted(zip(pa.rowidx.tolist(), cols.tolist(), pa.colvals.tolist()))
    assert a == b


@pytest.mark.parametrize("k", [8, 16, 32, 64, 128])
def test_lengths_and_placements_are_exactly_what_was_asked(k):
    kp, G = shapes.padded_rank(k)
    T = shapes.tile_rows(kp)
    assert T == {8: 1920, 16: 1056, 32: 560, 64: 288, 128: 144}[kp]
    m, n = 3 * T + 1, T + 20
    segs = [Seg("c0", "col", 0, 0), Seg("c1", "col", 5, 1), Seg("cG", "col", 6, G + 1), Seg("win", "col", 7, 40, "window", 1),
            Seg("last", "col", 8, 1, "last_tile"), Seg("edge", "col", 9, 6, "straddle", T), Seg("dup", "col", 10, 9, "dups"),
            Seg("rng", "col", 11, 30, "range", (T, 2 * T)), Seg("r0", "row", 3, 0), Seg("rlong", "row", 4, T + 1),
            Seg("redge", "row", 100, 4, "straddle", T), Seg("rdup", "row", 101, 6, "dups")]
    sh = shapes.build(m, n, k, segs, fill=3, losses="per_column", rx_per_row=True)
    check_views(sh.pa)
    for s in segs:
        got = sh.indices(s.view, s.index)
        assert len(got) == s.length, s
        assert np.array_equal(got, sh.lists[(s.view, s.index)])
    assert np.array_equal(sh.indices("col", sh.seg("win").index) // T, np.ones(40, int))
    assert list(sh.indices("col", 8)) == [m - 1] and (m - 1) // T == 3 and (m - 1) % T == 0   # the last tile holds one row
    assert sorted(set(sh.indices("col", 9).tolist())) == [T - 3, T - 2, T - 1, T, T + 1, T + 2]
    d = sh.indices("col", 10)
    assert np.all(d[0:8:2] == d[1:9:2]) and len(set(d.tolist())) == 5    # adjacent duplicates of one (i, j)
    assert np.all((sh.indices("col", 11) >= T) & (sh.indices("col", 11) < 2 * T))
    assert sorted(sh.indices("row", 100).tolist()) == [T - 2, T - 1, T, T + 1]
    assert len(sh.pa.losses) == n and len(set(sh.pa.losses["kind"].tolist())) == 6 and len(sh.pa.rx) == m
    listed_r = {s.index for s in segs if s.view == "row"}
    listed_c = {s.index for s in segs if s.view == "col"}
    for s in segs:   # a listed segment only meets unlisted ones
        assert not set(sh.indices(s.view, s.index).tolist()) & (listed_r if s.view == "col" else listed_c)
    assert sh.X0.shape == (k, m) and sh.Y0.shape == (k, n) and np.all(sh.X0 >= 0)   # rx per row includes NonNeg: a feasible start


def test_descriptor_counts_and_single_loss_models():
    sh = shapes.build(300, 300, 32, [], fill=5, losses="distinct", distinct=256)
    u = {tuple(r) for r in sh.pa.losses.tolist()}
    assert len(u) == 256
    sh = shapes.build(300, 300, 32, [], fill=5, losses="distinct", distinct=257)
    assert len({tuple(r) for r in sh.pa.losses.tolist()}) == 257
    for kind in shapes.EXACT_KINDS:
        sh = shapes.build(50, 40, 8, [Seg("a", "col", 2, 7)], fill=2, losses=kind, reg="nonneg")
        check_views(sh.pa)
        assert len(sh.pa.losses) == 1 and np.all(sh.Y0 >= 0)
    with pytest.raises(ValueError):
        shapes.build(50, 40, 8, [Seg("a", "col", 2, 60)], fill=2)     # more observations than rows to place them on
