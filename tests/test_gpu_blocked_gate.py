"""-m gpu: the phase gate of the phase-aligned passes (GLRM_HIP_BLOCKED_GATE, tiled_pass<..., L2 = true> in csrc/glrm_tiled.hpp) only
decides WHEN a lane group consumes its next batch of observations, never which accumulator a term goes to: factors, objectives and trial
counts are the same bits with the gate off, at its tightest (one row: every group but the trailing ones waits at almost every step) and at
the default, and the reported summation order does not change.  What these tests cannot show is that the gate has any effect (a gate the
compiler dropped would pass them all); that is what the C4 A/B runs and L2 counters under profiles/r07_* are for."""
import numpy as np
import pytest

import cases
import family_env
import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd import _capi, synth

pytestmark = pytest.mark.gpu
BLOCKED_ROWS, BLOCKED_COLS = 16, 32
GATES = (None, "0", "1", "37")  # None: the library's default


def force_blocked(monkeypatch, tps, fill):
    family_env.setenv(monkeypatch, family_env.blocked(tps, fill))


def run_under_gates(monkeypatch, pa, X0, Y0, params, **create_kw):
    api = _capi.hip_api()
    out = []
    for gate in GATES:
        if gate is None:
            monkeypatch.delenv("GLRM_HIP_BLOCKED_GATE", raising=False)
        else:
            monkeypatch.setenv("GLRM_HIP_BLOCKED_GATE", gate)
        obj, X, Y, st = cases.run_engine(api, pa, X0, Y0, params, **create_kw)
        assert st["tiled"] & (BLOCKED_ROWS | BLOCKED_COLS) == BLOCKED_ROWS | BLOCKED_COLS, (gate, st["tiled"])
        h = api.create(pa, **create_kw)
        try:
            order = [api.sum_order(h, v).asdict() for v in (0, 1)]
        finally:
            api.destroy(h)
        out.append((gate, np.asarray(obj), X, Y, st, order))
    return out


def assert_same_bits(runs):
    _, obj0, X0, Y0, st0, order0 = runs[0]
    for gate, obj, X, Y, st, order in runs[1:]:
        assert np.array_equal(obj, obj0), (gate, obj, obj0)
        assert np.array_equal(X, X0) and np.array_equal(Y, Y0), gate
        for key in ("trials_x", "trials_y", "accepts_x", "accepts_y"):
            assert st[key] == st0[key], (gate, key, st[key], st0[key])
        assert order == order0, (gate, order, order0)


def c4_recipe(m, n, q, k):
    rowptr, colidx, rowvals, colptr, rowidx, colvals, X0, Y0 = O.synth_cpu(m, n, k, q, value_model=1)
    one = np.array([(0, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    reg = np.array([(3, 0, 1.0)], dtype=_capi.REG_DTYPE)  # NonNegConstraint
    pa = _capi.ProblemArrays(m, n, k, rowptr, colidx, rowvals, colptr, rowidx, colvals, one, reg, reg)
    return pa, np.asfortranarray(np.abs(X0) / 8.0), np.asfortranarray(np.abs(Y0) / 8.0)


@pytest.mark.parametrize("k,tps,fill", [(64, "1", "3"), (64, "3", "100"), (32, "2", "7"), (16, "1", "50")])
def test_gate_changes_no_bit_on_the_c4_recipe(monkeypatch, k, tps, fill):
    """QuadLoss (the two-observation step) on the C4 recipe: several super-tiles and launch slices, eight-, four-lane and two-chunk layouts."""
    force_blocked(monkeypatch, tps, fill)
    pa, X0, Y0 = c4_recipe(12000, 1500, 100, k)
    assert_same_bits(run_under_gates(monkeypatch, pa, X0, Y0, L.ProxGradParams(max_iter=8), tiled=1))


@pytest.mark.parametrize("k", [32, 64])
def test_gate_changes_no_bit_with_a_loss_per_column(monkeypatch, k):
    """Quad / Logistic / OrdinalHinge columns: the whole batch of G observations per step (one loss evaluation per lane)."""
    force_blocked(monkeypatch, "1", "5")
    m, n, q = 2500, 2000, 100
    rowptr, colidx, rowvals, colptr, rowidx, colvals, X0, Y0 = O.synth_cpu(m, n, k, q, value_model=0, loss_mix=1)
    kinds = [L.QuadLoss().descriptor(), L.LogisticLoss().descriptor(), L.OrdinalHingeLoss(1, 5).descriptor()]
    losses = np.array([kinds[f % 3] for f in range(n)], dtype=_capi.LOSS_DTYPE)
    reg = np.array([(1, 0, 1.0)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, colidx, rowvals, colptr, rowidx, colvals, losses, reg, reg)
    runs = run_under_gates(monkeypatch, pa, np.asfortranarray(0.3 * X0), np.asfortranarray(0.3 * Y0), L.ProxGradParams(max_iter=6), tiled=1)
    assert_same_bits(runs)


def test_gate_changes_no_bit_on_a_power_law_omega(monkeypatch):
    """Zipf degrees: ragged lists of very different lengths inside one wave; the longest columns run on the gather sweep beside the passes."""
    force_blocked(monkeypatch, "2", "5")
    m, n, k = 30000, 3000, 32
    w = synth.ZipfWorkload(m, n, k, 3_000_000, s_rows=0.8, s_cols=0.8, seed=5, value_model=1, rx=(3, 0, 1.0), ry=(3, 0, 1.0), chunk=1 << 20)
    pa = w.host_problem()
    X0, Y0 = w.init_factors(k)
    X0, Y0 = X0.numpy().reshape(m, k).T, Y0.numpy().reshape(n, k).T
    X0, Y0 = np.asfortranarray(np.abs(X0) / k ** 0.5), np.asfortranarray(np.abs(Y0) / k ** 0.5)
    runs = run_under_gates(monkeypatch, pa, X0, Y0, L.ProxGradParams(max_iter=5, abs_tol=0.0, rel_tol=-1.0))
    assert_same_bits(runs)


def shuffle_inside_windows(ptr, idx, vals, rng, w=16):
    """The lists are only required to be in TILE order (check_sorted_kernel); every tile unit is a multiple of 16 rows, so permuting
    each segment's entries inside windows of w = 16 indices keeps the order the family admits while leaving the lists unsorted."""
    idx, vals = idx.copy(), vals.copy()
    for s in range(len(ptr) - 1):
        b, e = int(ptr[s]), int(ptr[s + 1])
        key = idx[b:e] // w
        perm = np.lexsort((rng.random(e - b), key))  # by window, random inside it
        idx[b:e], vals[b:e] = idx[b:e][perm], vals[b:e][perm]
    return idx, vals


@pytest.mark.parametrize("k", [32, 64])
def test_tightest_gate_ends_on_lists_unsorted_inside_a_tile(monkeypatch, k):
    """Lists in tile order but shuffled inside every 16-row window: a lane of a group may hold a smaller row than the group's next
    observation.  The trailing group is taken from each group's next row, so even the one-row gate ends its walk; bits as before."""
    force_blocked(monkeypatch, "1", "5")
    m, n, q = 4000, 400, 100
    rowptr, colidx, rowvals, colptr, rowidx, colvals, X0, Y0 = O.synth_cpu(m, n, k, q, value_model=1)
    rng = np.random.default_rng(11)
    colidx2, rowvals2 = shuffle_inside_windows(rowptr, colidx, rowvals, rng)
    rowidx2, colvals2 = shuffle_inside_windows(colptr, rowidx, colvals, rng)
    assert not np.array_equal(rowidx2, rowidx) and not np.array_equal(colidx2, colidx)
    one = np.array([(0, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    reg = np.array([(3, 0, 1.0)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, colidx2, rowvals2, colptr, rowidx2, colvals2, one, reg, reg)
    runs = run_under_gates(monkeypatch, pa, np.asfortranarray(np.abs(X0) / 8.0), np.asfortranarray(np.abs(Y0) / 8.0), L.ProxGradParams(max_iter=6), tiled=1)
    assert_same_bits(runs)
