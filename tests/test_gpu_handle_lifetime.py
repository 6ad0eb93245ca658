"""-m gpu: a long-lived handle is held to the bits of a fresh one, on every kernel family (the twelve of test_gpu_devmem.FAMILIES).

The hosts keep one handle alive across many calls (the model's cached handle, warm starts, the extensions' NULL-factor form); the rest of
the suite creates a handle, makes one call and destroys it.  Here every call sequence runs twice: on ONE handle, and call by call on
handles created for the call; X, Y, the recorded objective, the per-column objective and the trial / accept / launch counts must be equal
BIT FOR BIT (tests/handle_lifetime.py: same_bits) -- no tolerance is chosen anywhere.  The fresh-handle run is itself held to the CPU
oracle as the family's own tests hold it (handle_lifetime.ORACLE), so the long-lived handle answers to an independent reference.

A  glrm_hip_fit reused: fit(p1), fit(p1), fit(p2), fit(p1) and a warm-start chain; with GLRM_HIP_GRAPH unset and "0" where an iteration
   is captured as a graph; a fit after fit_sparse and after a step-level stretch.
B  calls that promise not to disturb a stepping sequence, between two stretches of half-steps with the four device buffers bound; calls
   that upload factors or write an objective vector, with their documented effect pinned; two self-checks that the comparison sees a
   disturbed step size and a factor moved by one ulp.
C  solve_x and a regularizer round trip leave only their documented change.
D  the host layer's cached handle through fit_b, impute_at, recommend, sample_at, transform, precision_at_k, fit_b.
E  sharded handles.

The step sizes have no getter: a call that disturbed them shows only in a later line search.  The reference runs therefore assert
(handle_lifetime.sensitive) that the stretch after the probes rejects and accepts on both views and counts differently from the same
stretch started from reset step sizes.  The dense family's step reports its trial / accept counts like the others, so no family is exempt
from the counts of section A; the dense and the float-storage family are outside section B, whose calls serve fp64 list handles.

Checked when the module was written: a build whose captured iteration kept a stale min_stepsize fails
test_each_captured_parameter_alone_rebuilds_the_iteration[graph], and one whose kernel_stats(reset=0) zeroed the device counters fails
every case of the probe tests."""
import numpy as np
import pytest

import cases
import handle_lifetime as H
import lowrankmodels.jl_amd as L
import oracle as O
import test_gpu_devmem as D
from lowrankmodels.jl_amd import _capi

pytestmark = pytest.mark.gpu


def hip():
    return _capi.hip_api()


_REFS = {}


def refs(family, graph=None, regs=None):
    """R1, R2 and the three links of the warm-start chain on fresh handles, each held to the oracle; computed once per (family, graph
    setting).  The caller has set the family's environment."""
    key = (family, graph, regs is not None)
    if key not in _REFS:
        api, sh = hip(), H.shape_of(family)
        orders = H.orders_of(api, family)
        out = {"R1": H.fresh_fit(api, family, H.p1(family), sh.X0, sh.Y0, regs), "R2": H.fresh_fit(api, family, H.p2(family), sh.X0, sh.Y0, regs)}
        chain, X, Y = [], sh.X0, sh.Y0
        for _ in range(3):
            chain.append(((X, Y), H.fresh_fit(api, family, H.link(family), X, Y, regs)))
            X, Y = chain[-1][1].X, chain[-1][1].Y
        out["chain"] = chain
        if regs is None:   # (the oracle does not have the vector-carrying regularizers: test_gpu_regularizers_vec.py holds them)
            H.hold_fit_to_oracle(family, out["R1"], H.p1(family), sh.X0, sh.Y0, orders)
            H.hold_fit_to_oracle(family, out["R2"], H.p2(family), sh.X0, sh.Y0, orders)
            for (X, Y), got in chain:
                H.hold_fit_to_oracle(family, got, H.link(family), X, Y, orders)
        _REFS[key] = out
    return _REFS[key]


def gather_vector_regs():
    """fixed_latent_features on every row of the gather shape: the vector-regularizer instantiation of the gather sweeps."""
    import regs_vec
    sh = H.shape_of("gather, several wave classes")
    rx = [L.fixed_latent_features(L.QuadReg(0.1), np.full(2, 0.25)) for _ in range(sh.pa.m)]
    return regs_vec.vec_args(rx, [L.QuadReg(0.1)], sh.pa.k)


# ================================================================================================ A. the whole-fit entry point, reused

def reused_fits(family, regs=None):
    """On ONE handle: fit(p1), fit(p1), fit(p2), fit(p1) from copies of the same start, then the warm-start chain."""
    api, sh = hip(), H.shape_of(family)
    h = H.create(api, family, regs)
    try:
        four = [H.fit_on(api, h, p, sh.X0, sh.Y0) for p in (H.p1(family), H.p1(family), H.p2(family), H.p1(family))]
        chain, X, Y = [], sh.X0, sh.Y0
        for _ in range(3):
            chain.append(H.fit_on(api, h, H.link(family), X, Y))
            X, Y = chain[-1].X, chain[-1].Y
        for _ in range(2):   # without a reset between them, the counters add up
            api.fit(h, H.p1(family), sh.X0.copy(order="F"), sh.Y0.copy(order="F"))
        totals = H.counters(api.kernel_stats(h))
    finally:
        api.destroy(h)
    return four, chain, totals


def check_reused(family, graph, regs=None):
    r = refs(family, graph, regs)
    four, chain, totals = reused_fits(family, regs)
    assert totals == {k: 2 * v for k, v in r["R1"].counts.items()}, (family, graph, "two fits without a counter reset", totals, r["R1"].counts)
    for i, (got, want) in enumerate(zip(four, (r["R1"], r["R1"], r["R2"], r["R1"]))):
        assert got.differs_from(want) is None, (family, graph, f"fit number {i + 1} on the handle", got.differs_from(want))
    for i, (got, (_, want)) in enumerate(zip(chain, r["chain"])):
        assert got.differs_from(want) is None, (family, graph, f"link {i + 1} of the warm-start chain", got.differs_from(want))
    return four, chain


@pytest.mark.parametrize("family", list(H.FAMILIES))
def test_a_reused_handle_fits_like_fresh_ones(monkeypatch, family):
    graphs = (None, "0") if family in H.GRAPH_FAMILIES else (None,)
    runs = {}
    for graph in graphs:
        H.set_family(monkeypatch, family, graph)
        runs[graph] = check_reused(family, graph)
    if len(graphs) == 2:   # the captured iteration and the plain launches: the same bits and the same launch counts
        for a, b in zip(runs[None][0] + runs[None][1], runs["0"][0] + runs["0"][1]):
            assert a.differs_from(b) is None, (family, "GLRM_HIP_GRAPH unset against 0", a.differs_from(b))
    c = refs(family, graphs[0])["R1"].counts
    # every family's fit rejects and accepts on both views (the dense step reports its counts as well: no family is exempt)
    assert c["trials_x"] > c["accepts_x"] > 0 and c["trials_y"] > c["accepts_y"] > 0, (family, c)


def test_a_reused_handle_with_vector_regularizers_fits_like_fresh_ones(monkeypatch):
    """set_regularizers_vec on the gather shape: the other instantiation of the gather sweeps, captured and replayed as well."""
    family, regs = "gather, several wave classes", gather_vector_regs()
    runs = {}
    for graph in (None, "0"):
        H.set_family(monkeypatch, family, graph)
        runs[graph] = check_reused(family, graph, regs)
        assert np.array_equal(runs[graph][0][0].X[:2], np.full((2, H.shape_of(family).pa.m), 0.25))   # the vectors pin the rows
    for a, b in zip(runs[None][0] + runs[None][1], runs["0"][0] + runs["0"][1]):
        assert a.differs_from(b) is None, ("GLRM_HIP_GRAPH unset against 0", a.differs_from(b))


@pytest.mark.parametrize("graph", [None, "0"], ids=["graph", "plain launches"])
def test_each_captured_parameter_alone_rebuilds_the_iteration(monkeypatch, graph):
    """The captured iteration holds inner_iter_X, inner_iter_Y, min_stepsize and -- with inner iterations, where the step-size reset is
    part of it -- stepsize by value.  Fits that differ from the one before in ONE of them, on one handle: each is the fresh handle's."""
    family = "gather, several wave classes"
    H.set_family(monkeypatch, family, graph)
    api, sh = hip(), H.shape_of(family)
    s, mn = H.FITTING[family]

    def prm(stepsize=0.5 * s, ix=2, iy=2, min_stepsize=2.0 * mn):
        return L.ProxGradParams(stepsize, max_iter=3, inner_iter_X=ix, inner_iter_Y=iy, abs_tol=-1e300, rel_tol=-1e300, min_stepsize=min_stepsize)
    variants = [{}, {"stepsize": 0.25 * s}, {}, {"min_stepsize": 30.0 * mn}, {}, {"ix": 3}, {}, {"iy": 1}, {}]
    h = H.create(api, family)
    try:
        got = [H.fit_on(api, h, prm(**kw), sh.X0, sh.Y0) for kw in variants]
    finally:
        api.destroy(h)
    fresh = {}
    for kw, g in zip(variants, got):
        key = tuple(sorted(kw.items()))
        if key not in fresh:
            fresh[key] = H.fresh_fit(api, family, prm(**kw), sh.X0, sh.Y0)
        assert g.differs_from(fresh[key]) is None, (graph, kw, g.differs_from(fresh[key]))
    base = fresh[()]
    for key, f in fresh.items():   # every variant is a different fit: a stale capture would have shown
        assert key == () or f.differs_from(base) is not None, key


@pytest.mark.parametrize("family", list(H.FAMILIES))
def test_a_fit_after_other_work_on_the_handle_is_the_fresh_fit(monkeypatch, family):
    """fit(p1), fit_sparse, fit(p1), a step-level stretch, fit(p1): every fit(p1) is R1.  fit_sparse is refused on a float-storage
    handle (include/glrm_hip_storage.h) and on a reference-order one (it restates the ProxGradParams half-steps only); there the
    refusal is checked in its place, and the fit after it is still R1."""
    for graph in ((None, "0") if family in H.GRAPH_FAMILIES else (None,)):
        H.set_family(monkeypatch, family, graph)
        fit_among_other_work(family, refs(family, graph)["R1"])


def fit_among_other_work(family, R1):
    api, sh = hip(), H.shape_of(family)
    s0, mn = H.STEPPING[family]
    h = H.create(api, family)
    try:
        got = H.fit_on(api, h, H.p1(family), sh.X0, sh.Y0)
        assert got.differs_from(R1) is None, (family, "first fit", got.differs_from(R1))
        sp = L.SparseProxGradParams(0.01, max_iter=3)
        if family in ("storage = f32", "sum_order = 1"):
            with pytest.raises(_capi.GLRMError) as e:
                api.fit_sparse(h, sp, sh.X0.copy(order="F"), sh.Y0.copy(order="F"))
            assert e.value.code == _capi.ERR_UNSUPPORTED
        else:
            api.fit_sparse(h, sp, sh.X0.copy(order="F"), sh.Y0.copy(order="F"))
        got = H.fit_on(api, h, H.p1(family), sh.X0, sh.Y0)
        assert got.differs_from(R1) is None, (family, "the fit after fit_sparse", got.differs_from(R1))
        api.objective(h, sh.X0, sh.Y0)              # (the fixed-order sum shares its partials with the captured iteration's)
        api.set_factors(h, sh.X0, sh.Y0)
        api.reset_stepsizes(h, s0)
        api.kernel_stats(h, reset=True)
        for _ in range(2):
            api.step_x(h, mn)
            api.step_y(h, mn)
        if family in H.LIST_F64:   # the stretch itself, after two fits on the handle: the first stretch of the fresh handle's script
            X, Y = np.zeros_like(sh.X0), np.zeros_like(sh.Y0)
            api.get_factors(h, X, Y)
            want, st = reference_script(family)[0], H.counters(api.kernel_stats(h))
            assert H.same_bits(X, want.X) and H.same_bits(Y, want.Y) and st == want.counts, (family, "the stretch after two fits", st, want.counts)
        api.reset_stepsizes(h, 0.37 * s0)               # what the stretch leaves behind is not the fit's start
        got = H.fit_on(api, h, H.p1(family), sh.X0, sh.Y0)
        assert got.differs_from(R1) is None, (family, "the fit after a step-level stretch", got.differs_from(R1))
    finally:
        api.destroy(h)


# ================================================================================================ B. calls that leave a stepping sequence alone

_SCRIPTS = {}


def reference_script(family):
    """The script without probes on a fresh handle, held to the oracle's and checked to be sensitive; once per family."""
    if family not in _SCRIPTS:
        api = hip()
        orders = H.orders_of(api, family)
        first, second, _, _, _ = H.script(api, family, True)
        _, after_reset, _, _, _ = H.script(api, family, True, reset_before_second=True)
        H.sensitive(second, after_reset, family)
        ofirst, osecond, _, _, _ = H.script(None, family, False, orders=orders)
        _, oafter_reset, _, _, _ = H.script(None, family, False, orders=orders, reset_before_second=True)
        H.sensitive(osecond, oafter_reset, family)
        for name, got, want in (("first", first, ofirst), ("second", second, osecond)):
            if H.ORACLE[family] == "tolerance":
                assert cases.fro_err(got.X, want.X) < 1e-5 and cases.fro_err(got.Y, want.Y) < 1e-5 and cases.rel_err(got.objcol, want.objcol) < 1e-5, (family, name)
            else:
                assert got.differs_from(want, keys=H.DECISIONS) is None, (family, name, "against the oracle", got.differs_from(want, keys=H.DECISIONS))
        _SCRIPTS[family] = (first, second)
    return _SCRIPTS[family]


def check_undisturbed(family, probe, what):
    first, second = reference_script(family)
    f, s, before, after, out = H.script(hip(), family, True, probe=probe)
    for name, a, b in zip(("dX", "dY", "dObjCol", "dObjRow"), before, after):
        assert H.same_bits(a, b), (family, what, f"{name} changed across the call")
    assert f.differs_from(first) is None, (family, what, f.differs_from(first))
    assert s.differs_from(second) is None, (family, what, "the steps after the call", s.differs_from(second))
    return out


@pytest.mark.parametrize("family", list(H.LIST_F64))
def test_the_probes_leave_a_stepping_sequence_alone(monkeypatch, family):
    """Every probe in one script.  The multi-dimensional family takes the probes that serve it."""
    H.set_family(monkeypatch, family)
    names = H.probes_of(family)
    out = check_undisturbed(family, H.run_probes(names, family), names)
    assert [n for n, _ in out] == list(names)


@pytest.mark.parametrize("probe", list(H.PROBES))
def test_each_probe_on_the_gather_family(monkeypatch, probe):
    family = "gather, several wave classes"
    H.set_family(monkeypatch, family)
    check_undisturbed(family, H.run_probes((probe,), family), probe)


def _halve_the_steps(api, h, sh, b):
    api.reset_stepsizes(h, 0.5 * H.STEPPING["gather, several wave classes"][0])


def _move_one_ulp(api, h, sh, b):
    X, Y = b.factors()
    r = int(np.argmax(np.diff(sh.pa.rowptr)))   # the longest row: its vector enters the sums of 1 537 columns
    X[0, r] = np.nextafter(X[0, r], np.inf)
    api.set_factors(h, X, Y)


@pytest.mark.parametrize("disturb", [_halve_the_steps, _move_one_ulp], ids=["reset_stepsizes(0.5 s0)", "set_factors, one ulp"])
def test_the_comparison_sees_a_disturbed_handle(monkeypatch, disturb):
    """The self-checks of the two scripts of this section: a probe that DOES change state -- the step sizes, which only the later line
    searches show, or one element of X by one ulp -- fails the comparison."""
    family = "gather, several wave classes"
    H.set_family(monkeypatch, family)
    first, second = reference_script(family)
    f, s, before, after, _ = H.script(hip(), family, True, probe=disturb)
    assert f.differs_from(first) is None
    assert s.differs_from(second) is not None, "the comparison cannot see what it is for"
    if disturb is _halve_the_steps:   # nothing the buffers show: only the counters and what the searches did with the steps
        assert all(H.same_bits(a, b) for a, b in zip(before, after))
        assert any(s.counts[k] != second.counts[k] for k in H.DECISIONS), (s.counts, second.counts)
    else:
        assert not H.same_bits(before[0], after[0])


def vectors_at(family, X, Y):
    """col_losses, row_penalties and col_penalties of a FRESH handle at (X, Y): what the calls are documented to write."""
    api, sh = hip(), H.shape_of(family)
    h = H.create(api, family)
    try:
        b = H.Bound(api, h, sh.pa, True)
        api.set_factors(h, X, Y)
        api.col_losses(h)
        losses = b.read()[2]
        api.row_penalties(h)
        px = b.read()[3]
        api.col_penalties(h)
        py = b.read()[2]
        assert H.same_bits(b.read()[3], px)
        return losses, px, py
    finally:
        api.destroy(h)


@pytest.mark.parametrize("family", list(H.LIST_F64))
def test_calls_that_upload_factors_or_write_an_objective_vector(monkeypatch, family):
    """Each call alone between the two stretches, given back exactly what get_factors returned: the factors and the step sizes are
    undisturbed (the steps after it are the reference's), and dObjCol / dObjRow hold exactly what include/glrm_hip.h says."""
    H.set_family(monkeypatch, family)
    api, sh = hip(), H.shape_of(family)
    first, second = reference_script(family)
    pa = sh.pa
    losses, px, py = vectors_at(family, first.X, first.Y)
    reference_order = H.ORACLE[family] == "reference"
    doms = H.domains_for(family)

    def objective(reg):
        def call(api, h, sh, b):
            X, Y = b.factors()
            return api.objective(h, X, Y, include_reg=reg)
        return call

    def with_factors(fn):
        def call(api, h, sh, b):
            X, Y = b.factors()
            return fn(api, h, X, Y, doms)
        return call
    r, c = H.query_pairs(pa)
    same = "same"
    calls = {   # name: (call, dObjCol after it, dObjRow after it)
        "impute_at(X, Y)": (with_factors(lambda api, h, X, Y, d: api.impute_at(h, X, Y, d, pa.m, pa.n, rows=r, cols=c)), same, same),
        "impute": (with_factors(lambda api, h, X, Y, d: api.impute(h, X, Y, d, pa.m, pa.n)), same, same),
        "error_metric": (with_factors(lambda api, h, X, Y, d: api.error_metric(h, X, Y, d, False)), same, same),
        # loss pass, row penalties, column penalties in this order (device_objective); the reference-order handle sums the terms of the
        # loss itself and writes the two penalty vectors only
        "objective": (objective(True), py, px),
        "objective, losses only": (objective(False), same if reference_order else losses, same),
        "col_losses": (lambda api, h, sh, b: api.col_losses(h), losses, same),
        "row_penalties": (lambda api, h, sh, b: api.row_penalties(h), same, px),
        "col_penalties": (lambda api, h, sh, b: api.col_penalties(h), py, same),
    }
    values = {}
    for name, (call, want_col, want_row) in calls.items():
        f, s, before, after, out = H.script(api, family, True, probe=call)
        values[name] = out
        assert H.same_bits(before[0], after[0]) and H.same_bits(before[1], after[1]), (family, name, "the factors changed")
        assert H.same_bits(after[2], before[2] if want_col is same else want_col), (family, name, "dObjCol")
        assert H.same_bits(after[3], before[3] if want_row is same else want_row), (family, name, "dObjRow")
        assert f.differs_from(first) is None and s.differs_from(second) is None, (family, name, s.differs_from(second))
    if not reference_order:   # the objective is the fixed-order sum of exactly these vectors
        assert values["objective"] == pytest.approx(losses.sum() + px.sum() + py.sum(), rel=1e-12)
        assert values["objective, losses only"] == pytest.approx(losses.sum(), rel=1e-12)


def test_init_svd_and_fit_sparse_leave_what_the_header_says(monkeypatch):
    """init_svd writes the caller's buffers only.  fit_sparse leaves the best model found in the resident factors, the column penalties
    in dObjCol and the row penalties in dObjRow (its last objective evaluation), and does not touch the step sizes."""
    family = "gather, several wave classes"
    H.set_family(monkeypatch, family)
    api, sh = hip(), H.shape_of(family)
    first, second = reference_script(family)

    def sparse_then_restore(api, h, sh, b):
        X, Y = b.factors()
        Xs, Ys = X.copy(order="F"), Y.copy(order="F")
        api.fit_sparse(h, L.SparseProxGradParams(0.01, max_iter=3), Xs, Ys)
        got = b.read()
        Xr, Yr = b.factors()
        assert H.same_bits(Xr, Xs) and H.same_bits(Yr, Ys)                 # the resident factors are the returned best model
        _, px, py = vectors_at(family, Xs, Ys)
        assert H.same_bits(got[2], py) and H.same_bits(got[3], px)
        api.set_factors(h, X, Y)                                            # back to where the stepping sequence stood
    f, s, before, after, _ = H.script(api, family, True, probe=sparse_then_restore)
    assert H.same_bits(before[0], after[0]) and H.same_bits(before[1], after[1])
    assert f.differs_from(first) is None and s.differs_from(second) is None, ("fit_sparse moved the step sizes", s.differs_from(second))
    check_undisturbed(family, H.run_probes(("init_svd",), family), "init_svd")


# ================================================================================================ C. calls that change state

@pytest.mark.parametrize("family", ["gather, several wave classes", "cached row sweep"])
def test_solve_x_leaves_its_rows_and_nothing_else(monkeypatch, family):
    """solve_x(3) off the cached family (the solve plan is built in the handle's arena mid-life) and on it; then reset_stepsizes, step_x,
    step_y equal a fresh handle given the factors the solve left, and a fit(p1) is R1."""
    H.set_family(monkeypatch, family)
    api, sh = hip(), H.shape_of(family)
    s0, mn = H.STEPPING[family]
    R1 = refs(family)["R1"]

    def tail(b):
        api.reset_stepsizes(b.h, s0)
        api.kernel_stats(b.h, reset=True)
        api.step_x(b.h, mn)
        api.step_y(b.h, mn)
        X, Y = b.factors()
        return H.Stretch(X, Y, b.read()[2], H.counters(api.kernel_stats(b.h, reset=True)))
    h = H.create(api, family)
    try:
        b = H.Bound(api, h, sh.pa, True)
        api.set_factors(h, sh.X0, sh.Y0)
        api.reset_stepsizes(h, s0)
        api.step_x(h, mn)                       # the handle has a life before the solve
        api.step_y(h, mn)
        Xb, Yb = b.factors()
        api.solve_x(h, 3, mn)
        info = api.solve_x_info(h)
        assert info["fused_rows"] + info["loop_rows"] == sh.pa.m, info
        Xs, Ys = b.factors()
        assert H.same_bits(Ys, Yb) and not H.same_bits(Xs, Xb)   # Y is never written
        got = tail(b)
        api.bind_buffers(h, None, None, None, None)
        after = H.fit_on(api, h, H.p1(family), sh.X0, sh.Y0)
        assert after.differs_from(R1) is None, (family, "the fit after solve_x", after.differs_from(R1))
    finally:
        api.destroy(h)
    h = H.create(api, family)
    try:
        b = H.Bound(api, h, sh.pa, True)
        api.set_factors(h, Xs, Ys)
        want = tail(b)
    finally:
        api.destroy(h)
    assert got.differs_from(want) is None, (family, got.differs_from(want))
    assert want.counts["trials_x"] > want.counts["accepts_x"] > 0


@pytest.mark.parametrize("graph", [None, "0"], ids=["graph", "plain launches"])
def test_a_regularizer_round_trip_between_two_fits(monkeypatch, graph):
    """set_regularizers(new), a fit under it, set_regularizers(old): the next fit(p1) is R1 -- the captured iteration reads the
    descriptors from the device, so it is kept across the swap and must not hold anything of the old ones by value."""
    family = "gather, several wave classes"
    H.set_family(monkeypatch, family, graph)
    api, sh = hip(), H.shape_of(family)
    R1 = refs(family, graph)["R1"]
    new = np.array([L.OneReg(0.7).descriptor()], dtype=_capi.REG_DTYPE)
    h = H.create(api, family)
    try:
        assert H.fit_on(api, h, H.p1(family), sh.X0, sh.Y0).differs_from(R1) is None
        api.set_regularizers(h, new, new)
        under_new = H.fit_on(api, h, H.p1(family), sh.X0, sh.Y0)
        assert under_new.differs_from(R1) is not None                     # the new descriptors took effect
        api.set_regularizers(h, sh.pa.rx, sh.pa.ry)
        got = H.fit_on(api, h, H.p1(family), sh.X0, sh.Y0)
        assert got.differs_from(R1) is None, (graph, got.differs_from(R1))
    finally:
        api.destroy(h)
    h = H.create(api, family)                                             # the fit under the new descriptors: a fresh handle created with them
    try:
        api.set_regularizers(h, new, new)
        assert H.fit_on(api, h, H.p1(family), sh.X0, sh.Y0).differs_from(under_new) is None
    finally:
        api.destroy(h)


# ================================================================================================ D. the host layer's cached handle

def host_sequence(close_each):
    g, X0, Y0 = D.list_model()
    rng = np.random.default_rng(8)
    p = L.HipProxGradParams(1.0, max_iter=6, abs_tol=-1e300, rel_tol=-1e300)
    rows, cols = np.arange(0, g.m, 3), (np.arange(0, g.m, 3) * 7) % g.n
    A_new = rng.standard_normal((4, g.n))
    X_new0 = rng.standard_normal((g.k, 4))
    test_feats = [[int((3 * i + 1) % g.n)] for i in range(g.m)]
    out, handles = [], []

    def done(*arrays):
        out.extend(np.array(a, dtype=np.float64) for a in arrays)
        handles.append(None if g._handle_cache is None else g._handle_cache[1])
        if close_each:
            g.close()
    _, _, ch1 = L.fit_b(g, p, verbose=False)
    done(g.X, g.Y, ch1.objective)
    done(L.impute_at(g, rows, cols, params=p))
    rc, rs = L.recommend(g, rows, 3, params=p)
    done(rc, rs)
    done(L.sample_at(g, rows, cols, seed=5, params=p))
    Xn, cht = L.transform(g, A_new, p, X0=X_new0)
    done(Xn, cht.objective)
    res = L.precision_at_k(g, test_feats, params=p, reg_params=[0.1], verbose=False, kprec=5, rng=np.random.default_rng(3))
    done(res[0], res[1], res[2], res[5])
    _, _, ch2 = L.fit_b(g, p, verbose=False)
    done(g.X, g.Y, ch2.objective)
    g.close()
    return out, handles


def test_the_cached_handle_of_the_host_layer_answers_like_fresh_ones():
    kept, handles = host_sequence(False)
    assert handles[0] is not None and all(h is handles[0] for h in handles), "the model did not keep one handle: the test would be vacuous"
    fresh, _ = host_sequence(True)
    assert len(kept) == len(fresh)
    for i, (a, b) in enumerate(zip(kept, fresh)):
        assert H.same_bits(a, b), ("returned array number", i)


# ================================================================================================ E. sharded handles

@pytest.mark.parametrize("arrival", [1, 2])
def test_a_reused_sharded_handle_fits_like_fresh_ones(arrival):
    """Three shards on device 0, the X exchange in two chunks (test_gpu_devmem.test_a_sharded_fit_gives_back_what_it_took)."""
    g, X0, Y0 = D.list_model()
    api, pa = hip(), g.problem_arrays()
    pa1 = L.HipProxGradParams(1.0, max_iter=4, abs_tol=-1e300, rel_tol=-1e300)
    pa2 = L.HipProxGradParams(0.5, max_iter=4, inner_iter_X=2, inner_iter_Y=2, abs_tol=-1e300, rel_tol=-1e300, min_stepsize=0.02)

    def fit(mh, p):
        X, Y = X0.copy(order="F"), Y0.copy(order="F")
        obj, _ = api.multi_fit(mh, p, X, Y)
        return obj, X, Y

    def make():
        return api.multi_create(pa, 3, device_ids=[0, 0, 0], x_chunks=2, arrival=arrival)
    mh = make()
    try:
        runs = [fit(mh, p) for p in (pa1, pa1, pa2, pa1)]
    finally:
        api.multi_destroy(mh)
    fresh = []
    for p in (pa1, pa2):
        mh = make()
        try:
            fresh.append(fit(mh, p))
        finally:
            api.multi_destroy(mh)
    for i, want in ((0, fresh[0]), (1, fresh[0]), (2, fresh[1]), (3, fresh[0])):
        for name, a, b in zip(("objective", "X", "Y"), runs[i], want):
            assert H.same_bits(a, b), (arrival, f"fit number {i + 1} on the multi handle", name)
    # the single-device engine on the same model: the sharded fit is held to it at the tolerance test_multi_in_process.py holds it
    one = cases.run_engine(api, pa, X0, Y0, pa1)
    assert cases.rel_err(fresh[0][0][1:], one[0][1:]) < 1e-5 and cases.fro_err(fresh[0][1], one[1]) < 1e-5 and cases.fro_err(fresh[0][2], one[2]) < 1e-5
