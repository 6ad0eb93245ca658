"""-m gpu: every sweep family against the oracle, BIT FOR BIT, on problems built for the edges where the kernels branch per segment
(tests/shapes.py): segment lengths at the gather sweep's wave classes (1 536 / 98 304) and lane-group trip counts, rows at the cached
sweep's cut, columns at long_from, observations in one tile window, in the last partial tile or super-tile, on both sides of a window edge,
duplicates, super-tile counts of 1 / 2 / the cap, the lane family's padding, stream forms and descriptor-id limit, the phase gate.

Every case (i) asserts the family bits of kernel_stats and the reported glrm_sum_order, and that each listed segment falls into the
per-segment class it was built for; (ii) runs ONE X half-step and then ONE Y half-step on both sides from the same start and requires every
column of X and Y, the per-column objective and the trial / accept totals to be equal (a mismatch lists the segments with their length,
class, tiles and super-tiles); (iii) compares the engine's half-steps with the REFERENCE-order oracle segment by segment -- a wrong TERM
shows there as an error far above rounding, while a wrong ORDER does not -- where a segment beyond 1e-9 only passes when the oracle's own
decision for it flips under set_accept_bias(+-1e-15); (iv) runs a few whole iterations through test_gpu_sum_order.engine_and_oracle_in_its_order.

Which (family, rank) pairs exist -- test_family_rank_pairs: the gather sweeps, LDS-tiled four-lane sweeps and phase-aligned passes at every
padded rank 8 / 16 / 32 / 64 / 128; the cached row sweep at padded ranks 32 and 64 only (the gather sweep otherwise); the lane-per-segment
passes at padded rank 32 only (the four / eight / sixteen-lane tiled kernels otherwise)."""
import numpy as np
import pytest
import torch

import family_env
import oracle as O
import shapes
import test_gpu_sum_order as S
from lowrankmodels.jl_amd import _capi
from shapes import Seg

pytestmark = pytest.mark.gpu
MIN_STEP = 0.01
TILED_R, TILED_C, BLOCKED_R, BLOCKED_C, CACHED, LANE_R, LANE_C = 1, 2, 16, 32, 64, 256, 512
ALL_BITS = TILED_R | TILED_C | BLOCKED_R | BLOCKED_C | CACHED | LANE_R | LANE_C
SWITCHES = ("GLRM_HIP_CACHED", "GLRM_HIP_CACHED_PERSIST", "GLRM_HIP_BLOCKED", "GLRM_HIP_BLOCKED_TPS", "GLRM_HIP_BLOCKED_FILL", "GLRM_HIP_BLOCKED_GATE",
            "GLRM_HIP_BLOCKED_LONG_FROM", "GLRM_HIP_TILED_LONG_FROM", "GLRM_HIP_COL_WORKGROUPS", "GLRM_HIP_LANE", "GLRM_HIP_LANE_DEAL",
            "GLRM_HIP_LANE_COMPACT", "GLRM_HIP_LANE_ROUNDS", "GLRM_HIP_LANE_GATHER_TO", "GLRM_HIP_LANE_GATHER_PACKED",
            "GLRM_HIP_LANE_GATHER_SPREAD", "GLRM_HIP_LANE_TAIL", "GLRM_HIP_LANE_TAIL_COLS", "GLRM_HIP_LANE_PER_OBS", "GLRM_HIP_GROUP_KINDS")
GATHER, BLOCKED, FOUR_LANE = family_env.GATHER, family_env.blocked("1", "3"), family_env.FOUR_LANE


# ------------------------------------------------------------------------------------------------ per-segment class and report

def seg_class(o, view, length):
    """The per-segment class a reported order puts a segment of `length` observations in (what eng_pass in oracle/glrm_oracle.c does)."""
    if o.family == 1:
        if view == "row" and o.cached_maxlen >= 0 and length <= o.cached_maxlen:
            return "cached"
        w = o.waves or (1 if length < o.waves4_from else 4 if length < o.waves8_from else 8)
        return f"waves{w}"
    if o.family == 2:
        return "diverted" if o.long_from > 0 and length >= o.long_from else "windowed"
    return "other"


def describe(sh, o, view, i, T):
    idx = sh.indices(view, i)
    d = {"seg": f"{view} {i}", "len": len(idx), "class": seg_class(o, view, len(idx))}
    if len(idx):
        sup = o.window * max(o.windows_per_sup, 1) if o.family == 2 and o.windows_per_sup > 0 else None
        d.update(tiles=(int(idx[0]) // T, int(idx[-1]) // T), sups=None if sup is None else (int(idx[0]) // sup, int(idx[-1]) // sup))
    named = [s.name for s in sh.segs if s.view == view and s.index == i]
    if named:
        d["name"] = named[0]
    return d


def mismatch_report(sh, orders, A, B, view):
    o = orders[0 if view == "row" else 1]
    bad = np.flatnonzero(np.any(A != B, axis=0))
    lines = [describe(sh, o, view, int(i), sh.T) for i in bad[:12]]
    return {"differing": len(bad), "of": A.shape[1], "segments": lines, "order": o.asdict()}


# ------------------------------------------------------------------------------------------------ the two half-steps on either side

def half_steps(api, pa, X0, Y0, stepsize, hip, orders=None, bias=0.0, y_start=None, do_y=True, **create_kw):
    """One X half-step, then one Y half-step (from the X it left, or from y_start = (X, Y) when given, X half-step skipped);
    returns X, Y after each, the per-column objective and the trial / accept totals after each."""
    h = api.create(pa, **create_kw)
    try:
        if orders is not None:
            for w, o in enumerate(orders):
                O.set_sum_order(h, w, o)
        if bias:
            O.set_accept_bias(h, bias)
        if hip:
            ld, dev = api.factor_ld(h), torch.device("cuda", 0)
            bufs = [torch.zeros(pa.m * ld, dtype=torch.float64, device=dev), torch.zeros(pa.d * ld, dtype=torch.float64, device=dev),
                    torch.zeros(pa.n, dtype=torch.float64, device=dev), torch.zeros(pa.m, dtype=torch.float64, device=dev)]
            torch.cuda.synchronize()   # the zeros are written on torch's stream, the handle launches on its own
            api.bind_buffers(h, *[b.data_ptr() for b in bufs])
            objcol = lambda: bufs[2].cpu().numpy().copy()   # noqa: E731
        else:
            oc = np.zeros(pa.n)
            api.bind_buffers(h, None, None, oc, None)
            objcol = lambda: oc.copy()   # noqa: E731
        out = {}
        X, Y = np.zeros_like(X0), np.zeros_like(Y0)
        if y_start is None:
            api.set_factors(h, X0, Y0)
            api.reset_stepsizes(h, stepsize)
            api.step_x(h, MIN_STEP)
            api.get_factors(h, X, Y)
            out["x"] = (X.copy(order="F"), Y.copy(order="F"), api.kernel_stats(h))
            if not do_y:
                return out
        else:
            api.set_factors(h, *y_start)
            api.reset_stepsizes(h, stepsize)
        api.step_y(h, MIN_STEP)
        api.get_factors(h, X, Y)
        out["y"] = (X.copy(order="F"), Y.copy(order="F"), api.kernel_stats(h), objcol())
        return out
    finally:
        api.destroy(h)


def rel_by_segment(A, B):
    den = np.maximum(np.abs(B).max(axis=0), 1e-300)
    return np.abs(A - B).max(axis=0) / den


def against_reference_order(sh, mine, start_x, start_y, stepsize, view):
    """The engine's half-step against the reference-order oracle's, segment by segment: beyond 1e-9 only where the oracle's own accept
    decision for the segment hangs on the last bits (it flips between accept bias +1e-15 and -1e-15)."""
    oapi = O.oracle_api()
    res = {}
    for bias in (0.0, 1e-15, -1e-15):
        if view == "row":
            r = half_steps(oapi, sh.pa, start_x, start_y, stepsize, False, bias=bias, do_y=False)["x"]
            res[bias] = r[0]
        else:
            r = half_steps(oapi, sh.pa, start_x, start_y, stepsize, False, bias=bias, y_start=(start_x, start_y))["y"]
            res[bias] = r[1]
    rel = rel_by_segment(mine, res[0.0])
    far = np.flatnonzero(rel > 1e-9)
    flips = np.any(res[1e-15] != res[-1e-15], axis=0)
    wrong = [int(i) for i in far if not flips[i]]
    return wrong, rel, len(far)


def run_case(monkeypatch, sh, env, create_kw, want_flags, forbid_flags, check_order, stepsize=1.0, iters=6):
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    api, oapi = _capi.hip_api(), O.oracle_api()
    O.set_threads(O.usable_cores())
    h = api.create(sh.pa, **create_kw)
    try:
        flags = api.kernel_stats(h)["tiled"]
        orders = [api.sum_order(h, 0), api.sum_order(h, 1)]
    finally:
        api.destroy(h)
    assert flags & want_flags == want_flags and not flags & forbid_flags, (flags, want_flags, forbid_flags)
    check_order(orders)
    for s in sh.segs:   # each boundary segment goes down the class it was built for, by the report and its own length
        got = seg_class(orders[0 if s.view == "row" else 1], s.view, s.length)
        assert got == s.intent, (s, got, orders[0 if s.view == "row" else 1].asdict())
    fams = tuple(o.asdict()["family_name"] for o in orders)

    g = half_steps(api, sh.pa, sh.X0, sh.Y0, stepsize, True, **create_kw)
    c = half_steps(oapi, sh.pa, sh.X0, sh.Y0, stepsize, False, orders=orders)
    Xg1, Yg1, sg1 = g["x"]
    Xc1, Yc1, sc1 = c["x"]
    assert np.array_equal(Yg1, sh.Y0) and np.array_equal(Yc1, sh.Y0)
    assert np.array_equal(Xg1, Xc1), ("X half-step differs from the oracle in the engine's order", mismatch_report(sh, orders, Xg1, Xc1, "row"))
    for key in ("trials_x", "accepts_x"):
        assert sg1[key] == sc1[key], (key, sg1[key], sc1[key])
    Xg2, Yg2, sg2, ocg = g["y"]
    Xc2, Yc2, sc2, occ = c["y"]
    assert np.array_equal(Xg2, Xg1) and np.array_equal(Xc2, Xc1)
    assert np.array_equal(Yg2, Yc2), ("Y half-step differs from the oracle in the engine's order", mismatch_report(sh, orders, Yg2, Yc2, "col"))
    assert np.array_equal(ocg, occ), ("per-column objective differs", np.flatnonzero(ocg != occ)[:12])
    for key in ("trials_x", "accepts_x", "trials_y", "accepts_y"):
        assert sg2[key] == sc2[key], (key, sg2[key], sc2[key])
    assert sg1["trials_x"] > 0 and sg2["trials_y"] > 0

    # wrong terms, not order: every segment within 1e-9 of the reference-order oracle, or a decision that hangs on the last bits
    for view, mine, sx, sy in (("row", Xg1, sh.X0, sh.Y0), ("col", Yg2, Xg1, sh.Y0)):
        wrong, rel, nfar = against_reference_order(sh, mine, sx, sy, stepsize, view)
        o = orders[0 if view == "row" else 1]
        assert not wrong, ("segments beyond 1e-9 of the reference order without a rounding tie", view, nfar,
                           [dict(describe(sh, o, view, i, sh.T), rel=float(rel[i])) for i in wrong[:12]])

    if iters:
        S.engine_and_oracle_in_its_order(sh.pa, sh.X0, sh.Y0, iters, want_flags, fams, forbid_flags=forbid_flags, **create_kw)
    return orders


def layout(o, lanes, comps, **fields):
    got = {"lanes": o.lanes, "comps": o.comps, **{f: getattr(o, f) for f in fields}}
    assert got == {"lanes": lanes, "comps": comps, **fields}, (got, o.asdict())


# ------------------------------------------------------------------------------------------------ gather sweeps (STRIDED)

def short_lengths(G):
    NG = 64 // G   # lane groups per wave: one trip of the wave covers NG observations
    return sorted({0, 1, G - 1, G, G + 1, NG - 1, NG, NG + 1, 2 * NG + 1})


def gather_segments(G, views=("col", "row"), start=0):
    segs = []
    for view in views:
        i = start
        for L_ in short_lengths(G):
            segs.append(Seg(f"{view}{L_}", view, i, L_, intent="waves1"))
            i += 1
        segs.append(Seg(f"{view}dup", view, i, 2 * (64 // G) + 3, "dups", intent="waves1"))
        i += 1
        for L_, cls in ((1535, "waves1"), (1536, "waves4"), (1537, "waves4")):
            segs.append(Seg(f"{view}{L_}", view, i, L_, intent=cls))
            i += 1
    return segs


@pytest.mark.parametrize("k", [8, 32, 33, 64, 128])
def test_gather_sweeps_at_trip_and_wave_class_edges(monkeypatch, k):
    kp, G = shapes.padded_rank(k)
    sh = shapes.build(1700, 1700, k, gather_segments(G), fill=3, seed=k)

    def check(o):
        for x in o:
            layout(x, G, kp // G, family=1, waves=0, batch=1)
        assert o[0].cached_maxlen == -1 and (o[0].waves4_from, o[0].waves8_from) == (1536, 98304)
    run_case(monkeypatch, sh, GATHER, {"tiled": 1}, 0, ALL_BITS, check)


def test_gather_sweeps_with_a_loss_per_column_and_a_regularizer_per_row(monkeypatch):
    """batch = 4 on every row (loss per observation) and on the one-wave columns only (batch_one_wave_only): the 1 535 / 1 536 columns sit
    on both sides of that switch."""
    sh = shapes.build(1700, 1700, 32, gather_segments(4), fill=3, losses="per_column", rx_per_row=True, seed=3)

    def check(o):
        layout(o[0], 4, 8, batch=4, batch_one_wave_only=0)
        layout(o[1], 4, 8, batch=4, batch_one_wave_only=1)
    run_case(monkeypatch, sh, GATHER, {"tiled": 1}, 0, ALL_BITS, check)


def test_gather_sweeps_eight_wave_columns(monkeypatch):
    """Columns of 98 303 / 98 304 / 98 305 observations: the 4 -> 8-wave class edge."""
    m = 98_420
    segs = [Seg("c98303", "col", 0, 98_303, intent="waves4"), Seg("c98304", "col", 1, 98_304, intent="waves8"),
            Seg("c98305", "col", 2, 98_305, "dups", intent="waves8"), Seg("c1536", "col", 3, 1536, intent="waves4"),
            Seg("c17", "col", 4, 17, intent="waves1")]
    sh = shapes.build(m, 300, 8, segs, fill=2, losses="huber", seed=8)

    def check(o):
        for x in o:
            layout(x, 4, 2, family=1, waves=0, cached_maxlen=-1)
    run_case(monkeypatch, sh, GATHER, {"tiled": 1}, 0, ALL_BITS, check, iters=4)


# ------------------------------------------------------------------------------------------------ cached row sweep

@pytest.mark.parametrize("persist", ["default", "0"])
@pytest.mark.parametrize("k", [32, 64])
def test_cached_rows_at_the_cut(monkeypatch, k, persist):
    """Rows of cached_maxlen - 1 / cached_maxlen / + 1 (104 at k = 64, 208 at k = 32), mixed with empty rows and a four-wave row: the cut
    between the cached sweep and the gather sweep of the same half-step."""
    kp, G = shapes.padded_rank(k)
    cm = 13 * (64 // G)
    segs = [Seg("r0", "row", 0, 0, intent="cached"), Seg("r1", "row", 1, 1, intent="cached"), Seg("r1536", "row", 2, 1536, intent="waves4")]
    i = 3
    for L_, cls in ((cm - 1, "cached"), (cm, "cached"), (cm + 1, "waves1")):
        for pl in ("uniform", "dups", "window"):
            segs.append(Seg(f"r{L_}{pl}", "row", i, L_, pl, 0, intent=cls))
            i += 1
    segs += [Seg("c0", "col", 0, 0, intent="waves1"), Seg("c1600", "col", 1, 1600, intent="waves4")]
    sh = shapes.build(1800, 1700, k, segs, fill=6, reg="nonneg", seed=k)
    env = family_env.cached(persist != "0")

    def check(o):
        layout(o[0], G, kp // G, family=1, cached_maxlen=cm, cached_waves=2)
        layout(o[1], G, kp // G, family=1, cached_maxlen=-1)
    run_case(monkeypatch, sh, env, {"tiled": 0}, CACHED, ALL_BITS & ~CACHED, check)


# ------------------------------------------------------------------------------------------------ LDS-tiled four-lane sweeps

def window_segments(T, m, n, G, sup_rows=None):
    """Columns (over the rows of X, tiles of T) and rows (over the columns, tiles of T) placed at the window edges."""
    segs = []
    for i, L_ in enumerate(sorted({0, 1, G - 1, G + 1})):
        segs.append(Seg(f"c{L_}", "col", i, L_, intent="windowed"))
    segs += [Seg("cwin1", "col", 10, 40, "window", 1, intent="windowed"), Seg("clast", "col", 11, 1, "last_tile", intent="windowed"),
             Seg("cedge", "col", 12, 8, "straddle", T, intent="windowed"), Seg("cedge2", "col", 13, 7, "straddle", 2 * T, intent="windowed"),
             Seg("cdup", "col", 14, 11, "dups", intent="windowed")]
    if sup_rows is not None:   # (as many rows as the last super-tile holds, up to 9)
        segs.append(Seg("clastsup", "col", 15, min(9, sup_rows[1] - sup_rows[0]), "range", sup_rows, intent="windowed"))
    segs += [Seg("r0", "row", 0, 0, intent="windowed"), Seg("r1", "row", 1, 1, intent="windowed"),
             Seg("rwin0", "row", 2, 30, "window", 0, intent="windowed"), Seg("rlast", "row", 3, 1, "last_tile", intent="windowed"),
             Seg("redge", "row", 4, 6, "straddle", T, intent="windowed"), Seg("rdup", "row", 5, 9, "dups", intent="windowed")]
    return segs


@pytest.mark.parametrize("k,sups", [(8, "two"), (16, "cap"), (64, "one"), (64, "default")])
def test_four_lane_tiles_at_window_and_super_tile_edges(monkeypatch, k, sups):
    """m = c T + 1 (the last tile holds one row), segments in one window, in the last partial tile or super-tile, across window edges;
    super-tiles of the column passes: one, two, at the cap (32 768 / T tiles, the last super-tile partial) and the default.  The
    k = 64 / one-super-tile case also diverts columns at long_from - 1 / long_from / + 1 (GLRM_HIP_TILED_LONG_FROM)."""
    kp, G = shapes.padded_rank(k)
    T = shapes.tile_rows(kp)
    cap = max(32768 // T, 1)
    m = (cap * T + 1) if sups == "cap" else 3 * T + 1
    n = 2 * T + 1
    ntiles = -(-m // T)
    groups = -(-n // (16 * (64 // G)))
    env = dict(FOUR_LANE)
    wps = {"one": ntiles, "two": -(-ntiles // 2), "cap": cap, "default": 1}[sups]
    if sups != "default":
        env["GLRM_HIP_COL_WORKGROUPS"] = str({"one": 1, "two": 2 * groups, "cap": 1}[sups])
    nsup = -(-ntiles // wps)
    segs = window_segments(T, m, n, G, sup_rows=((nsup - 1) * wps * T, m))
    if sups == "one":
        env["GLRM_HIP_TILED_LONG_FROM"] = "300"
        segs += [Seg("c299", "col", 20, 299, intent="windowed"), Seg("c300", "col", 21, 300, intent="diverted"),
                 Seg("c301", "col", 22, 301, "dups", intent="diverted")]
    sh = shapes.build(m, n, k, segs, fill=3, reg="one" if k == 16 else "quad", seed=k)

    def check(o):
        for x in o:
            layout(x, G, kp // G, family=2, window=T, batch=2, rotate=0, private_order=0)
        assert o[0].windows_per_sup == 0 and o[1].windows_per_sup == wps, (o[1].windows_per_sup, wps)
        assert o[1].long_from == (300 if sups == "one" else max(4096, 4 * (sh.pa.colptr[-1] // n))) and o[0].long_from == 0
    if sups == "cap":
        assert nsup == 2 and (m - 1) // T == cap                   # the last super-tile holds one tile of one row
    run_case(monkeypatch, sh, env, {"tiled": 2}, TILED_R | TILED_C, ALL_BITS & ~(TILED_R | TILED_C), check)


def test_four_lane_tiles_with_a_loss_per_column(monkeypatch):
    """rotate = 1 and batch = 4 on the column passes; rows regrouped by loss kind inside every window (private_order = 2)."""
    T = shapes.tile_rows(32)
    m, n = 3 * T + 1, 2 * T + 1
    sh = shapes.build(m, n, 32, window_segments(T, m, n, 4), fill=4, losses="per_column", seed=32)

    def check(o):
        layout(o[0], 4, 8, family=2, batch=4, rotate=0, private_order=2)
        layout(o[1], 4, 8, family=2, batch=4, rotate=1, private_order=0)
    run_case(monkeypatch, sh, FOUR_LANE, {"tiled": 2}, TILED_R | TILED_C, ALL_BITS & ~(TILED_R | TILED_C), check)


# ------------------------------------------------------------------------------------------------ lane per segment (k = 32)

LANE_FORMS = family_env.lane_forms("default", "deal off", "compact stream", "older forms (full grid / CSR)", "gathered, chunk lists", "gathered, packed lists",
                                   "a wave per row")


def lane_check(o):
    for x in o:
        layout(x, 2, 16, family=2, window=560, batch=2, rotate=2, private_order=0)


@pytest.mark.parametrize("form", list(LANE_FORMS))
def test_lane_passes_with_extreme_padding(monkeypatch, form):
    """A few columns of 400 observations inside ONE tile window among columns of a handful (one lane of a wave block busy for hundreds of
    steps while its neighbours idle), columns empty in most tiles, a row of 500 observations in one window; every form of the trial rounds
    (started at step 64 so the searches run several rounds), the padded and the compact stream, the deal of slots by class on and off."""
    T = 560
    m, n = 4 * T + 1, 700
    segs = [Seg(f"heavy{i}", "col", 3 * i, 400, "window", 1 + i % 2, intent="windowed") for i in range(4)]
    segs += [Seg(f"sparse{i}", "col", 20 + i, 3, intent="windowed") for i in range(4)]
    segs += [Seg("clast", "col", 30, 1, "last_tile", intent="windowed"), Seg("cedge", "col", 31, 10, "straddle", 2 * T, intent="windowed"),
             Seg("c0", "col", 32, 0, intent="windowed"), Seg("cdup", "col", 33, 13, "dups", intent="windowed")]
    segs += [Seg("rheavy", "row", 0, 500, "window", 0, intent="windowed"), Seg("r0", "row", 1, 0, intent="windowed"),
             Seg("rlast", "row", 2, 3, "last_tile", intent="windowed"), Seg("redge", "row", 3, 6, "straddle", T, intent="windowed")]
    sh = shapes.build(m, n, 32, segs, fill=5, seed=7)
    run_case(monkeypatch, sh, LANE_FORMS[form], {"tiled": 2}, TILED_R | TILED_C | LANE_R | LANE_C, BLOCKED_R | BLOCKED_C | CACHED, lane_check,
             stepsize=64.0, iters=4)


@pytest.mark.parametrize("m,n", [(63, 513), (64, 512), (65, 511), (511, 65), (512, 64), (513, 63)])
def test_lane_passes_at_wave_block_sizes(monkeypatch, m, n):
    """Segment counts one below, at and one above a 64-segment wave block and a 512-column workgroup."""
    segs = [Seg("c0", "col", 0, 0, intent="windowed"), Seg("r0", "row", 0, 0, intent="windowed"), Seg("c1", "col", 1, 1, intent="windowed"),
            Seg("cdup", "col", 2, 9, "dups", intent="windowed")]
    sh = shapes.build(m, n, 32, segs, fill=min(12, n - 3), losses="per_column", seed=m + n)

    def check(o):
        for x in o:
            layout(x, 2, 16, family=2, window=560, batch=2, rotate=2, private_order=0)
    run_case(monkeypatch, sh, {}, {"tiled": 2}, TILED_R | TILED_C | LANE_R | LANE_C, BLOCKED_R | BLOCKED_C | CACHED, check)


@pytest.mark.parametrize("distinct", [256, 257])
def test_lane_rows_and_the_descriptor_id_limit(monkeypatch, distinct):
    """256 distinct loss descriptors still number in one-byte ids: the rows stay on the lane passes; 257 do not, and the rows fall back to
    the four-lane kernels (kind-grouped windows, private_order = 2) while the columns stay on the lane passes."""
    T = 560
    segs = [Seg("rwin", "row", 0, 300, "window", 0, intent="windowed"), Seg("redge", "row", 1, 8, "straddle", T, intent="windowed"),
            Seg("cedge", "col", 0, 8, "straddle", T, intent="windowed")]
    sh = shapes.build(2 * T + 1, 2 * T + 1, 32, segs, fill=6, losses="distinct", distinct=distinct, seed=distinct)
    lane_rows = distinct <= 256

    def check(o):
        if lane_rows:
            layout(o[0], 2, 16, family=2, batch=2, rotate=2, private_order=0)
        else:
            layout(o[0], 4, 8, family=2, batch=4, rotate=0, private_order=2)
        layout(o[1], 2, 16, family=2, batch=2, rotate=2, private_order=0)
    want = TILED_R | TILED_C | LANE_C | (LANE_R if lane_rows else 0)
    run_case(monkeypatch, sh, {}, {"tiled": 2}, want, BLOCKED_R | BLOCKED_C | CACHED | (0 if lane_rows else LANE_R), check)


# ------------------------------------------------------------------------------------------------ phase-aligned passes

@pytest.mark.parametrize("gate", ["default", "1"])
@pytest.mark.parametrize("k", [16, 32, 64])
def test_phase_aligned_passes_at_edges(monkeypatch, k, gate):
    """One tile per super-tile, m = 3 T + 5 (the last super-tile partial): columns of 0 / 1 / G +- 1, in one super-tile only, in the last
    partial one, across a super-tile edge, duplicates, and at long_from - 1 / long_from / + 1 (GLRM_HIP_BLOCKED_LONG_FROM = 200); the
    phase gate at its default and at one row."""
    kp, G = shapes.padded_rank(k)
    T = shapes.tile_rows(kp)
    m, n = 3 * T + 5, 2 * T + 3
    segs = window_segments(T, m, n, G, sup_rows=(3 * T, m))
    segs += [Seg("c199", "col", 20, 199, intent="windowed"), Seg("c200", "col", 21, 200, intent="diverted"),
             Seg("c201", "col", 22, 201, "dups", intent="diverted"), Seg("csup1", "col", 23, 120, "window", 1, intent="windowed")]
    sh = shapes.build(m, n, k, segs, fill=4, reg="nonneg", seed=100 + k)
    env = dict(BLOCKED, GLRM_HIP_BLOCKED_LONG_FROM="200")
    if gate != "default":
        env["GLRM_HIP_BLOCKED_GATE"] = gate

    def check(o):
        for x in o:
            layout(x, G, kp // G, family=2, window=T, windows_per_sup=1, batch=2, private_order=0)
        assert o[1].long_from == 200 and o[0].long_from == 0
    run_case(monkeypatch, sh, env, {"tiled": 1}, BLOCKED_R | BLOCKED_C, ALL_BITS & ~(BLOCKED_R | BLOCKED_C), check)


# ------------------------------------------------------------------------------------------------ which (family, rank) pairs exist

FAMILY_RANK = {  # family: (environment, create kwargs)
    "gather": (GATHER, {"tiled": 1}),
    "cached": (family_env.cached(), {"tiled": 0}),
    "four-lane tiles": (FOUR_LANE, {"tiled": 2}),
    "lane": ({}, {"tiled": 2}),
    "phase-aligned": (BLOCKED, {"tiled": 1}),
}


@pytest.mark.parametrize("family", list(FAMILY_RANK))
def test_family_rank_pairs(monkeypatch, family):
    """Every family at every padded rank: where the family does not admit the rank, what the handle falls back to and reports instead."""
    env, kw = FAMILY_RANK[family]
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    api = _capi.hip_api()
    for k in (8, 16, 32, 33, 64, 128):
        kp, G = shapes.padded_rank(k)
        sh = shapes.build(400, 300, k, [], fill=6, seed=k)
        h = api.create(sh.pa, **kw)
        try:
            flags = api.kernel_stats(h)["tiled"]
            o = [api.sum_order(h, 0), api.sum_order(h, 1)]
        finally:
            api.destroy(h)
        fam = [x.family for x in o]
        if family == "gather":
            assert flags & ALL_BITS == 0 and fam == [1, 1] and o[0].lanes == G, (k, flags)
        elif family == "cached":
            if kp in (32, 64):
                assert flags & ALL_BITS == CACHED and o[0].cached_maxlen == 13 * (64 // G), (k, flags, o[0].asdict())
            else:   # refused: the register layout needs eight components per lane -- the plain gather sweep instead
                assert flags & ALL_BITS == 0 and o[0].cached_maxlen == -1 and fam == [1, 1], (k, flags, o[0].asdict())
        elif family in ("four-lane tiles", "lane"):
            lane = family == "lane" and kp == 32
            assert flags & ALL_BITS == TILED_R | TILED_C | (LANE_R | LANE_C if lane else 0) and fam == [2, 2], (k, flags)
            assert [(x.lanes, x.comps) for x in o] == ([(2, 16)] * 2 if lane else [(G, kp // G)] * 2), (k, [x.asdict() for x in o])
        else:
            assert flags & ALL_BITS == BLOCKED_R | BLOCKED_C and fam == [2, 2] and o[0].lanes == G, (k, flags)
