"""What tests/test_gpu_handle_lifetime.py runs and compares: the families of test_gpu_devmem.FAMILIES with the parameters that make a
carried step size matter, whole fits and stepping scripts on fresh and on long-lived handles, the probes that promise to leave a stepping
sequence alone, and the bit-for-bit comparison.

Every comparison is of BITS (uint64 views: -0.0, NaN payloads and Inf included) -- there is no tolerance to choose.  The only tolerances
are the ones the families' own tests hold against the CPU oracle where the oracle cannot follow the engine's summation order."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

import lowrankmodels.jl_amd as L
import oracle as O
import shapes
import test_gpu_devmem as D
import test_gpu_edge_shapes as E
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.domains import pack_domains

FAMILIES = D.FAMILIES
FAMILY_BITS = E.ALL_BITS | 4 | 8 | 128
COUNTERS = ("trials_x", "accepts_x", "trials_y", "accepts_y", "launches_x", "launches_y")
DECISIONS = COUNTERS[:4]

#: how a fresh handle's run is held to the CPU oracle: "order" -- the oracle adds in the order the handle reports (O.set_sum_order) and
#: lands on the same bits, as test_gpu_edge_shapes.py holds these families; "reference" -- sum_order = 1, the oracle's own order, bits
#: (test_gpu_reforder.py); "tolerance" -- 1e-5, where the oracle cannot follow the order: the engine's private tile sort (private_order
#: = 1, test_gpu_parity.py), the dense path, the general sweeps of multi-dimensional losses and fp32 storage, as their own tests do
ORACLE = {
    "gather, several wave classes": "order", "cached row sweep": "order",
    "LDS tiles, loss per column (descriptor ids, rows regrouped)": "order", "LDS tiles, lists tile-sorted by the engine": "tolerance",
    "lane passes, padded stream": "order", "lane passes, compact stream": "order", "phase-aligned passes, long columns": "order",
    "dense, quad_gram": "tolerance", "multi-dimensional losses": "tolerance", "sum_order = 1": "reference", "storage = f32": "tolerance",
    "rows from columns": "order",
}
assert set(ORACLE) == set(FAMILIES)

#: (start step, min_stepsize) of the stepping scripts.  Chosen on the CPU oracle (which reports the same counters) so that the two
#: iterations after the probes both reject and accept on both views and count differently from the same iterations started with the step
#: sizes reset: from 1e3 (the transform tests' start) every segment searches down in the first two iterations and carries what it found.
#: Where the carried steps never reject again at min_stepsize = 0.01, a larger min_stepsize makes segments give up (alpha = 1.1 min, no
#: accept), which is carried state as well.
STEPPING = {name: (1e3, 0.01) for name in FAMILIES}
STEPPING["lane passes, compact stream"] = (100.0, 1.0)
STEPPING["multi-dimensional losses"] = (1e3, 10.0)
STEPPING["rows from columns"] = (1e3, 0.8)

#: the whole fits start every line search from 1e3, so all of them search: the reference's default min_stepsize ratio serves every family
FITTING = {name: (1e3, 0.01) for name in FAMILIES}

GRAPH_FAMILIES = ("gather, several wave classes", "storage = f32", "rows from columns")   # what graph_eligible (csrc/glrm_hip.hip) admits
LIST_F64 = tuple(n for n in FAMILIES if n not in ("dense, quad_gram", "storage = f32"))   # section B: fp64, single shard, lists


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@lru_cache(maxsize=None)
def shape_of(family):
    sh = FAMILIES[family][0]()
    if family == "storage = f32":   # a start both the float handle and the fp64 oracle hold exactly
        sh = shapes.Shape(sh.pa, np.asfortranarray(sh.X0.astype(np.float32).astype(np.float64)),
                          np.asfortranarray(sh.Y0.astype(np.float32).astype(np.float64)), sh.segs, sh.T, sh.lists)
    return sh


def set_family(monkeypatch, family, graph=None):
    """The family's forcing environment and nothing else; graph: None = GLRM_HIP_GRAPH unset, "0" = plain launches."""
    for key in E.SWITCHES + ("GLRM_HIP_GRAPH", "GLRM_HIP_TILE_SORT"):
        monkeypatch.delenv(key, raising=False)
    for key, v in FAMILIES[family][1].items():
        monkeypatch.setenv(key, v)
    if graph is not None:
        monkeypatch.setenv("GLRM_HIP_GRAPH", graph)
    O.set_threads(O.usable_cores())


def create(api, family, regs=None):
    """A handle of the family, checked to be ON the family (no case passes on a fallback).  regs: set_regularizers_vec arguments."""
    _, _, kw, want, order_ok = FAMILIES[family]
    h = api.create(shape_of(family).pa, **kw)
    try:
        got = api.kernel_stats(h)["tiled"] & FAMILY_BITS
        assert got == want, (family, got, want)
        if order_ok is not None:
            assert order_ok([api.sum_order(h, 0), api.sum_order(h, 1)]), family
        if regs is not None:
            api.set_regularizers_vec(h, *regs)
    except BaseException:
        api.destroy(h)
        raise
    return h


def counters(st):
    return {k: st[k] for k in COUNTERS}


# ------------------------------------------------------------------------------------------------ whole fits

@dataclass
class Fit:
    obj: np.ndarray
    X: np.ndarray
    Y: np.ndarray
    counts: dict

    def differs_from(self, other):
        """None when every bit and every counter is equal, else what differs."""
        bad = [n for n, a, b in (("objective", self.obj, other.obj), ("X", self.X, other.X), ("Y", self.Y, other.Y)) if not same_bits(a, b)]
        bad += [f"{k}: {self.counts[k]} != {other.counts[k]}" for k in COUNTERS if self.counts[k] != other.counts[k]]
        return bad or None


def p1(family):
    return L.ProxGradParams(FITTING[family][0], max_iter=4, abs_tol=-1e300, rel_tol=-1e300, min_stepsize=FITTING[family][1])


def p2(family):
    """Another stepsize and min_stepsize, two inner iterations: the captured iteration holds the step-size reset."""
    s, mn = FITTING[family]
    return L.ProxGradParams(0.5 * s, max_iter=4, inner_iter_X=2, inner_iter_Y=2, abs_tol=-1e300, rel_tol=-1e300, min_stepsize=2.0 * mn)


def link(family):
    s, mn = FITTING[family]
    return L.ProxGradParams(s, max_iter=1, abs_tol=-1e300, rel_tol=-1e300, min_stepsize=mn)


def fit_on(api, h, prm, X0, Y0, fit=None):
    """One fit from copies of (X0, Y0) with the counters zeroed before it: the outputs and the counts of this call alone."""
    X, Y = X0.copy(order="F"), Y0.copy(order="F")
    api.kernel_stats(h, reset=True)
    obj, _ = (fit or api.fit)(h, prm, X, Y)
    return Fit(obj, X, Y, counters(api.kernel_stats(h, reset=True)))


def fresh_fit(api, family, prm, X0, Y0, regs=None):
    h = create(api, family, regs)
    try:
        return fit_on(api, h, prm, X0, Y0)
    finally:
        api.destroy(h)


def orders_of(api, family):
    h = create(api, family)
    try:
        return [api.sum_order(h, 0), api.sum_order(h, 1)]
    finally:
        api.destroy(h)


@lru_cache(maxsize=None)
def dense_lists():
    """The dense family's problem as explicit observation lists, which is what the oracle takes (test_gpu_dense.py)."""
    rng = np.random.default_rng(5)   # test_gpu_devmem.dense_shape, draw for draw
    m, n, k = 70, 50, 16
    g = L.GLRM(rng.standard_normal((m, n)), L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.1), k, X=rng.standard_normal((k, m)), Y=rng.standard_normal((k, n)))
    sh = shape_of("dense, quad_gram")
    assert np.array_equal(g.problem_arrays(dense=True).dense_A, sh.pa.dense_A) and np.array_equal(g.X, sh.X0)
    return g.problem_arrays()


def oracle_handle(family, orders):
    oapi = O.oracle_api()
    h = oapi.create(dense_lists() if family == "dense, quad_gram" else shape_of(family).pa)
    if ORACLE[family] == "order":
        for w, o in enumerate(orders):
            O.set_sum_order(h, w, o)
    return oapi, h


def hold_fit_to_oracle(family, got, prm, X0, Y0, orders):
    """A fresh handle's fit against the oracle's, as the family's own tests hold it."""
    import cases
    oapi, h = oracle_handle(family, orders)
    try:
        ref = fit_on(oapi, h, prm, X0, Y0)
    finally:
        oapi.destroy(h)
    mode = ORACLE[family]
    if mode == "tolerance":
        assert cases.rel_err(got.obj, ref.obj) < 1e-5 and cases.fro_err(got.X, ref.X) < 1e-5 and cases.fro_err(got.Y, ref.Y) < 1e-5, family
        return ref
    assert same_bits(got.X, ref.X) and same_bits(got.Y, ref.Y), (family, "factors differ from the oracle's")
    for k in DECISIONS:
        assert got.counts[k] == ref.counts[k], (family, k, got.counts[k], ref.counts[k])
    if mode == "reference":   # (the initial objective is summed per column first on the device: test_gpu_reforder.identical)
        assert same_bits(got.obj[1:], ref.obj[1:]) and cases.rel_err(got.obj[:1], ref.obj[:1]) < 1e-12, family
    else:                     # (only the final sum over the columns differs: test_gpu_sum_order.engine_and_oracle_in_its_order)
        assert cases.rel_err(got.obj[1:], ref.obj[1:]) < 1e-13 and cases.rel_err(got.obj[:1], ref.obj[:1]) < 1e-5, family
    return ref


# ------------------------------------------------------------------------------------------------ stepping scripts

class Bound:
    """A handle with the four device buffers bound (as test_gpu_edge_shapes.half_steps binds them), so that dX, dY, dObjCol and dObjRow
    can be read around a probe; on the oracle: host buffers for the two objective vectors."""

    def __init__(self, api, h, pa, hip):
        self.api, self.h, self.pa, self.hip = api, h, pa, hip
        if hip:
            ld, dev = api.factor_ld(h), torch.device("cuda", 0)
            self.bufs = [torch.zeros(n, dtype=torch.float64, device=dev) for n in (pa.m * ld, pa.d * ld, pa.n, pa.m)]
            torch.cuda.synchronize()   # the zeros are written on torch's stream, the handle launches on its own
            api.bind_buffers(h, *[b.data_ptr() for b in self.bufs])
        else:
            self.bufs = [None, None, np.zeros(pa.n), np.zeros(pa.m)]
            api.bind_buffers(h, None, None, self.bufs[2], self.bufs[3])

    def read(self):
        """(dX, dY, dObjCol, dObjRow) as host arrays (the oracle: its factors through get_factors)."""
        self.api.synchronize(self.h)
        if self.hip:
            return [b.cpu().numpy().copy() for b in self.bufs]
        X, Y = np.zeros((self.pa.k, self.pa.m), order="F"), np.zeros((self.pa.k, self.pa.d), order="F")
        self.api.get_factors(self.h, X, Y)
        return [X, Y, self.bufs[2].copy(), self.bufs[3].copy()]

    def factors(self):
        X, Y = np.zeros((self.pa.k, self.pa.m), order="F"), np.zeros((self.pa.k, self.pa.d), order="F")
        self.api.get_factors(self.h, X, Y)
        return X, Y


@dataclass
class Stretch:
    X: np.ndarray
    Y: np.ndarray
    objcol: np.ndarray
    counts: dict

    def differs_from(self, other, keys=COUNTERS):
        bad = [n for n, a, b in (("X", self.X, other.X), ("Y", self.Y, other.Y), ("dObjCol", self.objcol, other.objcol)) if not same_bits(a, b)]
        bad += [f"{k}: {self.counts[k]} != {other.counts[k]}" for k in keys if self.counts[k] != other.counts[k]]
        return bad or None


def steps(b, pairs, min_step, since=None, launches_since=None):
    """`pairs` times (step_x, step_y): the factors, the per-column objective and the counts after.  since = None: the counters are zeroed
    before.  Otherwise they run on, and the counts are the totals minus `since` (trials and accepts) and minus `launches_since`."""
    if since is None:
        b.api.kernel_stats(b.h, reset=True)
        since = launches_since = dict.fromkeys(COUNTERS, 0)
    for _ in range(pairs):
        b.api.step_x(b.h, min_step)
        b.api.step_y(b.h, min_step)
    X, Y = b.factors()
    total = counters(b.api.kernel_stats(b.h))
    counts = {k: total[k] - (since if k in DECISIONS else launches_since)[k] for k in COUNTERS}
    return Stretch(X, Y, b.read()[2], counts)


def script(api, family, hip, probe=None, orders=None, reset_before_second=False, start=None):
    """set_factors, reset_stepsizes(s0), two (step_x, step_y), PROBE, two (step_x, step_y).  Returns (first stretch, second stretch,
    the four buffers before the probe, after it, what the probe returned).  reset_before_second: the second stretch from
    reset_stepsizes(s0) instead of the carried step sizes (the sensitivity check).  start: (X, Y) instead of the family's."""
    sh = shape_of(family)
    s0, mn = STEPPING[family]
    if hip:
        h = create(api, family)
    else:
        api, h = oracle_handle(family, orders)
    try:
        b = Bound(api, h, sh.pa, hip)
        api.set_factors(h, *(start or (sh.X0, sh.Y0)))
        api.reset_stepsizes(h, s0)
        first = steps(b, 2, mn)
        before = b.read()
        out = probe(api, h, sh, b) if probe is not None else None
        after = b.read()
        # The trial / accept totals run on across the probe: one that zeroed or bumped them shows in the second stretch's counts.  The
        # launch counts are taken from behind the probe (col_losses and its kin are launches of the sweep kernels).
        if reset_before_second:
            api.reset_stepsizes(h, s0)
        second = steps(b, 2, mn, since=first.counts, launches_since=counters(api.kernel_stats(h)))
        return first, second, before, after, out
    finally:
        api.destroy(h)


def sensitive(second, second_after_reset, family):
    """The sensitivity conditions of a reference run: the stretch after the probes rejects and accepts on both views, and counts
    differently from the same stretch started with the step sizes reset -- so a probe that disturbed them would show."""
    c, r = second.counts, second_after_reset.counts
    for v in "xy":
        assert c[f"trials_{v}"] > c[f"accepts_{v}"] > 0, (family, v, c)
    assert [c[k] for k in DECISIONS] != [r[k] for k in DECISIONS], (family, c, r)


# ------------------------------------------------------------------------------------------------ probes

def domains_of(sh):
    """The default domain of every column's loss (shapes.build: one QuadLoss, or the exact kinds in turn)."""
    pa = sh.pa
    if len(pa.losses) == 1:
        return pack_domains([L.RealDomain()] * pa.n)
    objs = [shapes.column_loss(shapes.EXACT_KINDS[f % len(shapes.EXACT_KINDS)], f) for f in range(pa.n)]
    assert np.array_equal(np.array([o.descriptor() for o in objs], dtype=_capi.LOSS_DTYPE), pa.losses)
    return pack_domains([L.default_domain(o) for o in objs])


def domains_for(family):
    if family == "multi-dimensional losses":
        import cases
        kwargs, _ = cases.build_multidim_case("mnl")   # test_gpu_devmem.multidim_shape
        return pack_domains([L.default_domain(lo) for lo in kwargs["losses"]])
    return domains_of(shape_of(family))


def query_pairs(pa, count=600):
    t = np.arange(count, dtype=np.int64)
    return (t * 7919) % pa.m, ((t * 104729) % pa.n).astype(np.int32)


def probe_impute_at(api, h, sh, b):
    pa, doms = sh.pa, b.doms
    r, c = query_pairs(pa)
    out = [api.impute_at(h, None, None, doms, pa.m, pa.n, rows=r, cols=c, block_entries=97)]
    assert api.impute_at_info()["blocks"] > 1
    out.append(api.impute_at(h, None, None, doms, pa.m, pa.n, rows=np.arange(min(3, pa.m)), block_entries=max(pa.n // 2, 1)))
    assert api.impute_at_info()["blocks"] > 1
    return out


def probe_sample_at(api, h, sh, b):
    pa, doms = sh.pa, b.doms
    r, c = query_pairs(pa)
    out = []
    for keep in (False, True):
        o, kept, sd = api.sample_at(h, None, None, doms, pa.m, pa.n, rows=r, cols=c, seed=11, noise="residual", keep_observed=keep, block_entries=97)
        out += [o, sd]
        if b.real_quad_columns:
            assert api.sample_at_info()["variance_columns"] > 0   # the variance pass ran
    return out


def probe_row_topk(api, h, sh, b):
    cols, vals, count = api.row_topk(h, None, None, np.arange(0, sh.pa.m, max(sh.pa.m // 40, 1)), 5, m=sh.pa.m)
    return [vals]


def probe_xy_select(api, h, sh, b):
    return [np.array(api.xy_select(h, None, None, 17), dtype=np.float64)]


def probe_precision_scan(api, h, sh, b):
    pa = sh.pa
    ptr = np.arange(pa.m + 1, dtype=np.int64)                       # one test entry per row
    idx = ((np.arange(pa.m, dtype=np.int64) * 31) % pa.n).astype(np.int32)
    q, _, _ = api.xy_select(h, None, None, max(pa.m // 2, 1))
    tp, fp, hits, rows = api.precision_scan(h, None, None, q, ptr, idx, 10)
    return [np.array([tp, fp, rows], dtype=np.float64)]


def probe_kernel_stats(api, h, sh, b):
    api.kernel_stats(h, reset=False)


def probe_sum_order(api, h, sh, b):
    api.sum_order(h, 0), api.sum_order(h, 1)


def probe_synchronize(api, h, sh, b):
    api.synchronize(h)


def probe_subset(api, h, sh, b):
    pa = sh.pa
    nnz = int(pa.colptr[-1])   # (both views hold the same entries; a rows-from-columns problem carries the column view only)
    child = api.subset(h, np.arange(nnz) % 3, np.arange(nnz) % 3, 0, invert=True)
    try:
        api.set_factors(child, sh.X0, sh.Y0)
        api.reset_stepsizes(child, 1.0)
        api.step_x(child, 0.01)
        api.step_y(child, 0.01)
        api.synchronize(child)
    finally:
        api.destroy(child)


def probe_init_svd(api, h, sh, b):
    X, Y = np.zeros_like(sh.X0), np.zeros_like(sh.Y0)
    api.init_svd(h, X, Y, max_iter=2)


def probe_init_kmeanspp(api, h, sh, b):
    k = sh.pa.k
    api.init_kmeanspp(h, sh.Y0.copy(order="F"), 3, np.linspace(0.1, 0.9, k - 1))


def probe_init_nndsvd(api, h, sh, b):
    X, Y = np.zeros_like(sh.X0), np.zeros_like(sh.Y0)
    api.init_nndsvd(h, X, Y, svd_max_iter=2)


PROBES = {"impute_at": probe_impute_at, "sample_at": probe_sample_at, "row_topk": probe_row_topk, "xy_select": probe_xy_select,
          "precision_scan": probe_precision_scan, "kernel_stats": probe_kernel_stats, "sum_order": probe_sum_order,
          "synchronize": probe_synchronize, "subset": probe_subset, "init_svd": probe_init_svd, "init_kmeanspp": probe_init_kmeanspp,
          "init_nndsvd": probe_init_nndsvd}
#: the probes that serve a model with multi-dimensional losses (the others refuse it: tested where they live)
MULTIDIM_PROBES = ("impute_at", "sample_at", "kernel_stats", "sum_order", "synchronize", "subset", "init_svd")


def probes_of(family):
    return MULTIDIM_PROBES if family == "multi-dimensional losses" else tuple(PROBES)


def run_probes(names, family):
    """One probe function that runs `names` in turn (a handle's domains are packed once)."""
    def probe(api, h, sh, b):
        b.doms = domains_for(family)
        b.real_quad_columns = family != "multi-dimensional losses"   # every other shape has QuadLoss columns with a Real domain
        out = []
        for n in names:
            out.append((n, PROBES[n](api, h, sh, b)))
        return out
    return probe
