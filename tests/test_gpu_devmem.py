"""-m gpu: device memory has one owner and every entry point one device scope (csrc/glrm_devmem.hpp).

The TEST BUILD of the engine counts the live allocations of its arenas (glrm_test_live_device_allocations, csrc/glrm_testhooks.hip; the
product library answers -1).  Every handle of every kernel family gives back exactly what it took when it is destroyed, every extension call
returns with the count it found (plus what it is documented to leave on the handle), and so does every refusal that fires after device memory
has been taken.  Borrowed arrays (GLRM_PROBLEM_BORROW_DEVICE_ARRAYS) never enter an arena and keep their contents.  With two devices visible:
no entry point leaves the caller's current device changed.  Shapes: the smallest ones test_gpu_families.py, test_gpu_edge_shapes.py and
test_gpu_storage_f32.py use to reach each family."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import cases
import lowrankmodels.jl_amd as L
import regs_vec
import shapes
import test_gpu_edge_shapes as E
import test_gpu_impute as I
import test_rows_from_cols as RC
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.domains import pack_domains
from shapes import Seg

pytestmark = pytest.mark.gpu
MIN_STEP = 0.01


def engine():
    return _capi.hip_testing_api()


def live():
    fn = engine().lib.glrm_test_live_device_allocations
    fn.restype = C.c_longlong
    n = fn()
    assert n >= 0, "the test build counts; -1 is the product library's answer"
    return n


@contextmanager
def balanced(extra=0):
    before = live()
    yield
    assert live() == before + extra, (before, live(), extra)


def test_the_product_library_does_not_count():
    fn = _capi.hip_api().lib.glrm_test_live_device_allocations
    fn.restype = C.c_longlong
    assert fn() == -1


# ------------------------------------------------------------------------------------------------ balance per family

def gather_shape():
    return shapes.build(1700, 1700, 32, E.gather_segments(4), fill=3, seed=32)


def cached_shape():
    k, cm = 32, 13 * 16
    segs = [Seg("r0", "row", 0, 0), Seg("r1", "row", 1, 1), Seg("r1536", "row", 2, 1536), Seg("rcut", "row", 3, cm), Seg("rcut1", "row", 4, cm + 1),
            Seg("c0", "col", 0, 0), Seg("c1600", "col", 1, 1600)]
    return shapes.build(1800, 1700, k, segs, fill=6, reg="nonneg", seed=k)


def tiled_shape():
    T = shapes.tile_rows(32)
    m, n = 3 * T + 1, 2 * T + 1
    return shapes.build(m, n, 32, E.window_segments(T, m, n, 4), fill=4, losses="per_column", seed=32)


def unordered(sh):
    """The same problem with every list reversed: out of tile order, so the engine sorts its private copy (GLRM_HIP_TILE_SORT=2)."""
    pa = sh.pa

    def rev(ptr, idx, vals):
        idx, vals = idx.copy(), vals.copy()
        for s in range(len(ptr) - 1):
            idx[ptr[s]:ptr[s + 1]] = idx[ptr[s]:ptr[s + 1]][::-1]
            vals[ptr[s]:ptr[s + 1]] = vals[ptr[s]:ptr[s + 1]][::-1]
        return idx, vals
    colidx, rowvals = rev(pa.rowptr, pa.colidx, pa.rowvals)
    rowidx, colvals = rev(pa.colptr, pa.rowidx, pa.colvals)
    return shapes.Shape(_capi.ProblemArrays(pa.m, pa.n, pa.k, pa.rowptr, colidx, rowvals, pa.colptr, rowidx, colvals, pa.losses, pa.rx, pa.ry),
                        sh.X0, sh.Y0, sh.segs, sh.T, sh.lists)


def lane_shape():
    segs = [Seg("c0", "col", 0, 0), Seg("r0", "row", 0, 0), Seg("c1", "col", 1, 1), Seg("cdup", "col", 2, 9, "dups")]
    return shapes.build(65, 511, 32, segs, fill=12, losses="per_column", seed=576)


def lane_quad_shape():
    segs = [Seg("c0", "col", 0, 0), Seg("r0", "row", 0, 0), Seg("c1", "col", 1, 1), Seg("cdup", "col", 2, 9, "dups")]
    return shapes.build(65, 511, 32, segs, fill=12, seed=577)


def blocked_shape():
    k, G = 32, 4
    T = shapes.tile_rows(k)
    m, n = 3 * T + 5, 2 * T + 3
    segs = E.window_segments(T, m, n, G, sup_rows=(3 * T, m))
    segs += [Seg("c199", "col", 20, 199), Seg("c200", "col", 21, 200), Seg("c201", "col", 22, 201, "dups")]
    return shapes.build(m, n, k, segs, fill=4, reg="nonneg", seed=132)


def dense_shape():
    rng = np.random.default_rng(5)
    m, n, k = 70, 50, 16
    g = L.GLRM(rng.standard_normal((m, n)), L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.1), k, X=rng.standard_normal((k, m)), Y=rng.standard_normal((k, n)))
    return shapes.Shape(g.problem_arrays(dense=True), np.asfortranarray(g.X), np.asfortranarray(g.Y), [], 0, {})


def multidim_shape():
    kwargs, _ = cases.build_multidim_case("mnl")
    g = L.GLRM(**kwargs)
    return shapes.Shape(g.problem_arrays(), np.asfortranarray(g.X), np.asfortranarray(g.Y), [], 0, {})


def from_cols_shape():
    both, cols_only, X0, Y0 = RC.pattern(np.random.default_rng(370), 300, 70, 5, 0.2)
    return shapes.Shape(cols_only, X0, Y0, [], 0, {})


BLOCKED_LONG = dict(E.BLOCKED, GLRM_HIP_BLOCKED_LONG_FROM="200")
TILED = E.TILED_R | E.TILED_C
FAMILIES = {  # name: (shape, environment, create kwargs, family bits wanted, check of the handle's reported order)
    "gather, several wave classes": (gather_shape, E.GATHER, {"tiled": 1}, 0, None),
    "cached row sweep": (cached_shape, dict(E.GATHER, GLRM_HIP_CACHED="1"), {"tiled": 0}, E.CACHED, None),
    "LDS tiles, loss per column (descriptor ids, rows regrouped)": (tiled_shape, E.FOUR_LANE, {"tiled": 2}, TILED, lambda o: o[0].private_order == 2),
    "LDS tiles, lists tile-sorted by the engine": (lambda: unordered(tiled_shape()), dict(E.FOUR_LANE, GLRM_HIP_TILE_SORT="2"), {"tiled": 2}, TILED,
                                                   lambda o: o[0].private_order == 1),
    "lane passes, padded stream": (lane_shape, {}, {"tiled": 2}, TILED | E.LANE_R | E.LANE_C, None),
    "lane passes, compact stream": (lane_quad_shape, {"GLRM_HIP_LANE_COMPACT": "1"}, {"tiled": 2}, TILED | E.LANE_R | E.LANE_C, None),
    "phase-aligned passes, long columns": (blocked_shape, BLOCKED_LONG, {"tiled": 1}, E.BLOCKED_R | E.BLOCKED_C, lambda o: o[1].long_from == 200),
    "dense, quad_gram": (dense_shape, {}, {"quad_gram": 1}, 4, None),
    "multi-dimensional losses": (multidim_shape, {}, {}, 8, None),
    "sum_order = 1": (gather_shape, {}, {"sum_order": 1}, 128, None),
    "storage = f32": (gather_shape, E.GATHER, {"storage": 1}, 0, None),
    "rows from columns": (from_cols_shape, E.GATHER, {}, 0, None),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_handle_gives_back_what_it_took(monkeypatch, family):
    make, env, create_kw, bits, order_ok = FAMILIES[family]
    for key in E.SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    sh = make()
    api = engine()
    with balanced():
        h = api.create(sh.pa, **create_kw)
        try:
            assert live() > 0
            st = api.kernel_stats(h)
            assert st["tiled"] & (E.ALL_BITS | 4 | 8 | 128) == bits, (family, st["tiled"])
            if order_ok is not None:
                assert order_ok([api.sum_order(h, 0), api.sum_order(h, 1)]), family
            api.set_factors(h, sh.X0, sh.Y0)
            api.reset_stepsizes(h, 1.0)
            api.step_x(h, MIN_STEP)
            api.step_y(h, MIN_STEP)
            api.synchronize(h)
        finally:
            api.destroy(h)


def test_a_borrowing_handle_frees_only_its_own_and_leaves_the_callers_arrays():
    from lowrankmodels.jl_amd import synth
    m, n, k, q = 4000, 1200, 32, 60
    w = synth.DeviceWorkload(m, n, k, q, loss_mix=1)   # a loss per column: the row view is regrouped into a private copy, the column view is read in place
    mine = (w.rowptr, w.colidx, w.rowvals, w.colptr, w.rowidx, w.colvals)
    snap = [t.clone() for t in mine]
    api = engine()
    with balanced():
        h = api.create(w.problem(borrow=True), tiled=2)
        try:
            assert api.kernel_stats(h)["tiled"] & TILED == TILED
            ld = api.factor_ld(h)
            dX, dY = w.init_factors(ld)
            api.set_factors(h, np.asfortranarray(0.3 * dX.cpu().numpy().reshape(m, ld)[:, :k].T), np.asfortranarray(0.3 * dY.cpu().numpy().reshape(n, ld)[:, :k].T))
            api.reset_stepsizes(h, 1.0)
            api.step_x(h, MIN_STEP)
            api.step_y(h, MIN_STEP)
        finally:
            api.destroy(h)
    torch.cuda.synchronize()
    for a, b in zip(snap, mine):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ balance per extension call

def list_model(seed=21, m=60, n=40, k=5):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, k)) @ rng.standard_normal((k, n))
    Ii, Jj = np.nonzero(rng.random((m, n)) < 0.5)
    g = L.GLRM(A, L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.1), k, obs=(Ii, Jj), X=rng.standard_normal((k, m)), Y=rng.standard_normal((k, n)))
    return g, np.asfortranarray(g.X), np.asfortranarray(g.Y)


def vector_regs(g, fixed_value):
    """rx with fixed_latent_features on every row (2 pinned entries), ry as it is: the arguments of set_regularizers_vec."""
    rx = [L.fixed_latent_features(L.QuadReg(0.1), np.full(2, fixed_value)) for _ in range(g.m)]
    return regs_vec.vec_args(rx, g.ry, g.k)


def test_every_extension_call_returns_with_the_count_it_found():
    g, X0, Y0 = list_model()
    pa, m, n, k = g.problem_arrays(), g.m, g.n, g.k
    api = engine()
    doms = pack_domains([L.RealDomain()] * n)
    with balanced():
        api.scale_columns(pa, _capi.SCALE_EQUILIBRATE)
    with balanced():
        h = api.create(pa)
        try:
            api.set_factors(h, X0, Y0)   # the handle's own factors and objective buffers exist from here on
            with balanced():
                api.init_svd(h, X0.copy(order="F"), Y0.copy(order="F"))
            with balanced():
                api.init_kmeanspp(h, Y0.copy(order="F"), 3, np.linspace(0.1, 0.9, k - 1))
            with balanced():
                api.impute(h, X0, Y0, doms, m, n)
            with balanced():
                api.error_metric(h, X0, Y0, doms, True)
            before = live()
            child = api.subset(h, np.arange(pa.rowptr[-1]) % 3, np.arange(pa.colptr[-1]) % 3, 0)
            assert live() > before       # the child's own handle; the compacted views it was copied from are gone
            api.destroy(child)
            assert live() == before
            with balanced():
                q, _, _ = api.xy_select(h, X0, Y0, 7)
            with balanced():
                api.precision_scan(h, X0, Y0, q, pa.rowptr, pa.colidx, 5)
            with balanced():
                api.fit_sparse(h, L.SparseProxGradParams(0.01, max_iter=3), X0.copy(order="F"), Y0.copy(order="F"))
            with balanced(extra=2):      # the vector table and the length table of rx stay on the handle
                api.set_regularizers_vec(h, *vector_regs(g, 0.5))
            with balanced():             # the second call's tables replace the first's
                api.set_regularizers_vec(h, *vector_regs(g, 0.25))
            with balanced(extra=-2):     # the plain call drops them
                api.set_regularizers(h, pa.rx, pa.ry)
        finally:
            api.destroy(h)


# ------------------------------------------------------------------------------------------------ sharded fits (glrm_hip_multi_*)

@pytest.mark.parametrize("arrival", [1, 2])
def test_a_sharded_fit_gives_back_what_it_took(arrival):
    """Three shards on device 0, the X exchange in two chunks; arrival = 1: the Y half-step takes the chunks in arrival order (chunk events),
    arrival = 2: it waits for the whole exchange."""
    g, X0, Y0 = list_model()
    api = engine()
    with balanced():
        mh = api.multi_create(g.problem_arrays(), 3, device_ids=[0, 0, 0], x_chunks=2, arrival=arrival)
        try:
            assert live() > 0
            obj, _ = api.multi_fit(mh, L.HipProxGradParams(1.0, max_iter=2), X0.copy(order="F"), Y0.copy(order="F"))
            assert len(obj) == 3
            assert api.multi_info(mh, 3)["exchange"] == 0
        finally:
            api.multi_destroy(mh)


def test_the_replica_of_a_shard_is_counted():
    """A shard's replica of X, Y and the two objective vectors belongs to the shard's arena: bound to the handle, the four stand where the
    handle's own four would (ensure_owned, at the first set_factors), so one shard holds exactly what a single-device handle holds."""
    g, X0, Y0 = list_model()
    pa = g.problem_arrays()
    api = engine()
    before = live()
    h = api.create(pa)
    try:
        api.set_factors(h, X0, Y0)
        single = live() - before
    finally:
        api.destroy(h)
    assert live() == before
    mh = api.multi_create(pa, 1, device_ids=[0])
    try:
        assert live() - before == single, (live() - before, single)
    finally:
        api.multi_destroy(mh)
    assert live() == before


# ------------------------------------------------------------------------------------------------ balance on failing paths

def refused(code, fn, *args, **kw):
    with pytest.raises(_capi.GLRMError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, e.value.message)
    return e.value.message


def test_a_sharded_create_that_fails_before_its_replicas_exist_gives_everything_back(monkeypatch):
    g, X0, Y0 = list_model()
    monkeypatch.setenv("GLRM_HIP_TEST_FAIL_FINALIZE", "1")
    with balanced():
        msg = refused(_capi.ERR_OOM, engine().multi_create, g.problem_arrays(), 3, device_ids=[0, 0, 0])
    assert "shard" in msg and "injected" in msg, msg


def test_a_sharded_create_that_fails_after_its_replicas_exist_gives_everything_back(monkeypatch):
    """The emulator's mode is checked last: the replicas, the arrival events and the chunk events have been made by then."""
    g, X0, Y0 = list_model()
    monkeypatch.setenv("GLRM_EXCHANGE_EMULATE_GBPS", "1")
    monkeypatch.setenv("GLRM_EXCHANGE_EMULATE_MODE", "3")
    with balanced():
        msg = refused(_capi.ERR_INVALID, engine().multi_create, g.problem_arrays(), 2, device_ids=[0, 0])
    assert "must be 1" in msg and "or 2" in msg, msg


def test_a_set_up_that_fails_half_way_is_given_back_by_destroy(monkeypatch):
    g, X0, Y0 = list_model()
    api = engine()
    monkeypatch.setenv("GLRM_HIP_TEST_FAIL_FINALIZE", "1")
    with balanced():
        h = api.create(g.problem_arrays(), defer=True)
        try:
            assert "injected" in refused(_capi.ERR_OOM, api.finalize, h, api.signature(h))
        finally:
            api.destroy(h)


def test_impute_without_a_rule_gives_back_its_scratch():
    name, D, loss = I.UNSUPPORTED_PAIRS[0]
    g, X, Y, doms = I.table_model([(I.R, L.QuadLoss()), (D, loss)], 130, 3, seed=5)
    api = engine()
    with balanced():
        h = api.create(g.problem_arrays())
        try:
            api.set_factors(h, X, Y)
            with balanced():
                refused(_capi.ERR_UNSUPPORTED, api.impute, h, X, Y, doms, g.m, g.n)
            with balanced():
                refused(_capi.ERR_UNSUPPORTED, api.error_metric, h, X, Y, doms, False)
        finally:
            api.destroy(h)


def test_a_row_index_out_of_range_gives_back_the_half_built_handle():
    """Device arrays: nothing is checked on the host, the index check of the device transpose refuses after the row view has been allocated."""
    both, cols_only, X0, Y0 = RC.pattern(np.random.default_rng(370), 300, 70, 5, 0.2)
    badidx = cols_only.rowidx.copy()
    badidx[7] = 300
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in (cols_only.colptr, badidx, cols_only.colvals)]
    bad = _capi.ProblemArrays(300, 70, 5, None, None, None, *(int(x.data_ptr()) for x in t), both.losses, both.rx, both.ry,
                              flags=_capi.PROBLEM_ROWS_FROM_COLS | _capi.PROBLEM_DEVICE_ARRAYS)
    with balanced():
        assert "outside [0, m)" in refused(_capi.ERR_INVALID, engine().create, bad)


def test_a_refused_vector_table_leaves_the_previous_one_in_force():
    g, X0, Y0 = list_model()
    api = engine()
    with balanced():
        h = api.create(g.problem_arrays())
        try:
            api.set_factors(h, X0, Y0)
            with balanced(extra=2):
                api.set_regularizers_vec(h, *vector_regs(g, 0.5))
            rx, vx, ry, vy = vector_regs(g, 0.25)
            vec, length = vx
            length = length.copy()
            length[0] = g.k + 1          # nfix beyond k
            with balanced():
                refused(_capi.ERR_INVALID, api.set_regularizers_vec, h, rx, (vec, length), ry, vy)
            api.reset_stepsizes(h, 1.0)
            api.step_x(h, MIN_STEP)
            X, Y = np.zeros_like(X0), np.zeros_like(Y0)
            api.get_factors(h, X, Y)
            assert np.array_equal(X[:2], np.full((2, g.m), 0.5))   # the first call's vectors still pin the rows
        finally:
            api.destroy(h)


def test_a_value_beyond_float_range_gives_back_the_half_built_handle():
    g, X0, Y0 = list_model()
    pa = g.problem_arrays()
    pa.rowvals = pa.rowvals.copy()
    pa.rowvals[4] = 1e39
    with balanced():
        assert "f32" in refused(_capi.ERR_NONFINITE, engine().create, pa, storage=1)


# ------------------------------------------------------------------------------------------------ one device scope

def test_no_entry_point_changes_the_callers_current_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    g, X0, Y0 = list_model()
    pa, m, n, k = g.problem_arrays(), g.m, g.n, g.k
    doms = pack_domains([L.RealDomain()] * n)
    api = engine()
    torch.cuda.set_device(0)
    h = api.create(pa, device_id=1)
    kids = []

    def call(fn, *args, **kw):
        out = fn(*args, **kw)
        assert torch.cuda.current_device() == 0, fn.__name__
        return out
    try:
        assert torch.cuda.current_device() == 0
        call(api.set_factors, h, X0, Y0)
        call(api.step_x, h, MIN_STEP)                                   # a core entry point
        call(api.impute, h, X0, Y0, doms, m, n)
        call(api.error_metric, h, X0, Y0, doms, False)
        call(api.init_kmeanspp, h, Y0.copy(order="F"), 3, np.linspace(0.1, 0.9, k - 1))
        call(api.init_svd, h, X0.copy(order="F"), Y0.copy(order="F"))
        kids.append(call(api.subset, h, np.arange(pa.rowptr[-1]) % 3, np.arange(pa.colptr[-1]) % 3, 0))
        q, _, _ = call(api.xy_select, h, X0, Y0, 7)
        call(api.precision_scan, h, X0, Y0, q, pa.rowptr, pa.colidx, 5)
        call(api.scale_columns, pa, _capi.SCALE_EQUILIBRATE, device_id=1)
        call(api.fit_sparse, h, L.SparseProxGradParams(0.01, max_iter=2), X0.copy(order="F"), Y0.copy(order="F"))
        call(api.set_regularizers_vec, h, *vector_regs(g, 0.5))
        mh = call(api.multi_create, pa, 2, device_ids=[1, 0])            # the sharded entry points select every shard's device in turn
        try:
            call(api.multi_fit, mh, L.HipProxGradParams(1.0, max_iter=2), X0.copy(order="F"), Y0.copy(order="F"))
            call(api.multi_set_regularizers, mh, pa.rx, pa.ry)
            call(api.multi_info, mh, 2)
        finally:
            call(api.multi_destroy, mh)
    finally:
        for c in kids:
            api.destroy(c)
        api.destroy(h)
        assert torch.cuda.current_device() == 0
