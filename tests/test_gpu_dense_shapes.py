"""-m gpu: the dense hand-over (`glrm_problem.dense_A`, csrc/glrm_dense.hpp / .hip) in every storage layout a host may pass and in every
launch shape the host layer picks, one half-step at a time against the oracle run on the explicit lists of the same model.

What decides the launch shape (csrc/glrm_dense.hip): `launch_dense_any` takes the 16-wave workgroup (NWD = 16) when
nseg * nsup >= 256 * 256 and the 4-wave one otherwise; `pick_sup` cuts the opposing dimension into ceil(n_other / 32768) super-tiles.
The 65 573 x 40 problems (tests/dense_layouts.py) therefore run their long side on dense_pass_kernel<KP, *, 16> with a last workgroup
of 37 segments, and their short side on the 4-wave kernel over three super-tiles whose last one holds 21 797 vectors.  kernel_stats
does not say which instantiation ran; that these cases reach the 16-wave kernel was shown once by zeroing wave 15's operand in
dense_pass_kernel (a 4-wave workgroup has no wave 15): the launch-shape and mixed-activity tests failed, all 17, and nothing else."""
import ctypes
import functools
import time

import numpy as np
import pytest

import cases
import dense_layouts as D
import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd import _capi

pytestmark = pytest.mark.gpu
TIGHT = dict(rtol=1e-9, atol=1e-12)   # the project's tolerance for one dense half-step (tests/test_gpu_fullsize.py)
GRAM = dict(rtol=1e-7, atol=1e-10)    # ... with glrm_options.quad_gram
COUNTS = ("trials_x", "trials_y", "accepts_x", "accepts_y")


def hip():
    return _capi.hip_api()


@pytest.fixture(scope="module", autouse=True)
def release_shared_problems():
    """The launch-shape problems and the oracle's results on them are shared by the tests of this module and dropped after the last."""
    yield
    oracle_reference.cache_clear()
    mixed_problem.cache_clear()


# ---- 1. layouts are a pure copy ---------------------------------------------------------------------------------------------------

def small_model(m, n, k, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, k)) @ rng.standard_normal((k, n)) / np.sqrt(k) + 0.1 * rng.standard_normal((m, n))
    X0, Y0 = np.asfortranarray(rng.standard_normal((k, m))), np.asfortranarray(rng.standard_normal((k, n)))
    g = L.GLRM(A, L.QuadLoss(), L.QuadReg(0.1), L.NonNegConstraint(), k, X=X0, Y=Y0)
    assert g.dense_eligible()
    return g, X0, Y0


@pytest.mark.parametrize("m,n,k", [(37, 50, 9), (333, 257, 32), (130, 65, 64)])
@pytest.mark.parametrize("quad_gram", [0, 1])
def test_every_layout_gives_the_same_bits(m, n, k, quad_gram):
    """Row-major / column-major x ld = dimension / dimension + 5 (NaN in the padding) x host / device: both packed views are copies of
    the same entries, so three iterations give the objective vector, X and Y of the row-major, unpadded, host handle bit for bit.
    (That the NaN check leaves the padding alone has a test of its own below.)"""
    g, X0, Y0 = small_model(m, n, k, 2000 + m + n + k)
    params = L.ProxGradParams(max_iter=3)
    pa = g.problem_arrays(dense=True)
    o_ref, X_ref, Y_ref, st = cases.run_engine(hip(), pa, X0, Y0, params, quad_gram=quad_gram)
    assert st["tiled"] & 4 and len(o_ref) == 4 and np.all(np.isfinite(o_ref[1:]))
    for colmajor in (0, 1):
        for pad in (0, 5):
            for device in (False, True):
                q = D.relayout(pa, colmajor, pad, device)
                o, X, Y, st = cases.run_engine(hip(), q, X0, Y0, params, quad_gram=quad_gram)
                assert st["tiled"] & 4
                assert np.array_equal(o, o_ref) and np.array_equal(X, X_ref) and np.array_equal(Y, Y_ref), (colmajor, pad, device)


@pytest.mark.parametrize("colmajor", [0, 1])
@pytest.mark.parametrize("rows,cols", [(None, None), ((5, 30), (7, 41))])
def test_nan_in_the_padding_does_not_trip_the_nan_check(colmajor, rows, cols):
    """The NaN check (glrm_setup_dense) walks a HOST matrix, the shard's rows of it, along the storage order (a device matrix is not
    walked): with NaN in all of the padding and nowhere else create must not answer ERR_NONFINITE, whole or as a shard, and one NaN
    put on a logical entry of the same buffer must."""
    g, X0, Y0 = small_model(37, 50, 9, 3)
    q = D.relayout(g.problem_arrays(dense=True, rows=rows, cols=cols), colmajor, 5)
    buf = q.dense_A
    assert np.isnan(buf).sum() == 5 * buf.shape[0] and np.isnan(buf[:, -5:]).all()
    try:
        h = hip().create(q)
    except _capi.GLRMError as e:
        assert e.code != _capi.ERR_NONFINITE, "the NaN check read the padding: " + e.message
        raise
    hip().destroy(h)
    i, j = 6, 8                                   # inside the shard's row block
    buf[(j, i) if colmajor else (i, j)] = np.nan
    with pytest.raises(_capi.GLRMError) as ei:
        hip().create(q)
    assert ei.value.code == _capi.ERR_NONFINITE and "(6, 8)" in ei.value.message


# ---- 2. column-major shards -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("parts", ["two", "empty_sides"])
@pytest.mark.parametrize("quad_gram", [0, 1])
def test_column_major_shards_equal_one_row_major_shard(quad_gram, parts):
    """tests/test_gpu_dense.py::test_dense_two_shards_equal_one_shard with the shards created from a column-major host buffer with a
    padded leading dimension (glrm_setup_dense uploads each shard's row block and column block with 2D copies; which of them is a set
    of contiguous runs flips with the storage order), and with a partition in which every shard has one empty side (`ns <= 0`)."""
    import torch
    g, X0, Y0 = small_model(260, 150, 32, 8)
    m, n = g.m, g.n
    api, params = hip(), L.ProxGradParams(max_iter=6)
    o1, X1, Y1, _ = cases.run_engine(api, g.problem_arrays(dense=True), X0, Y0, params, quad_gram=quad_gram)
    bounds = {"two": ([(0, 100), (100, m)], [(0, 70), (70, n)]),
              "empty_sides": ([(0, 100), (100, m), (m, m)], [(0, 70), (70, 70), (70, n)])}[parts]
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda", 0)
    shards = [D.relayout(g.problem_arrays(rows=r, cols=c, dense=True), 1, 5) for r, c in zip(*bounds)]
    hs = [api.create(q, stream=stream, quad_gram=quad_gram) for q in shards]
    ld = api.factor_ld(hs[0])
    dX, dY = torch.zeros(m * ld, dtype=torch.float64, device=dev), torch.zeros(n * ld, dtype=torch.float64, device=dev)
    dC, dR = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(m, dtype=torch.float64, device=dev)
    for h in hs:
        api.bind_buffers(h, dX.data_ptr(), dY.data_ptr(), dC.data_ptr(), dR.data_ptr())
    api.set_factors(hs[0], X0, Y0)
    for h in hs:
        api.reset_stepsizes(h, params.stepsize)
    objs = []
    for _ in range(params.max_iter):
        for h in hs:
            api.step_x(h, params.min_stepsize)
        for h in hs:
            api.step_y(h, params.min_stepsize)
        objs.append(api.sum(hs[0], dC.data_ptr(), n))
    X2, Y2 = np.zeros_like(X0), np.zeros_like(Y0)
    api.get_factors(hs[0], X2, Y2)
    for h in hs:
        api.destroy(h)
    assert np.array_equal(X1, X2) and np.array_equal(Y1, Y2) and np.array_equal(o1[1:], np.array(objs))


# ---- 3. every launch shape against the oracle -------------------------------------------------------------------------------------

class Session:
    """One handle of either engine with a bound per-column objective buffer (device memory for the HIP engine, numpy for the oracle)."""

    def __init__(self, api, pa, **kw):
        self.api, self.n, self.dev = api, pa.n, api.device_type == "cuda"
        if self.dev:
            import torch
            kw["stream"] = torch.cuda.current_stream().cuda_stream
            self.oc = torch.zeros(pa.n, dtype=torch.float64, device="cuda")
            self.ptr = self.oc.data_ptr()
        else:
            self.oc = self.ptr = np.zeros(pa.n)
        self.h = api.create(pa, **kw)
        if pa.dense_A is not None:
            st = api.kernel_stats(self.h)
            assert st["tiled"] & 4 and st["nnz_rows"] == pa.m * pa.n, "the dense MFMA path was not taken"
        api.bind_buffers(self.h, None, None, self.ptr, None)

    def objcol(self):
        return self.oc.cpu().numpy() if self.dev else self.oc.copy()

    def factors(self, k, m):
        X, Y = np.zeros((k, m), order="F"), np.zeros((k, self.n), order="F")
        self.api.get_factors(self.h, X, Y)
        return X, Y

    def close(self):
        self.api.destroy(self.h)


def fixed_alpha(other, n_other):
    """gradstep_* moves a segment by alpha / (n_other + 1) times its gradient: this alpha makes that factor 1 / (2 scale |other|_2^2),
    the reciprocal of the largest curvature of the segment's loss -- the longest step that does not overshoot, which moves a vector by
    about its own size, so that a tolerance on the new vector is a tolerance on the gradient."""
    return (n_other + 1) / (2 * D.LOSS_SCALE * np.linalg.norm(other, 2) ** 2)


def probe_fixed(s, X0, Y0):
    """(a) the passes that make no decision: objective with and without the regularizers, col_losses into the bound buffer, one
    gradstep_x and then one gradstep_y at a fixed alpha."""
    api, h = s.api, s.h
    k, m = X0.shape
    out = {"obj_reg": api.objective(h, X0, Y0, True), "obj_loss": api.objective(h, X0, Y0, False)}
    api.set_factors(h, X0, Y0)
    api.col_losses(h)
    out["col_losses"] = s.objcol()
    api.gradstep_x(h, fixed_alpha(Y0, s.n))
    api.gradstep_y(h, fixed_alpha(X0, m))
    out["X"], out["Y"] = s.factors(k, m)
    return out


def probe_search(s, X0, Y0, stepsize=1.0, min_stepsize=0.01, iters=1):
    """(b) reset_stepsizes, then `iters` x (step_x, step_y): factors, the per-column objectives, their sum per iteration, the counts."""
    api, h = s.api, s.h
    k, m = X0.shape
    api.set_factors(h, X0, Y0)
    api.reset_stepsizes(h, stepsize)
    api.kernel_stats(h, reset=True)
    objs = []
    for _ in range(iters):
        api.step_x(h, min_stepsize)
        api.step_y(h, min_stepsize)
        objs.append(api.sum(h, s.ptr, s.n))
    out = {"objs": np.array(objs), "objcol": s.objcol()}
    out["X"], out["Y"] = s.factors(k, m)
    st = api.kernel_stats(h)
    out.update({c: st[c] for c in COUNTS})
    return out


def build(A, X0, Y0, rx, ry):
    dense, lists = D.dense_problem(A, X0.shape[0], D.LOSS_SCALE, rx, ry)
    return dense, lists, X0, Y0


@functools.lru_cache(maxsize=None)
def oracle_reference(m, n, k):
    """The oracle's probes (a) and (b) of one problem, computed once and shared (read-only) by the tests below."""
    dense, lists, X0, Y0 = build(*D.launch_case(m, n, k))
    O.set_threads(4)
    s = Session(O.oracle_api(), lists)
    ref = {"fixed": probe_fixed(s, X0, Y0), "search": probe_search(s, X0, Y0)}
    s.close()
    for d in ref.values():
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return dense, X0, Y0, ref


def engine_probes(dense, X0, Y0, quad_gram, fixed=True):
    s = Session(hip(), dense, quad_gram=quad_gram)   # (asserts that the handle is on the dense path)
    got = {"fixed": probe_fixed(s, X0, Y0) if fixed else None, "search": probe_search(s, X0, Y0)}
    s.close()
    return got


def assert_fixed(got, ref):
    for key in ("obj_reg", "obj_loss"):
        assert np.isfinite(ref[key])
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-9, atol=0, err_msg=key)
    for key in ("col_losses", "X", "Y"):
        np.testing.assert_allclose(got[key], ref[key], err_msg=key, **TIGHT)
    assert ref["obj_reg"] > ref["obj_loss"] > 0 and np.any(ref["X"] != 0) and np.any(ref["Y"] != 0)


def assert_search(got, ref):
    for key in ("X", "Y", "objcol", "objs"):
        assert np.all(np.isfinite(ref[key]))
        np.testing.assert_allclose(got[key], ref[key], err_msg=key, **TIGHT)
    assert {c: got[c] for c in COUNTS} == {c: ref[c] for c in COUNTS}
    assert ref["accepts_x"] > 0 and ref["accepts_y"] > 0


@pytest.mark.parametrize("m,n,k", D.LAUNCH_SHAPES)
def test_launch_shapes_without_decisions(m, n, k):
    """(a) on the launch-shape problems: every entry of col_losses and of both factors after gradstep_x / gradstep_y, and the objective
    with and without the regularizers, at rtol = 1e-9, atol = 1e-12.  Relies on launch_dense_any's rule nseg * nsup >= 65 536 for the
    16-wave kernel on the 65 573-segment side and on pick_sup's three super-tiles on the other."""
    dense, X0, Y0, ref = oracle_reference(m, n, k)
    s = Session(hip(), dense)
    got = probe_fixed(s, X0, Y0)
    s.close()
    assert_fixed(got, ref["fixed"])


@pytest.mark.parametrize("m,n,k", D.LAUNCH_SHAPES)
def test_launch_shapes_with_the_line_search(m, n, k):
    """(b) on the launch-shape problems: all of X, all of Y and dObjCol after step_x, step_y at 1e-9 / 1e-12, and trial and accept counts
    equal to the oracle's (a decision flips only if it sits within ~1e-13 of its boundary: ~1e-8 expected flips over 65 573 rows)."""
    dense, X0, Y0, ref = oracle_reference(m, n, k)
    got = engine_probes(dense, X0, Y0, 0, fixed=False)
    assert_search(got["search"], ref["search"])


@pytest.mark.parametrize("m,n,k", D.LAUNCH_SHAPES)
def test_launch_shapes_with_quad_gram(m, n, k):
    """(c) as (b) with glrm_options.quad_gram at its 1e-7 / 1e-10: the trial values come from the quadratic form, so at most 5 segments
    (rows of X, columns of Y, entries of dObjCol together) may fall outside and each count may differ from the oracle's by at most 5,
    the allowance tests/test_gpu_dense.py::compare_dense grants."""
    dense, X0, Y0, ref = oracle_reference(m, n, k)
    got, ref = engine_probes(dense, X0, Y0, 1, fixed=False)["search"], ref["search"]
    out = {key: int(np.count_nonzero(~np.isclose(got[key], ref[key], **GRAM).reshape(-1, got[key].shape[-1]).all(axis=0)))
           for key in ("X", "Y", "objcol")}
    diffs = {c: int(got[c] - ref[c]) for c in COUNTS}
    print(f"quad_gram {m} x {n}, k = {k}: segments outside 1e-7 / 1e-10: {out}; count differences: {diffs}")
    assert sum(out.values()) <= 5, out
    assert max(abs(v) for v in diffs.values()) <= 5, diffs
    np.testing.assert_allclose(got["objs"], ref["objs"], rtol=1e-7)


# ---- 4. mixed activity in the trial rounds ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mixed_problem():
    return build(*D.mixed_activity_case(32))


@pytest.mark.parametrize("min_stepsize", [0.01, 0.5])
def test_trial_rounds_with_mixed_activity(min_stepsize):
    """In the trial pass (`!GRAD`) a wave without an active segment skips its MFMAs but still stages the opposing factor and meets the
    barriers.  stepsize = 1e3 on dense_layouts.mixed_activity_case (rows over four decades, 8 to 23 halvings per row in the first X
    half-step, whole waves finishing rounds before their neighbours); with min_stepsize = 0.5 a quarter of the rows give up without an
    accepted trial.  Two iterations against the oracle: equal counts, factors and objectives at 1e-9 / 1e-12."""
    dense, lists, X0, Y0 = mixed_problem()
    O.set_threads(4)
    so = Session(O.oracle_api(), lists)
    ref = probe_search(so, X0, Y0, stepsize=1e3, min_stepsize=min_stepsize, iters=2)
    so.close()
    sg = Session(hip(), dense)
    got = probe_search(sg, X0, Y0, stepsize=1e3, min_stepsize=min_stepsize, iters=2)
    sg.close()
    print(f"mixed activity, min_stepsize = {min_stepsize}: engine {[got[c] for c in COUNTS]}, oracle {[ref[c] for c in COUNTS]} ({COUNTS})")
    assert {c: got[c] for c in COUNTS} == {c: ref[c] for c in COUNTS}
    for key in ("X", "Y", "objcol", "objs"):
        assert np.all(np.isfinite(ref[key]))
        np.testing.assert_allclose(got[key], ref[key], err_msg=key, **TIGHT)
    if min_stepsize == 0.01:
        assert got["trials_x"] > 3 * got["accepts_x"] > 0
    else:
        assert got["accepts_x"] < 2 * D.BIG


# ---- 5. small edges ---------------------------------------------------------------------------------------------------------------

EDGES = ([(1, 70, 9), (70, 1, 9)] + [(100, 100, k) for k in (9, 16, 17, 32, 33, 64)] +
         [(c, c, 20) for c in (15, 16, 17, 63, 64, 65, 127, 129)])   # c x c: both half-steps see c opposing vectors


@pytest.mark.parametrize("m,n,k", EDGES)
def test_small_edges(m, n, k):
    """One segment on either side, every rank class and its neighbours (kp = 16 / 32 / 64), and opposing counts around the 16-vector
    MFMA tile, the 64-vector stage and the rounding of the packed leading dimension: probes (a) and (b) against the oracle."""
    dense, X0, Y0, ref = oracle_reference(m, n, k)
    got = engine_probes(dense, X0, Y0, 0)
    assert_fixed(got["fixed"], ref["fixed"])
    assert_search(got["search"], ref["search"])


# ---- 6. many segments -------------------------------------------------------------------------------------------------------------

def test_two_million_rows_column_major():
    """2 100 000 x 16, k = 9, ZeroReg, column-major with ld = m as julia/HipGLRM.jl passes it (~6 GB on the device, most of it the
    padded column view).  dense_pack_kernel takes its segment tiles from gridDim.y: 2 100 224 / 32 = 65 632 of them, more than the
    65 535 some runtimes stop at; this one launches them.  Create, the objective against numpy (1e-10), and after step_x rows 0..15 and
    the last 300 against the oracle's step on the list problem made of exactly those rows and the same Y.  On the X half-step 2.1e6
    segments x 1 super-tile run the 16-wave kernel.  Takes 0.8 s."""
    import torch
    if torch.cuda.mem_get_info()[0] < 16e9:
        pytest.skip("needs 16 GB of free device memory")
    m, n, k = 2_100_000, 16, 9
    rng = np.random.default_rng(6)
    X0 = np.asfortranarray(rng.standard_normal((k, m)) / 3.0)
    Y0 = np.asfortranarray(rng.standard_normal((k, n)))
    At = np.ascontiguousarray((X0.T @ rng.standard_normal((k, n)) + 0.1 * rng.standard_normal((m, n))).T)   # n x m: column-major A
    zero = np.array([D.ZEROREG], dtype=_capi.REG_DTYPE)
    loss = np.array([(0, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, None, None, None, None, None, None, loss, zero, zero, dense_A=At, dense_ld=m, dense_colmajor=1)
    t0 = time.perf_counter()
    s = Session(hip(), pa)
    api, h = s.api, s.h
    R = X0.T @ Y0 - At.T
    want = float(np.sum(R * R, dtype=np.longdouble))
    assert api.objective(h, X0, Y0, False) == pytest.approx(want, rel=1e-10)
    api.set_factors(h, X0, Y0)
    p = L.ProxGradParams()
    api.reset_stepsizes(h, p.stepsize)
    api.step_x(h, p.min_stepsize)
    X1, _ = s.factors(k, m)
    st = api.kernel_stats(h)
    s.close()
    print(f"2.1e6 rows: create + objective + step_x {time.perf_counter() - t0:.2f} s; trials_x {st['trials_x']}, accepts_x {st['accepts_x']}")
    assert m <= st["trials_x"] and 0 < st["accepts_x"] <= m
    rows = np.concatenate([np.arange(16), np.arange(m - 300, m)])
    _, lists = D.dense_problem(np.ascontiguousarray(At[:, rows].T), k, 1.0, D.ZEROREG, D.ZEROREG)
    so = Session(O.oracle_api(), lists)
    so.api.set_factors(so.h, np.asfortranarray(X0[:, rows]), Y0)
    so.api.reset_stepsizes(so.h, p.stepsize)
    so.api.step_x(so.h, p.min_stepsize)
    Xo, _ = so.factors(k, len(rows))
    so.close()
    np.testing.assert_allclose(X1[:, rows], Xo, **TIGHT)
    assert np.all(np.any(X1[:, rows] != X0[:, rows], axis=0))   # the rows really moved


# ---- 7. refusals and messages -----------------------------------------------------------------------------------------------------

def test_refusals_leave_the_library_usable():
    g, X0, Y0 = small_model(40, 30, 16, 9)
    api = hip()
    good = g.problem_arrays(dense=True)

    def still_works():
        h = api.create(D.relayout(good, 1, 5))
        assert api.kernel_stats(h)["tiled"] & 4
        api.destroy(h)

    def raw_create(pa, **fields):
        cp = api._cproblem(pa)
        for f, v in fields.items():
            setattr(cp, f, v)
        o = _capi.COptions(-1, 0, 0, 0, None, 0, 0, 0, 0, 0, 0)
        h = ctypes.c_void_p()
        rc = api._f["create"](ctypes.byref(h), ctypes.byref(cp), ctypes.byref(o))
        assert not h.value
        return rc, api.last_error()

    still_works()
    # column-major needs ld >= m; n = 30 < m = 40 is what a caller passes who forgot the storage order
    q = D.relayout(good, 1, 0)
    q.dense_ld = g.n
    with pytest.raises(_capi.GLRMError) as ei:
        api.create(q)
    assert ei.value.code == _capi.ERR_INVALID and "dense_ld" in ei.value.message
    still_works()
    # a NaN at logical (3, 4) of the column-major padded matrix (whose padding is NaN as well) is reported as (3, 4)
    q = D.relayout(good, 1, 5)
    q.dense_A[4, 3] = np.nan
    with pytest.raises(_capi.GLRMError) as ei:
        api.create(q)
    assert ei.value.code == _capi.ERR_NONFINITE and "(3, 4)" in ei.value.message
    still_works()
    # ranks outside 9..64 through the raw ABI (GLRM.problem_arrays refuses them before the library sees them)
    for k in (8, 65):
        rc, msg = raw_create(good, k=k)
        assert rc == _capi.ERR_UNSUPPORTED and "9..64" in msg, (k, rc, msg)
        still_works()
    rc, msg = raw_create(good, dense_reserved=1)
    assert rc == _capi.ERR_INVALID and "dense_reserved" in msg
    still_works()
