"""CPU: the helper behind tests/test_gpu_dense_shapes.py -- the four storage layouts describe one matrix, and the oracle that the dense
path is held to at rtol = 1e-9 is itself four orders of magnitude closer than that to an extended-precision transcription."""
import numpy as np
import pytest

import dense_layouts as D
import lowrankmodels.jl_amd as L
import oracle as O


@pytest.mark.parametrize("rows,cols", [(None, None), ((3, 20), (5, 50))])
def test_relayout_indexes_back_to_the_same_matrix(rows, cols):
    rng = np.random.default_rng(1)
    m, n, k = 37, 50, 9
    A = rng.standard_normal((m, n))
    g = L.GLRM(A, L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), k)
    pa = g.problem_arrays(dense=True, rows=rows, cols=cols)
    assert np.array_equal(D.logical(pa), A)
    for colmajor in (0, 1):
        for pad in (0, 5):
            q = D.relayout(pa, colmajor, pad)
            assert q.dense_colmajor == colmajor and q.dense_ld == (m if colmajor else n) + pad and q.flags == pa.flags
            assert (q.row_begin, q.row_end, q.col_begin, q.col_end) == (pa.row_begin, pa.row_end, pa.col_begin, pa.col_end)
            assert np.array_equal(D.logical(q), A)                      # bit for bit: a copy
            buf = np.asarray(q.dense_A)
            assert buf.size == (n if colmajor else m) * q.dense_ld
            assert np.isnan(buf).sum() == pad * (n if colmajor else m)  # exactly the padding is NaN
            assert q.dense_keep is q.dense_A
    assert pa.dense_ld == n and not pa.dense_colmajor                   # the input is left as it was


def test_dense_problem_is_the_constructors_model():
    """dense_problem's lists are the ones GLRM builds for a fully observed matrix."""
    rng = np.random.default_rng(2)
    A = rng.standard_normal((7, 5))
    dense, lists = D.dense_problem(A, 9, 2.5, D.QUADREG, D.NONNEG)
    ref = L.GLRM(A, L.QuadLoss(2.5), L.QuadReg(0.1), L.NonNegConstraint(), 9).problem_arrays()
    for f in ("rowptr", "colidx", "rowvals", "colptr", "rowidx", "colvals", "losses", "rx", "ry"):
        assert np.array_equal(getattr(lists, f), getattr(ref, f)), f
    assert np.array_equal(D.logical(dense), A)


@pytest.mark.parametrize("m,n,k", D.LAUNCH_SHAPES)
def test_oracle_margin_against_longdouble(m, n, k):
    """The oracle's column losses and both gradients at the launch-shape problems against a numpy longdouble transcription, relative to
    the sum of the absolute values of each sum's terms: bound 1e-11 (the worst case of a sequential fp64 sum of 65 573 terms is
    65 573 eps = 1.5e-11; the tests on the device allow 1e-9).  Measured over the five shapes: sums of 65 573 terms 1.6e-14 .. 2.0e-14
    (column losses) and 1.9e-15 .. 7.1e-15 (gradients), sums of 40 terms 5e-16 .. 8e-16: the oracle stands more than 1e4 x inside the
    1e-9 it is used at."""
    A, X0, Y0, _, _ = D.launch_case(m, n, k)
    _, lists = D.dense_problem(A, k, D.LOSS_SCALE, D.ZEROREG, D.ZEROREG)
    api = O.oracle_api()
    O.set_threads(4)
    h = api.create(lists)
    oc = np.zeros(n)
    api.bind_buffers(h, None, None, oc, None)
    api.set_factors(h, X0, Y0)
    api.col_losses(h)
    closs = oc.copy()
    # alpha = l makes the step exactly 1: x_new = x - g (no regularizer), and g = x - x_new is exact to eps * |x| << |g|'s terms
    X1, Y1 = np.zeros_like(X0), np.zeros_like(Y0)
    api.gradstep_x(h, n + 1.0)
    api.get_factors(h, X1, Y1)
    GX = X0 - X1
    assert np.array_equal(Y1, Y0)
    api.set_factors(h, X0, Y0)
    api.gradstep_y(h, m + 1.0)
    api.get_factors(h, X1, Y1)
    GY = Y0 - Y1
    api.destroy(h)
    rows, cols, (cl, cla), (gx, gxa), (gy, gya) = D.longdouble_terms(A, X0, Y0, D.LOSS_SCALE)
    assert min(len(rows), len(cols)) == D.SMALL and max(len(rows), len(cols)) > 2000   # every long sum, a sample of the short ones
    # the start itself enters g = x - x_new with one rounding of its own
    e = (float(np.max(np.abs(closs[cols] - cl) / cla)), float(np.max(np.abs(GX[:, rows] - gx) / (gxa + np.abs(X0[:, rows])))),
         float(np.max(np.abs(GY[:, cols] - gy) / (gya + np.abs(Y0[:, cols])))))
    print(f"oracle vs longdouble {m} x {n}, k = {k}: column losses {e[0]:.2e}, grad X {e[1]:.2e}, grad Y {e[2]:.2e}")
    assert np.finfo(np.longdouble).eps < 1e-18, "numpy longdouble is not extended precision here"
    assert max(e) < 1e-11, e
