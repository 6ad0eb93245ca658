"""transform (lowrankmodels.jl_amd/transform.py) without a GPU: on the oracle engine -- which has no transform extension -- the driver runs
its iteration as a loop of step_x calls, and must leave exactly what a hand-written loop of the step-level entry points leaves; the
stopping rule is proxgrad.jl:210-213; the argument rules raise."""
import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd.fit import _should_stop

M, N, K = 60, 25, 5


def fitted(seed=3):
    """A 'fitted' model (its Y is what transform reads) and new rows: 60 x 25, k = 5, QuadLoss + QuadReg, 40 % observed."""
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((K, N))
    model = L.GLRM(rng.standard_normal((8, N)), L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.2), K, Y=Y, X=rng.standard_normal((K, 8)))
    A = rng.standard_normal((M, K)) @ Y + 0.1 * rng.standard_normal((M, N))
    obs = np.nonzero(rng.random((M, N)) < 0.4)
    return model, A, obs, rng.standard_normal((K, M))


def by_hand(model, A, obs, X0, p):
    """reset_stepsizes / step_x / col_losses / col_penalties through the Api, as the reference's loop without STEP 2 orders them"""
    api = O.oracle_api()
    g = L.GLRM(A, L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.2), K, obs=obs, X=X0, Y=model.Y)
    h = api.create(g.problem_arrays())
    try:
        oc, orow = np.zeros(N), np.zeros(M)
        api.bind_buffers(h, None, None, oc.ctypes.data, orow.ctypes.data)
        X, Y = np.array(X0, order="F"), np.array(model.Y, order="F")
        api.set_factors(h, X, Y)
        api.reset_stepsizes(h, p.stepsize)
        api.col_losses(h)
        loss = api.sum(h, oc.ctypes.data, N)
        api.row_penalties(h)
        px = api.sum(h, orow.ctypes.data, M)
        api.col_penalties(h)
        objs = [loss + (px + api.sum(h, oc.ctypes.data, N))]
        for _ in range(p.max_iter):
            if p.inner_iter_X > 1:
                api.reset_stepsizes(h, p.stepsize)
            for _ in range(p.inner_iter_X):
                api.step_x(h, p.min_stepsize)
            api.col_losses(h)
            loss = api.sum(h, oc.ctypes.data, N)
            api.col_penalties(h)
            objs.append(loss + api.sum(h, oc.ctypes.data, N))
        api.get_factors(h, X, Y)
    finally:
        api.destroy(h)
    return X, np.array(objs)


@pytest.mark.parametrize("inner", [1, 3])
def test_transform_on_the_oracle_engine_is_the_step_x_loop(inner):
    model, A, obs, X0 = fitted()
    p = L.HipProxGradParams(1.0, max_iter=6, inner_iter_X=inner, abs_tol=0.0, rel_tol=0.0)
    Ybytes = model.Y.tobytes()
    X, ch = L.transform(model, A, p, obs=obs, X0=X0, api=O.oracle_api())
    Xh, objs = by_hand(model, A, obs, X0, p)
    assert X.shape == (K, M) and X.dtype == np.float64
    assert np.array_equal(X, Xh) and not np.array_equal(X, X0)
    assert len(ch.objective) == 7 and np.array_equal(np.array(ch.objective), objs)
    assert np.all(np.diff(objs[1:]) <= 0) and objs[-1] < objs[1]
    assert model.Y.tobytes() == Ybytes
    assert np.array_equal(L.inverse_transform(model, X), X.T @ model.Y)


def test_default_start_is_the_constructors_draw():
    model, A, obs, _ = fitted()
    p = L.HipProxGradParams(1.0, max_iter=0)
    X, ch = L.transform(model, A, p, obs=obs, rng=np.random.default_rng(5), api=O.oracle_api())
    assert np.array_equal(X, np.random.default_rng(5).standard_normal((K, M))) and len(ch.objective) == 1


def restated_stop(objs, scaled_abs_tol, rel_tol):
    """proxgrad.jl:210-213 on a recorded objective vector: the iteration the loop breaks at (or the last one)"""
    for i in range(1, len(objs)):
        dec = objs[i - 1] - objs[i]
        if i > 10 and (dec < scaled_abs_tol or dec / objs[i] < rel_tol):
            return i
    return len(objs) - 1


def test_the_stopping_rule_fires_where_the_restatement_says():
    model, A, obs, X0 = fitted()
    free = L.HipProxGradParams(1.0, max_iter=40, abs_tol=0.0, rel_tol=0.0)
    _, full = L.transform(model, A, free, obs=obs, X0=X0, api=O.oracle_api())
    objs = np.array(full.objective)
    assert len(objs) == 41
    nobs = len(obs[0])
    for abs_tol, rel_tol in ((0.0, 1e-3), (1e-5, 0.0), (1e-7, 1e-5)):
        want = restated_stop(objs, abs_tol * nobs, rel_tol)
        p = L.HipProxGradParams(1.0, max_iter=40, abs_tol=abs_tol, rel_tol=rel_tol)
        _, ch = L.transform(model, A, p, obs=obs, X0=X0, api=O.oracle_api())
        assert len(ch.objective) - 1 == want and np.array_equal(np.array(ch.objective), objs[: want + 1]), (abs_tol, rel_tol, want)
        assert all(not _should_stop(i, objs[i - 1], objs[i], abs_tol * nobs, rel_tol) for i in range(1, want))
    assert 10 < restated_stop(objs, 0.0, 1e-3) < 40                      # the rule does fire inside the run for one of the settings


def test_rx_rule_and_ngpus_refusal():
    model, A, obs, X0 = fitted()
    api = O.oracle_api()
    model.rx[3] = L.QuadReg(0.7)                                        # the fitted rows no longer carry one regularizer
    with pytest.raises(ValueError, match="rx is required"):
        L.transform(model, A, L.HipProxGradParams(max_iter=1), obs=obs, X0=X0, api=api)
    X, _ = L.transform(model, A, L.HipProxGradParams(max_iter=1), obs=obs, X0=X0, rx=L.QuadReg(0.1), api=api)
    assert X.shape == (K, M)
    with pytest.raises(ValueError, match="ngpus"):
        L.transform(model, A, L.HipProxGradParams(max_iter=1, ngpus=2), obs=obs, X0=X0, rx=L.QuadReg(0.1), api=api)
    with pytest.raises(TypeError):
        L.transform(model, A, L.ProxGradParams(), obs=obs, X0=X0, rx=L.QuadReg(0.1), api=api)
