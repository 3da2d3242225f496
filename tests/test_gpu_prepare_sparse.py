"""Tier 2 (GPU): gpmpc_prepare_sparse -- the sparse (DTC / projected-process) GP on inducing inputs.

Accuracy against the longdouble restatement of tests/sparse_gp_ref.py by the rule
    tolerance = 10 e64 + 64 eps scale            (e64: the float64 restatement's own error against longdouble on that case,
                                                  computed here, never taken from the GPU; eps = 2^-52; scale = max magnitude)
and the contracts of include/gpmpc.h: the cached factors and their exact symmetry, the state being that of gpmpc_set_factors,
bitwise determinism and independence of "sparse_chunk_points", the state rules (mode 4, forget, a following prepare), the
argument errors, and the model-level option ModelConfig.num_inducing_points.
"""
import numpy as np
import pytest
import torch

import sparse_gp_ref as ref
from helpers import record

pytestmark = pytest.mark.gpu

CASE_NAMES = list(ref.CASES)


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


def _fresh():
    import gp_mpc_amd
    return gp_mpc_amd.HipEngine(0)


def _np(t):
    return t.cpu().numpy()


def _prepare_sparse(eng, c, **kw):
    eng.prepare_sparse(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, **kw)


def _predict(eng, c):
    out = eng.predict(c.Xq)
    return _np(out["mean"]), _np(out["var"])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# -- 1. accuracy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_accuracy_against_longdouble(engine, name):
    c = ref.case(name)
    _prepare_sparse(engine, c)
    mean, var = _predict(engine, c)
    e_mean = float(np.max(np.abs(mean - c.mean_ld)))
    e_var = float(np.max(np.abs(var - c.var_ld)))
    print(f"{name}: GPU mean {e_mean:.3e} (tol {c.tol_mean:.3e}, numpy {c.e64_mean:.3e})  "
          f"var {e_var:.3e} (tol {c.tol_var:.3e}, numpy {c.e64_var:.3e})")
    record(f"prepare_sparse[{name}]", mean=e_mean, var=e_var, numpy_mean=c.e64_mean, numpy_var=c.e64_var)
    assert e_mean <= c.tol_mean
    assert e_var <= c.tol_var


# -- 2. cached factors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_cached_factors_shapes_and_symmetry(engine, name):
    c = ref.case(name)
    _prepare_sparse(engine, c)
    iK, beta = engine.factors()
    assert tuple(iK.shape) == (c.D, c.M, c.M) and tuple(beta.shape) == (c.D, c.M)
    iK = _np(iK)
    assert np.all(np.isfinite(iK)) and np.all(np.isfinite(_np(beta)))
    assert _same_bits(iK, np.ascontiguousarray(np.swapaxes(iK, 1, 2)))


# -- 3. the state is the one gpmpc_set_factors leaves --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_state_equals_set_factors(engine, name):
    c = ref.case(name)
    D, E = c.D, c.E
    A, B, H = 1, 4, 5
    time = E == 5
    rng = np.random.default_rng(7)
    actions = rng.uniform(0.1, 0.9, size=(B, H, A))
    mu0 = rng.uniform(0.3, 0.7, size=D)
    S0 = np.diag(rng.uniform(1e-3, 3e-3, size=D))
    target = np.full(D + A, 0.5)
    W, W_T = np.eye(D + A), np.eye(D)
    mu_in = rng.uniform(0.2, 0.8, size=(B, E))
    if time:
        mu_in[:, 4] = rng.uniform(0.0, c.N - 1.0, size=B)
    var_in = np.stack([np.diag(rng.uniform(1e-3, 3e-3, size=E)) for _ in range(B)])
    if time:
        var_in[:, 4, :] = 0.0
        var_in[:, :, 4] = 0.0

    def run(eng):
        eng.set_cost(target, W, W_T, 1.0)
        r = eng.rollout(actions, mu0, S0, include_time=time, time0=3.0)
        m = eng.moments(mu_in, var_in)
        rl = eng.rollout_linear(actions, mu0, S0, include_time=time, time0=3.0)
        return [_np(r[k]) for k in ("J", "mu", "Sig")] + [_np(m[k]) for k in ("M", "S", "V")] + \
               [_np(rl[k]) for k in ("J", "mu", "Sig")]

    _prepare_sparse(engine, c)
    got = run(engine)
    iK, beta = engine.factors()
    other = _fresh()
    try:
        other.set_factors(c.Z, iK, beta, c.ls, c.os)
        want = run(other)
    finally:
        other.close()
    for g, w in zip(got, want):
        assert np.all(np.isfinite(g))
        assert _same_bits(g, w)


# -- 4. determinism ---------------------------------------------------------------------------------------------------------------
def _factors_and_predictions(eng, c):
    iK, beta = eng.factors()
    mean, var = _predict(eng, c)
    return _np(iK), _np(beta), mean, var


@pytest.mark.parametrize("name", ["n257_m70", "n1000_m130"])
def test_two_calls_give_the_same_bits(engine, name):
    c = ref.case(name)
    _prepare_sparse(engine, c)
    first = _factors_and_predictions(engine, c)
    _prepare_sparse(engine, c)
    second = _factors_and_predictions(engine, c)
    for a, b in zip(first, second):
        assert _same_bits(a, b)


def test_chunk_size_leaves_every_bit():
    c = ref.case("n1000_m130")
    eng = _fresh()
    try:
        _prepare_sparse(eng, c)
        auto = _factors_and_predictions(eng, c)
        for chunk in (64, 256):
            eng.set_option("sparse_chunk_points", chunk)
            _prepare_sparse(eng, c)
            for a, b in zip(auto, _factors_and_predictions(eng, c)):
                assert _same_bits(a, b), chunk
        with pytest.raises(Exception):
            eng.set_option("sparse_chunk_points", 100)               # not a multiple of 64
    finally:
        eng.close()


# -- 5. state rules ---------------------------------------------------------------------------------------------------------------
def test_state_rules():
    import gp_mpc_amd
    from gp_mpc_amd import _lib
    c = ref.case("n257_m70")
    eng, fresh = _fresh(), _fresh()
    try:
        _prepare_sparse(eng, c)
        assert eng.last_prepare_mode == 4
        assert eng.N == c.M
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:
            eng.forget([3])
        assert ei.value.code == _lib.GPMPC_ERR_ARG
        mean, var = _predict(eng, c)                                  # ... and the sparse model is still there
        assert np.max(np.abs(mean - c.mean_ld)) <= c.tol_mean and np.max(np.abs(var - c.var_ld)) <= c.tol_var
        eng.prepare(c.X, c.Y, c.ls, c.os, c.nz)
        assert eng.last_prepare_mode == 0
        fresh.prepare(c.X, c.Y, c.ls, c.os, c.nz)
        for a, b in zip(_factors_and_predictions(eng, c), _factors_and_predictions(fresh, c)):
            assert _same_bits(a, b)
    finally:
        eng.close()
        fresh.close()


# -- 6. errors --------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_cached_model_untouched():
    from gp_mpc_amd import _lib
    c = ref.case("n37_m16")
    eng = _fresh()
    try:
        eng.prepare(c.X, c.Y, c.ls, c.os, c.nz)
        before = _factors_and_predictions(eng, c)
        dev = [eng._dev(v) for v in (c.X, c.Y, c.Z, c.ls, c.os, c.nz)]
        X, Y, Z, ls, osc, nz = [t.data_ptr() for t in dev]
        N, M, D, E = c.N, c.M, c.D, c.E
        st = eng._stream()

        def call(X=X, Y=Y, N=N, Z=Z, M=M, ls=ls, osc=osc, nz=nz, jit=1e-6, D=D, E=E):
            return eng.lib.gpmpc_prepare_sparse(eng._h, X, Y, N, Z, M, ls, osc, nz, jit, D, E, st)

        bad = [dict(X=None), dict(Y=None), dict(Z=None), dict(ls=None), dict(osc=None), dict(nz=None), dict(N=0), dict(N=-3),
               dict(M=0), dict(M=-1), dict(jit=-1e-9), dict(jit=float("nan")), dict(jit=float("inf"))]
        for kw in bad:
            assert call(**kw) == _lib.GPMPC_ERR_ARG, kw
            assert eng.last_prepare_mode == 0
            for a, b in zip(before, _factors_and_predictions(eng, c)):
                assert _same_bits(a, b), kw
        assert eng.lib.gpmpc_prepare_sparse(None, X, Y, N, Z, M, ls, osc, nz, 1e-6, D, E, st) == _lib.GPMPC_ERR_ARG
        assert call(D=17, E=20) == _lib.GPMPC_ERR_LIMIT and call(E=25) == _lib.GPMPC_ERR_LIMIT
        assert call() == _lib.GPMPC_OK and eng.last_prepare_mode == 4
    finally:
        eng.close()


def test_lost_pivot_is_not_pd_and_leaves_no_model():
    import gp_mpc_amd
    c = ref.case("n37_m16")
    eng = _fresh()
    try:
        eng.prepare(c.X, c.Y, c.ls, c.os, c.nz)
        # a negative noise makes B = I + V V^T / n indefinite: the second Cholesky loses its first pivot
        with pytest.raises(gp_mpc_amd.NotPositiveDefiniteError):
            eng.prepare_sparse(c.X, c.Y, c.Z, c.ls, c.os, -c.nz, ref.JITTER_REL)
        with pytest.raises(gp_mpc_amd.GpmpcError):
            eng.factors()
        _prepare_sparse(eng, c)                                       # ... and the handle recovers
        mean, _ = _predict(eng, c)
        assert np.max(np.abs(mean - c.mean_ld)) <= c.tol_mean
    finally:
        eng.close()


def test_fewer_points_than_inducing_inputs(engine):
    """N < M is legal: 20 memory points on 37 inducing inputs agree with the float64 restatement to the rule's tolerance."""
    c = ref.case("n37_m16")
    X, Y, Z = c.X[:20], c.Y[:20], c.X
    iK_ld, beta_ld = ref.sparse_factors(X, Y, Z, c.ls, c.os, c.nz, ref.JITTER_REL, ref.LD)
    mean_ld, var_ld = ref.predict(Z, c.ls, c.os, iK_ld, beta_ld, c.Xq, ref.LD)
    iK64, beta64 = ref.sparse_factors(X, Y, Z, c.ls, c.os, c.nz, ref.JITTER_REL)
    mean64, var64 = ref.predict(Z, c.ls, c.os, iK64, beta64, c.Xq)
    engine.prepare_sparse(X, Y, Z, c.ls, c.os, c.nz, ref.JITTER_REL)
    out = engine.predict(c.Xq)
    e_mean, e_var = np.max(np.abs(_np(out["mean"]) - mean_ld)), np.max(np.abs(_np(out["var"]) - var_ld))
    tol_mean = 10 * np.max(np.abs(mean64 - mean_ld)) + 64 * ref.EPS * np.max(np.abs(mean_ld))
    tol_var = 10 * np.max(np.abs(var64 - var_ld)) + 64 * ref.EPS * np.max(np.abs(var_ld))
    print(f"N < M: GPU mean {e_mean:.3e} (tol {tol_mean:.3e})  var {e_var:.3e} (tol {tol_var:.3e})")
    assert e_mean <= tol_mean and e_var <= tol_var


# -- 7. model level ---------------------------------------------------------------------------------------------------------------
def test_model_level_option_equals_engine_level_call():
    from gp_mpc_amd import GpStateTransitionModel
    from gp_mpc_amd.config_classes.model_config import ModelConfig
    c = ref.case("n257_m70")
    gp_init = {"noise_covar.noise": list(c.nz), "base_kernel.lengthscale": c.ls.tolist(), "outputscale": list(c.os)}
    eng, other = _fresh(), _fresh()
    try:
        model = GpStateTransitionModel(ModelConfig(gp_init=gp_init, num_inducing_points=c.M), dim_state=3, dim_action=1, engine=eng)
        model.prepare_inference(torch.as_tensor(c.X), torch.as_tensor(c.Y))
        assert eng.last_prepare_mode == 4 and eng.N == c.M and len(model.x_mem) == c.N
        rng = np.random.default_rng(11)
        H = 5
        actions = rng.uniform(0.1, 0.9, size=(H, 1))
        mu0, S0 = rng.uniform(0.3, 0.7, size=3), np.diag(np.full(3, 2e-3))
        mu, Sig = model.predict_trajectory(actions, mu0, S0, H, 0)
        other.prepare_sparse(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL)
        want = other.rollout(actions[None], mu0, S0, stage_costs=False)
        assert _same_bits(mu.numpy(), _np(want["mu"][0])) and _same_bits(Sig.numpy(), _np(want["Sig"][0]))
        assert np.all(np.isfinite(mu.numpy()))
    finally:
        eng.close()
        other.close()
