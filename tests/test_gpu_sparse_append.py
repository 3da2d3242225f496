"""Tier 2 (GPU): gpmpc_sparse_append -- memory points joining a sparse GP in O(M^2).

Accuracy: build on the first N0 rows of a case, append the others, and compare gpmpc_predict with the longdouble from-scratch
restatement of the WHOLE memory (tests/sparse_append_ref.py, tests/sparse_gp_ref.py) by the project's rule for gpmpc_prepare_sparse
    tolerance = 10 e64 + 64 eps scale        (e64: the from-scratch float64 restatement's own error on the full memory; computed
                                              from the numpy restatements, never taken from the GPU)
and the contracts of include/gpmpc.h: exact symmetry, the state being that of gpmpc_set_factors, k points in one call = k calls,
determinism, the record being refreshed by gpmpc_prepare_sparse, the state rules (mode 5, the record dropped by gpmpc_prepare and
gpmpc_set_factors, forget), argument errors that leave everything untouched, and the model-level option
ModelConfig.inducing_refresh_every."""
import numpy as np
import pytest
import torch

import sparse_append_ref as ar
import sparse_gp_ref as ref
from helpers import record

pytestmark = pytest.mark.gpu

# M = 1; M = 16 in one call; M = 64 with the time input; M = 70 in one call (two column tiles, 64 points); M = 130 (three column
# tiles, five row groups); fewer points than inducing inputs; D = 1; D = 16 with E = 20
ACCURACY_CASES = ["m1", "n37_m16_29+8", "n257_m64_time_248+9", "n257_m70_193+64", "n150_m130", "n20_m37", "d1", "d16_e20"]


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


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _build(eng, c, n0=None):
    n0 = c.N0 if n0 is None else n0
    eng.prepare_sparse(c.X[:n0], c.Y[:n0], c.Z, c.ls, c.os, c.nz, ref.JITTER_REL)
    return n0


def _build_and_append(eng, c, n0=None, one_by_one=False):
    n0 = _build(eng, c, n0)
    if one_by_one:
        for q in range(n0, c.N):
            eng.sparse_append(c.X[q:q + 1], c.Y[q:q + 1])
    else:
        eng.sparse_append(c.X[n0:], c.Y[n0:])


def _state(eng, c):
    iK, beta = eng.factors()
    out = eng.predict(c.Xq)
    return _np(iK), _np(beta), _np(out["mean"]), _np(out["var"])


def _within_tolerance(eng, c, label):
    out = eng.predict(c.Xq)
    e_mean = float(np.max(np.abs(_np(out["mean"]) - c.mean_ld)))
    e_var = float(np.max(np.abs(_np(out["var"]) - c.var_ld)))
    print(f"{label}: GPU mean {e_mean:.3e} (tol {c.tol_mean:.3e}, numpy from scratch {c.e64_mean:.3e})  "
          f"var {e_var:.3e} (tol {c.tol_var:.3e}, numpy from scratch {c.e64_var:.3e})")
    record(f"sparse_append[{label}]", mean=e_mean, var=e_var, numpy_mean=c.e64_mean, numpy_var=c.e64_var)
    assert e_mean <= c.tol_mean
    assert e_var <= c.tol_var


# -- 1. accuracy, symmetry, shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ACCURACY_CASES)
def test_accuracy_against_longdouble_build_of_the_whole_memory(engine, name):
    c = ar.case(name)
    _build_and_append(engine, c)
    assert engine.last_prepare_mode == 5 and engine.N == c.M
    _within_tolerance(engine, c, name)


@pytest.mark.parametrize("name", ACCURACY_CASES)
def test_factors_exactly_symmetric_and_shapes_unchanged(engine, name):
    c = ar.case(name)
    _build_and_append(engine, c)
    iK, beta = engine.factors()
    assert tuple(iK.shape) == (c.D, c.M, c.M) and tuple(beta.shape) == (c.D, c.M)
    iK = _np(iK)
    assert np.all(np.isfinite(iK)) and np.all(np.isfinite(_np(beta)))
    assert _same_bits(iK, np.ascontiguousarray(np.swapaxes(iK, 1, 2)))


# -- 2. the state is the one gpmpc_set_factors leaves ---------------------------------------------------------------------------------
def test_state_equals_set_factors(engine):
    c = ar.case("n257_m70_193+64")
    D, E, A, B, H = c.D, c.E, 1, 2, 3
    rng = np.random.default_rng(7)
    actions = rng.uniform(0.1, 0.9, size=(B, H, A))
    mu0 = rng.uniform(0.3, 0.7, size=D)
    S0 = np.diag(rng.uniform(1e-3, 3e-3, size=D))
    mu_in = rng.uniform(0.2, 0.8, size=(B, E))
    var_in = np.stack([np.diag(rng.uniform(1e-3, 3e-3, size=E)) for _ in range(B)])

    def run(eng):
        eng.set_cost(np.full(D + A, 0.5), np.eye(D + A), np.eye(D), 1.0)
        p = eng.predict(c.Xq)
        m = eng.moments(mu_in, var_in)
        r = eng.rollout(actions, mu0, S0)
        return [_np(p[k]) for k in ("mean", "var")] + [_np(m[k]) for k in ("M", "S", "V")] + [_np(r[k]) for k in ("J", "mu", "Sig")]

    _build_and_append(engine, c)
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


# -- 3. determinism ----------------------------------------------------------------------------------------------------------------
def test_k_points_in_one_call_are_k_calls_and_two_runs_agree(engine):
    c = ar.case("n257_m70_193+64")
    n0 = c.N - 9                                                      # M = 70, k = 9
    _build_and_append(engine, c, n0)
    first = _state(engine, c)
    _build_and_append(engine, c, n0)
    second = _state(engine, c)
    _build_and_append(engine, c, n0, one_by_one=True)
    single = _state(engine, c)
    assert engine.last_prepare_mode == 5
    for a, b, s in zip(first, second, single):
        assert _same_bits(a, b)
        assert _same_bits(a, s)


def test_prepare_sparse_refreshes_the_record():
    """append; gpmpc_prepare_sparse of the full memory; the same append again: the bits of a fresh handle given the last two --
    and the first sequence once more gives its first bits (nothing of the earlier appends survives in the record)."""
    c = ar.case("n37_m16_29+8")
    extra_X, extra_Y = c.X[c.N0:], c.Y[c.N0:]
    eng, fresh = _fresh(), _fresh()
    try:
        _build_and_append(eng, c)
        first = _state(eng, c)
        eng.prepare_sparse(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL)
        eng.sparse_append(extra_X, extra_Y)
        again = _state(eng, c)
        fresh.prepare_sparse(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL)
        fresh.sparse_append(extra_X, extra_Y)
        for a, b in zip(again, _state(fresh, c)):
            assert _same_bits(a, b)
        _build_and_append(eng, c)
        for a, b in zip(first, _state(eng, c)):
            assert _same_bits(a, b)
    finally:
        eng.close()
        fresh.close()


# -- 4. state rules ----------------------------------------------------------------------------------------------------------------
def test_state_rules():
    import gp_mpc_amd
    from gp_mpc_amd import _lib
    c = ar.case("n37_m16_29+8")
    eng = _fresh()
    try:
        _build_and_append(eng, c)
        assert eng.last_prepare_mode == 5 and eng.N == c.M
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:              # no (X, Y) record after an append either
            eng.forget([3])
        assert ei.value.code == _lib.GPMPC_ERR_ARG
        _within_tolerance(eng, c, "after a refused forget")
        # gpmpc_prepare drops the record: an append is an argument error and the exact model keeps its bits
        eng.prepare(c.X, c.Y, c.ls, c.os, c.nz)
        assert eng.last_prepare_mode == 0
        before = _state(eng, c)
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:
            eng.sparse_append(c.X[:1], c.Y[:1])
        assert ei.value.code == _lib.GPMPC_ERR_ARG and eng.last_prepare_mode == 0
        for a, b in zip(before, _state(eng, c)):
            assert _same_bits(a, b)
        # ... and so does gpmpc_set_factors
        _build(eng, c)
        iK, beta = eng.factors()
        eng.set_factors(c.Z, iK, beta, c.ls, c.os)
        before = _state(eng, c)
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:
            eng.sparse_append(c.X[c.N0:], c.Y[c.N0:])
        assert ei.value.code == _lib.GPMPC_ERR_ARG
        for a, b in zip(before, _state(eng, c)):
            assert _same_bits(a, b)
        # a later gpmpc_prepare is a full factorisation
        _build_and_append(eng, c)
        eng.prepare(c.X, c.Y, c.ls, c.os, c.nz)
        assert eng.last_prepare_mode == 0
    finally:
        eng.close()


# -- 5. errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_model_and_record_untouched():
    from gp_mpc_amd import _lib
    c = ar.case("n37_m16_29+8")
    eng = _fresh()
    try:
        _build(eng, c)
        before = _state(eng, c)
        Xn, Yn = eng._dev(c.X[c.N0:]), eng._dev(c.Y[c.N0:])
        k, D, E = c.N - c.N0, c.D, c.E
        st = eng._stream()

        def call(X=Xn.data_ptr(), Y=Yn.data_ptr(), k=k, D=D, E=E):
            return eng.lib.gpmpc_sparse_append(eng._h, X, Y, k, D, E, st)

        for kw in (dict(X=None), dict(Y=None), dict(k=0), dict(k=-2), dict(D=D + 1), dict(D=D - 1), dict(E=E + 1), dict(E=E - 1)):
            assert call(**kw) == _lib.GPMPC_ERR_ARG, kw
            assert eng.last_prepare_mode == 4
            for a, b in zip(before, _state(eng, c)):
                assert _same_bits(a, b), kw
        assert eng.lib.gpmpc_sparse_append(None, Xn.data_ptr(), Yn.data_ptr(), k, D, E, st) == _lib.GPMPC_ERR_ARG
        assert call() == _lib.GPMPC_OK and eng.last_prepare_mode == 5          # the record is intact: a valid append still works
        _within_tolerance(eng, c, "after argument errors")
        empty = _fresh()                                                   # no model at all
        try:
            assert empty.lib.gpmpc_sparse_append(empty._h, Xn.data_ptr(), Yn.data_ptr(), k, D, E, st) == _lib.GPMPC_ERR_ARG
        finally:
            empty.close()
    finally:
        eng.close()


# -- 6. model level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("selection", ["strided", "greedy"])
def test_model_level_refresh_interval(selection):
    from gp_mpc_amd import GpStateTransitionModel
    from gp_mpc_amd.config_classes.model_config import ModelConfig
    c = ref.case("n37_m16")
    gp_init = {"noise_covar.noise": list(c.nz), "base_kernel.lengthscale": c.ls.tolist(), "outputscale": list(c.os)}
    eng = _fresh()
    try:
        cfg = ModelConfig(gp_init=gp_init, num_inducing_points=16, inducing_refresh_every=4, inducing_selection=selection)
        model = GpStateTransitionModel(cfg, dim_state=3, dim_action=1, engine=eng)
        X, Y = torch.as_tensor(c.X), torch.as_tensor(c.Y)
        modes = []
        for n in range(30, 37):
            model.prepare_inference(X[:n], Y[:n])
            modes.append(eng.last_prepare_mode)
            assert model.is_sparse and len(model.x_mem) == n and eng.N == 16
            idx = model.inducing_idx
            rows = idx.cpu().numpy().astype(np.int64) if isinstance(idx, torch.Tensor) else np.asarray(idx, dtype=np.int64)
            Z = c.X[rows]                                             # the SAME Z, from scratch on the whole memory so far
            iK_ld, beta_ld = ref.sparse_factors(c.X[:n], c.Y[:n], Z, c.ls, c.os, c.nz, ref.JITTER_REL, ref.LD)
            mean_ld, var_ld = ref.predict(Z, c.ls, c.os, iK_ld, beta_ld, c.Xq, ref.LD)
            iK64, beta64 = ref.sparse_factors(c.X[:n], c.Y[:n], Z, c.ls, c.os, c.nz, ref.JITTER_REL)
            mean64, var64 = ref.predict(Z, c.ls, c.os, iK64, beta64, c.Xq)
            tol_mean = 10 * np.max(np.abs(mean64 - mean_ld)) + 64 * ref.EPS * np.max(np.abs(mean_ld))
            tol_var = 10 * np.max(np.abs(var64 - var_ld)) + 64 * ref.EPS * np.max(np.abs(var_ld))
            out = eng.predict(c.Xq)
            e_mean, e_var = np.max(np.abs(_np(out["mean"]) - mean_ld)), np.max(np.abs(_np(out["var"]) - var_ld))
            print(f"{selection} n = {n} mode {modes[-1]}: mean {e_mean:.3e} (tol {tol_mean:.3e})  var {e_var:.3e} (tol {tol_var:.3e})")
            assert e_mean <= tol_mean and e_var <= tol_var
        assert modes == [4, 5, 5, 5, 5, 4, 5]
        model.prepare_inference(X[:36], Y[:36])                           # unchanged memory and hyper-parameters: no call at all
        assert eng.last_prepare_mode == 5
        model.models[1].initialize(**{"covar_module.outputscale": np.array(0.7)})
        model.prepare_inference(X[:37], Y[:37])                           # one more row, but other hyper-parameters: a rebuild
        assert eng.last_prepare_mode == 4
    finally:
        eng.close()
