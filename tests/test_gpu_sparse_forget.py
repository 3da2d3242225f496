"""Tier 2 (GPU): gpmpc_sparse_forget -- memory points leaving a sparse GP in O(M^2).

Accuracy: build on the whole memory of a case, forget some rows by their values, and compare gpmpc_predict with the longdouble
from-scratch restatement of the REDUCED memory (tests/sparse_forget_ref.py) by
    tolerance = 10 max(e_scratch, e_rec) + 64 eps scale      (e_scratch: the from-scratch float64 restatement's own error on the
                                                              reduced memory; e_rec: the float64 numpy recurrence's; both from
                                                              numpy alone, never taken from the GPU)
and the contracts of include/gpmpc.h: exact symmetry, the state being that of gpmpc_set_factors, k points in one call = k calls,
determinism, forgets and appends chaining, the state rules (mode 6, the record refreshed by gpmpc_prepare_sparse and dropped by
gpmpc_prepare and gpmpc_set_factors), argument errors that leave everything untouched, the lost pivot of a point that never was
in the model (GPMPC_ERR_NOT_PD, no model afterwards), and the model-level option ModelConfig.inducing_forget."""
import numpy as np
import pytest
import torch

import sparse_append_ref as ar
import sparse_forget_ref as fr
import sparse_gp_ref as ref
from helpers import record

pytestmark = pytest.mark.gpu

# M = 1 (2 -> 1 points); M = 16 oldest and scattered rows; M = 64 with the time input; M = 70 (two column tiles, 64 points);
# M = 130 (three column tiles, the last partial); fewer points than inducing inputs; D = 1; D = 16 with E = 20
ACCURACY_CASES = ["m1-1", "n37_m16-8", "n37_m16-scattered", "n257_m64_time-9", "n257_m70-64", "n150_m130-10", "n20_m37-8", "d1-8",
                  "d16_e20-8"]


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


def _build(eng, c, rows=None):
    rows = slice(None) if rows is None else rows
    eng.prepare_sparse(c.X[rows], c.Y[rows], c.Z, c.ls, c.os, c.nz, ref.JITTER_REL)


def _build_and_forget(eng, c, one_by_one=False):
    _build(eng, c)
    if one_by_one:
        for q in c.gone:
            eng.sparse_forget(c.X[q:q + 1], c.Y[q:q + 1])
    else:
        eng.sparse_forget(c.X[c.gone], c.Y[c.gone])


def _state(eng, c):
    iK, beta = eng.factors()
    out = eng.predict(c.Xq)
    return _np(iK), _np(beta), _np(out["mean"]), _np(out["var"])


def _within_tolerance(eng, c, label):
    out = eng.predict(c.Xq)
    e_mean = float(np.max(np.abs(_np(out["mean"]) - c.mean_ld)))
    e_var = float(np.max(np.abs(_np(out["var"]) - c.var_ld)))
    print(f"{label}: GPU mean {e_mean:.3e} (tol {c.tol_mean:.3e}; numpy from scratch {c.e64_mean:.3e}, numpy recurrence "
          f"{c.erec_mean:.3e})  var {e_var:.3e} (tol {c.tol_var:.3e}; numpy from scratch {c.e64_var:.3e}, numpy recurrence "
          f"{c.erec_var:.3e})")
    record(f"sparse_forget[{label}]", mean=e_mean, var=e_var, numpy_mean=c.e64_mean, numpy_var=c.e64_var,
           numpy_recurrence_mean=c.erec_mean, numpy_recurrence_var=c.erec_var)
    assert e_mean <= c.tol_mean
    assert e_var <= c.tol_var


# -- 1. accuracy, symmetry, shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ACCURACY_CASES)
def test_accuracy_against_longdouble_build_of_the_reduced_memory(engine, name):
    c = fr.case(name)
    _build_and_forget(engine, c)
    assert engine.last_prepare_mode == 6 and engine.N == c.M
    _within_tolerance(engine, c, name)
    iK, beta = engine.factors()
    assert tuple(iK.shape) == (c.D, c.M, c.M) and tuple(beta.shape) == (c.D, c.M)
    iK = _np(iK)
    assert np.all(np.isfinite(iK)) and np.all(np.isfinite(_np(beta)))
    assert _same_bits(iK, np.ascontiguousarray(np.swapaxes(iK, 1, 2)))             # iK_eff[a,i,j] == iK_eff[a,j,i]


def test_sliding_window_of_appends_and_forgets(engine):
    c = fr.sliding_window()
    _build(engine, c, slice(0, c.n0))
    for s in range(c.steps):
        engine.sparse_append(c.X[c.n0 + s:c.n0 + s + 1], c.Y[c.n0 + s:c.n0 + s + 1])
        assert engine.last_prepare_mode == 5
        engine.sparse_forget(c.X[s:s + 1], c.Y[s:s + 1])
        assert engine.last_prepare_mode == 6
    _within_tolerance(engine, c, c.name)


# -- 2. bits -------------------------------------------------------------------------------------------------------------------------
def test_k_points_in_one_call_are_k_calls_and_two_runs_agree(engine):
    c = fr.case("n37_m16-scattered")                                  # 8 rows
    _build_and_forget(engine, c)
    first = _state(engine, c)
    _build_and_forget(engine, c)
    second = _state(engine, c)
    _build_and_forget(engine, c, one_by_one=True)
    single = _state(engine, c)
    assert engine.last_prepare_mode == 6
    for a, b, s in zip(first, second, single):
        assert _same_bits(a, b)
        assert _same_bits(a, s)


def test_state_equals_set_factors(engine):
    c = fr.case("n257_m70-64")
    D, A, B, H = c.D, 1, 2, 3
    rng = np.random.default_rng(7)
    actions = rng.uniform(0.1, 0.9, size=(B, H, A))
    mu0 = rng.uniform(0.3, 0.7, size=D)
    S0 = np.diag(rng.uniform(1e-3, 3e-3, size=D))

    def run(eng):
        eng.set_cost(np.full(D + A, 0.5), np.eye(D + A), np.eye(D), 1.0)
        p = eng.predict(c.Xq)
        r = eng.rollout(actions, mu0, S0)
        return [_np(p[k]) for k in ("mean", "var")] + [_np(r[k]) for k in ("J", "mu", "Sig")]

    _build_and_forget(engine, c)
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


# -- 3. state rules ------------------------------------------------------------------------------------------------------------------
def test_prepare_sparse_refreshes_the_record():
    """forget; gpmpc_prepare_sparse of the whole memory again; the same forget: the first bits again (nothing of the earlier
    removals survives in the record), which are also those of a fresh handle."""
    c = fr.case("n37_m16-8")
    eng, fresh = _fresh(), _fresh()
    try:
        _build_and_forget(eng, c)
        first = _state(eng, c)
        _build_and_forget(eng, c)
        _build_and_forget(fresh, c)
        for a, b, f in zip(first, _state(eng, c), _state(fresh, c)):
            assert _same_bits(a, b)
            assert _same_bits(a, f)
    finally:
        eng.close()
        fresh.close()


def test_state_rules():
    import gp_mpc_amd
    from gp_mpc_amd import _lib
    c = fr.case("n37_m16-8")
    eng = _fresh()
    try:
        _build_and_forget(eng, c)
        assert eng.last_prepare_mode == 6 and eng.N == c.M
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:              # no (X, Y) record: the index form is still refused
            eng.forget([3])
        assert ei.value.code == _lib.GPMPC_ERR_ARG
        _within_tolerance(eng, c, "after a refused index forget")
        # gpmpc_prepare drops the record: a sparse forget is an argument error and the exact model keeps its bits
        eng.prepare(c.X, c.Y, c.ls, c.os, c.nz)
        assert eng.last_prepare_mode == 0
        before = _state(eng, c)
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:
            eng.sparse_forget(c.X[:1], c.Y[:1])
        assert ei.value.code == _lib.GPMPC_ERR_ARG and eng.last_prepare_mode == 0
        for a, b in zip(before, _state(eng, c)):
            assert _same_bits(a, b)
        # ... and so does gpmpc_set_factors
        _build(eng, c)
        iK, beta = eng.factors()
        eng.set_factors(c.Z, iK, beta, c.ls, c.os)
        before = _state(eng, c)
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:
            eng.sparse_forget(c.X[c.gone], c.Y[c.gone])
        assert ei.value.code == _lib.GPMPC_ERR_ARG
        for a, b in zip(before, _state(eng, c)):
            assert _same_bits(a, b)
    finally:
        eng.close()


# -- 4. errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_model_and_record_untouched():
    from gp_mpc_amd import _lib
    c = fr.case("n37_m16-8")
    eng = _fresh()
    try:
        _build(eng, c)
        before = _state(eng, c)
        Xo, Yo = eng._dev(c.X[c.gone]), eng._dev(c.Y[c.gone])
        k, D, E = len(c.gone), c.D, c.E
        st = eng._stream()

        def call(X=Xo.data_ptr(), Y=Yo.data_ptr(), k=k, D=D, E=E):
            return eng.lib.gpmpc_sparse_forget(eng._h, X, Y, k, D, E, st)

        for kw in (dict(X=None), dict(Y=None), dict(k=0), dict(k=-2), dict(D=D + 1), dict(D=D - 1), dict(E=E + 1), dict(E=E - 1)):
            assert call(**kw) == _lib.GPMPC_ERR_ARG, kw
            assert eng.last_prepare_mode == 4
            for a, b in zip(before, _state(eng, c)):
                assert _same_bits(a, b), kw
        assert eng.lib.gpmpc_sparse_forget(None, Xo.data_ptr(), Yo.data_ptr(), k, D, E, st) == _lib.GPMPC_ERR_ARG
        assert call() == _lib.GPMPC_OK and eng.last_prepare_mode == 6          # the record is intact: a valid forget still works
        _within_tolerance(eng, c, "after argument errors")
        empty = _fresh()                                                   # no model at all
        try:
            assert empty.lib.gpmpc_sparse_forget(empty._h, Xo.data_ptr(), Yo.data_ptr(), k, D, E, st) == _lib.GPMPC_ERR_ARG
        finally:
            empty.close()
    finally:
        eng.close()


def test_a_point_that_never_was_in_the_model_loses_the_pivot():
    """The m1 construction of tests/test_sparse_forget_reference.py (p^T p = 3.2, 2.2, 1.8): an error code from a completed call,
    after which the handle holds no model."""
    import gp_mpc_amd
    from gp_mpc_amd import _lib
    m1, built_on, gone = fr.lost_pivot_setup()
    eng = _fresh()
    try:
        eng.prepare_sparse(m1.X[built_on], m1.Y[built_on], m1.Z, m1.ls, m1.os, m1.nz, ref.JITTER_REL)
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:
            eng.sparse_forget(m1.X[gone], m1.Y[gone])
        assert ei.value.code == _lib.GPMPC_ERR_NOT_PD
        assert "point 0" in str(ei.value) and "output 0" in str(ei.value)
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:              # no model
            eng.predict(m1.Xq)
        assert ei.value.code == _lib.GPMPC_ERR_ARG
        with pytest.raises(gp_mpc_amd.GpmpcError) as ei:              # ... and no record
            eng.sparse_append(m1.X[gone], m1.Y[gone])
        assert ei.value.code == _lib.GPMPC_ERR_ARG
        c = fr.case("m1-1")                                               # the handle is usable again after a prepare
        _build_and_forget(eng, c)
        _within_tolerance(eng, c, "after a lost pivot")
    finally:
        eng.close()


# -- 5. model level ------------------------------------------------------------------------------------------------------------------
def test_model_level_forget_then_append():
    from gp_mpc_amd import GpStateTransitionModel
    from gp_mpc_amd.config_classes.model_config import ModelConfig
    c = ref.case("n37_m16")
    gp_init = {"noise_covar.noise": list(c.nz), "base_kernel.lengthscale": c.ls.tolist(), "outputscale": list(c.os)}
    eng = _fresh()
    try:
        cfg = ModelConfig(gp_init=gp_init, num_inducing_points=16, inducing_refresh_every=8, inducing_forget=True)
        model = GpStateTransitionModel(cfg, dim_state=3, dim_action=1, engine=eng)
        X, Y = torch.as_tensor(c.X), torch.as_tensor(c.Y)
        modes = []
        model.prepare_inference(X[:35], Y[:35])
        modes.append(eng.last_prepare_mode)
        Z = c.X[np.asarray(model.inducing_idx, dtype=np.int64)]
        model.forget([0, 1])
        modes.append(eng.last_prepare_mode)
        assert len(model.x_mem) == 33 and model.inducing_idx[0] == -1 and model.inducing_idx[-1] == 32
        model.prepare_inference(X[2:37], Y[2:37])
        modes.append(eng.last_prepare_mode)
        assert modes == [4, 6, 5] and model.is_sparse and len(model.x_mem) == 35 and eng.N == 16
        # the same Z, from scratch on rows 2..36; the tolerance from the numpy recurrence of the same three calls
        w = fr.Case()
        w.Z, w.ls, w.os, w.nz, w.Xq, w.X, w.Y = Z, c.ls, c.os, c.nz, c.Xq, c.X, c.Y
        r = ar.build_record(c.X[:35], c.Y[:35], Z, c.ls, c.os, c.nz, ref.JITTER_REL)
        fr.forget(r, c.X[:2], c.Y[:2])
        ar.append(r, c.X[35:], c.Y[35:])
        fr.tolerance(w, *fr.reference(w, np.arange(2, 37)), *fr.predict(w, r))
        _within_tolerance(eng, w, "model level: prepare, forget 2, append 2")
    finally:
        eng.close()
