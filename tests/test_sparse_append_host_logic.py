"""CPU tests of the host side of ModelConfig.inducing_refresh_every: the sequence of engine calls prepare_inference makes -- when
it appends (gpmpc_sparse_append) and when it rebuilds (select or stride, then gpmpc_prepare_sparse).  No GPU: the engine is the
stand-in of tests/sparse_append_stub_engine.py."""
import numpy as np
import pytest
import torch

from oracle import synth
from sparse_append_stub_engine import SparseAppendStubEngine

M = 7


def _model(w, **model_kw):
    from gp_mpc_amd import GpStateTransitionModel
    from gp_mpc_amd.config_classes import ModelConfig
    N, D, A, E, H, B = w.dims
    cfg = ModelConfig(gp_init={"noise_covar.noise": list(w.noises), "base_kernel.lengthscale": w.lengthscales.tolist(),
                               "outputscale": list(w.outputscales)}, **model_kw)
    eng = SparseAppendStubEngine()
    return GpStateTransitionModel(cfg, dim_state=D, dim_action=A, engine=eng), eng


def _rows(N, m):
    return [0] if m == 1 else [int(round(i * (N - 1) / (m - 1))) for i in range(m)]


def _prep(m, w, n, **kw):
    m.prepare_inference(torch.as_tensor(w.X[:n]), torch.as_tensor(w.Y[:n]), **kw)


def _kinds(eng):
    return [k[0] for k in eng.log]


@pytest.fixture(scope="module")
def w():
    return synth.make_workload(N=23, D=2, A=1, H=3, B=1, seed=4)


def test_config_validates_and_defaults_to_rebuilding():
    from gp_mpc_amd.config_classes import ModelConfig
    assert ModelConfig().inducing_refresh_every is None
    assert ModelConfig(inducing_refresh_every=1).inducing_refresh_every == 1
    assert ModelConfig(num_inducing_points=5, inducing_refresh_every=32.0).inducing_refresh_every == 32
    for bad in (0, -3, 2.5, True, False):
        with pytest.raises(ValueError):
            ModelConfig(inducing_refresh_every=bad)


def test_first_prepare_then_appends_of_one_and_of_several_rows(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8)
    _prep(m, w, 12)
    (kind, X, Z, jitter), = eng.log
    assert kind == "prepare_sparse" and np.array_equal(X, w.X[:12]) and np.array_equal(Z, w.X[_rows(12, M)])
    idx = list(m.inducing_idx)
    _prep(m, w, 13)                                                   # one row
    assert _kinds(eng) == ["prepare_sparse", "sparse_append"]
    assert np.array_equal(eng.log[1][1], w.X[12:13]) and np.array_equal(eng.log[1][2], w.Y[12:13])
    _prep(m, w, 17)                                                   # several rows in one call
    assert _kinds(eng) == ["prepare_sparse", "sparse_append", "sparse_append"]
    assert np.array_equal(eng.log[2][1], w.X[13:17]) and np.array_equal(eng.log[2][2], w.Y[13:17])
    # the inducing rows are kept, the memory the model reports is the whole one, and that is what training is shipped
    assert list(m.inducing_idx) == idx and m.is_sparse and eng.last_prepare_mode == 5
    assert np.array_equal(np.asarray(m.x_mem), w.X[:17]) and np.array_equal(np.asarray(m.y_mem), w.Y[:17])
    st = m.save_state()
    assert np.array_equal(np.asarray(st.inputs), w.X[:17]) and "inducing_refresh_every" not in st.constraints_hyperparams


def test_unchanged_memory_makes_no_call(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8)
    _prep(m, w, 12)
    _prep(m, w, 12)
    assert _kinds(eng) == ["prepare_sparse"]
    _prep(m, w, 13)
    _prep(m, w, 13)
    assert _kinds(eng) == ["prepare_sparse", "sparse_append"]


def test_the_refresh_boundary(w):
    """R = 3: three appended rows ride on the model, the fourth rebuilds it on freshly chosen rows and restarts the count; a single
    call that would cross the boundary rebuilds as a whole."""
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=3)
    for n in range(12, 20):
        _prep(m, w, n)
    assert _kinds(eng) == ["prepare_sparse"] + ["sparse_append"] * 3 + ["prepare_sparse"] + ["sparse_append"] * 3
    assert np.array_equal(eng.log[4][1], w.X[:16]) and np.array_equal(eng.log[4][2], w.X[_rows(16, M)])
    assert m.inducing_idx == _rows(16, M)
    m2, eng2 = _model(w, num_inducing_points=M, inducing_refresh_every=3)
    _prep(m2, w, 12)
    _prep(m2, w, 14)                                                  # 2 appended
    _prep(m2, w, 16)                                                  # 2 + 2 > 3
    assert _kinds(eng2) == ["prepare_sparse", "sparse_append", "prepare_sparse"]
    assert np.array_equal(eng2.log[2][1], w.X[:16])
    _prep(m2, w, 19)                                                  # the count starts again: 3 <= 3
    assert _kinds(eng2)[-1] == "sparse_append" and np.array_equal(eng2.log[-1][1], w.X[16:19])


def test_a_hyper_parameter_change_rebuilds(w):
    for key, val in (("covar_module.outputscale", np.array(0.3)), ("likelihood.noise", np.array([2e-3])),
                     ("covar_module.base_kernel.lengthscale", np.full((1, w.X.shape[1]), 1.7))):
        m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8)
        _prep(m, w, 12)
        _prep(m, w, 13)
        m.models[1].initialize(**{key: val})
        _prep(m, w, 14)
        assert _kinds(eng) == ["prepare_sparse", "sparse_append", "prepare_sparse"], key
        assert np.array_equal(eng.log[2][1], w.X[:14])
        _prep(m, w, 15)                                               # ... and appends ride on the new hyper-parameters
        assert _kinds(eng)[-1] == "sparse_append"
        m.models[1].initialize(**{key: val})                          # the same values again are no change
        _prep(m, w, 16)
        assert _kinds(eng)[-1] == "sparse_append"
        m.models[0].initialize(**{key: val})
        _prep(m, w, 16)                                               # an unchanged memory under new hyper-parameters rebuilds too
        assert _kinds(eng)[-1] == "prepare_sparse" and len(eng.log) == 6


def test_a_changed_earlier_row_rebuilds(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8)
    _prep(m, w, 12)
    X, Y = w.X[:13].copy(), w.Y[:13].copy()
    X[4, 0] += 1e-9                                                   # same counts, other values: compared by value
    m.prepare_inference(torch.as_tensor(X), torch.as_tensor(Y))
    assert _kinds(eng) == ["prepare_sparse", "prepare_sparse"] and np.array_equal(eng.log[1][1], X)
    Y2 = Y.copy()
    Y2[0, 1] -= 1e-9
    m.prepare_inference(torch.as_tensor(np.concatenate([X, w.X[13:14]])), torch.as_tensor(np.concatenate([Y2, w.Y[13:14]])))
    assert _kinds(eng)[-1] == "prepare_sparse" and len(eng.log) == 3


def test_a_shrunk_or_shifted_memory_rebuilds(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8)
    _prep(m, w, 14)
    _prep(m, w, 12)                                                   # shrunk
    assert _kinds(eng) == ["prepare_sparse", "prepare_sparse"] and np.array_equal(eng.log[1][1], w.X[:12])
    m.prepare_inference(torch.as_tensor(w.X[1:14]), torch.as_tensor(w.Y[1:14]))     # a capped window: oldest row out, one in
    assert _kinds(eng)[-1] == "prepare_sparse" and np.array_equal(eng.log[2][1], w.X[1:14])
    _prep(m, w, 5)                                                    # no more than M points: the exact model
    assert _kinds(eng)[-1] == "prepare" and not m.is_sparse
    _prep(m, w, 12)                                                   # growing out of it is a rebuild, not an append
    assert _kinds(eng)[-1] == "prepare_sparse"


def test_explicit_inducing_inputs_never_append(w):
    Z = torch.as_tensor(w.X[[0, 5, 9]])
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8)
    _prep(m, w, 12, inducing_inputs=Z)
    _prep(m, w, 13, inducing_inputs=Z)                                # explicit again: rebuilt on them
    assert _kinds(eng) == ["prepare_sparse", "prepare_sparse"] and np.array_equal(eng.log[1][2], Z.numpy())
    _prep(m, w, 14)                                                   # the config's choice after an explicit one: a rebuild
    assert _kinds(eng)[-1] == "prepare_sparse" and np.array_equal(eng.log[2][2], w.X[_rows(14, M)])
    _prep(m, w, 15)
    assert _kinds(eng)[-1] == "sparse_append"
    _prep(m, w, 16, inducing_inputs=Z)                                # explicit after the config's: a rebuild on Z
    assert _kinds(eng)[-1] == "prepare_sparse" and np.array_equal(eng.log[-1][2], Z.numpy())
    _prep(m, w, 17)
    assert _kinds(eng)[-1] == "prepare_sparse"


def test_an_engine_without_a_record_falls_back_to_the_rebuild(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8)
    _prep(m, w, 12)
    eng.refuse_append = True                                          # e.g. the shared engine was given other factors meanwhile
    _prep(m, w, 13)
    assert _kinds(eng) == ["prepare_sparse", "sparse_append", "prepare_sparse"]
    assert np.array_equal(eng.log[2][1], w.X[:13]) and np.array_equal(np.asarray(m.x_mem), w.X[:13])
    eng.refuse_append = False
    _prep(m, w, 14)
    assert _kinds(eng)[-1] == "sparse_append" and np.array_equal(eng.log[-1][1], w.X[13:14])


@pytest.mark.parametrize("kw", [dict(), dict(num_inducing_points=M), dict(num_inducing_points=M, inducing_selection="strided")])
def test_refresh_none_is_todays_sequence_call_for_call(w, kw):
    """Without the option every prepare_inference makes exactly the call it made before the option existed -- also for a config
    object from before it existed."""
    m, eng = _model(w, **kw)
    legacy, eng2 = _model(w, **kw)
    del legacy.config.inducing_refresh_every
    want = "prepare_sparse" if kw else "prepare"
    for mm, ee in ((m, eng), (legacy, eng2)):
        for n in (12, 13, 13, 17, 12):
            _prep(mm, w, n)
        assert _kinds(ee) == [want] * 5
        assert [len(k[1]) for k in ee.log] == [12, 13, 13, 17, 12]
        assert "sparse_append" not in _kinds(ee)


def test_forget_on_an_appended_model_is_still_refused(w):
    from gp_mpc_amd import GpmpcError, _lib
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8)
    _prep(m, w, 12)
    _prep(m, w, 13)
    with pytest.raises(GpmpcError) as ei:
        m.forget([0])
    assert ei.value.code == _lib.GPMPC_ERR_ARG and len(m.x_mem) == 13 and _kinds(eng) == ["prepare_sparse", "sparse_append"]
