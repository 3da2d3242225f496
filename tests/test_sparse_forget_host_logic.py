"""CPU tests of the host side of ModelConfig.inducing_forget: the sequence of engine calls GpStateTransitionModel.forget and
prepare_inference make -- when rows leave the sparse model through gpmpc_sparse_forget, when the forget is refused so that the
caller rebuilds, and what happens to x_mem / y_mem, `inducing_idx` and the count of changed rows.  No GPU: the engine is the
stand-in of tests/sparse_forget_stub_engine.py."""
import numpy as np
import pytest
import torch

from helpers import make_controller
from oracle import synth
from sparse_forget_stub_engine import SparseForgetStubEngine

M = 7


def _model(w, **model_kw):
    from gp_mpc_amd import GpStateTransitionModel
    from gp_mpc_amd.config_classes import ModelConfig
    N, D, A, E, H, B = w.dims
    cfg = ModelConfig(gp_init={"noise_covar.noise": list(w.noises), "base_kernel.lengthscale": w.lengthscales.tolist(),
                               "outputscale": list(w.outputscales)}, **model_kw)
    eng = SparseForgetStubEngine()
    return GpStateTransitionModel(cfg, dim_state=D, dim_action=A, engine=eng), eng


def _rows(N, m):
    return [0] if m == 1 else [int(round(i * (N - 1) / (m - 1))) for i in range(m)]


def _prep(m, X, Y):
    m.prepare_inference(torch.as_tensor(X), torch.as_tensor(Y))


def _kinds(eng):
    return [k[0] for k in eng.log]


def _refused(m, idx):
    from gp_mpc_amd import GpmpcError, _lib
    with pytest.raises(GpmpcError) as ei:
        m.forget(idx)
    assert ei.value.code == _lib.GPMPC_ERR_ARG
    return ei.value


@pytest.fixture(scope="module")
def w():
    return synth.make_workload(N=23, D=2, A=1, H=3, B=1, seed=4)


def test_config_validates_and_defaults_to_refusing():
    from gp_mpc_amd.config_classes import ModelConfig
    assert ModelConfig().inducing_forget is False
    assert ModelConfig(num_inducing_points=5, inducing_refresh_every=4, inducing_forget=True).inducing_forget is True
    for bad in (0, 1, None, "yes", 1.0):
        with pytest.raises(ValueError):
            ModelConfig(inducing_forget=bad)


@pytest.mark.parametrize("kw", [dict(num_inducing_points=M), dict(num_inducing_points=M, inducing_refresh_every=8),
                                dict(num_inducing_points=M, inducing_forget=True),
                                dict(num_inducing_points=M, inducing_refresh_every=8, inducing_forget=False)])
def test_without_both_options_forget_is_refused_as_before(w, kw):
    """The option off, or on without a refresh interval -- and a config object from before the option existed."""
    m, eng = _model(w, **kw)
    legacy, eng2 = _model(w, **kw)
    del legacy.config.inducing_forget
    for mm, ee in ((m, eng), (legacy, eng2)):
        _prep(mm, w.X[:14], w.Y[:14])
        assert "sparse" in str(_refused(mm, [0, 3]))
        assert _kinds(ee) == ["prepare_sparse"] and len(mm.x_mem) == 14 and mm.is_sparse


def test_forget_hands_the_rows_values_to_the_engine_and_shrinks_the_memory(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8, inducing_forget=True)
    _prep(m, w.X[:14], w.Y[:14])
    m.forget([0, 3, 13])
    assert _kinds(eng) == ["prepare_sparse", "sparse_forget"] and eng.last_prepare_mode == 6
    assert np.array_equal(eng.log[1][1], w.X[[0, 3, 13]]) and np.array_equal(eng.log[1][2], w.Y[[0, 3, 13]])
    keep = np.setdiff1d(np.arange(14), [0, 3, 13])
    assert np.array_equal(np.asarray(m.x_mem), w.X[keep]) and np.array_equal(np.asarray(m.y_mem), w.Y[keep]) and m.is_sparse
    st = m.save_state()
    assert np.array_equal(np.asarray(st.inputs), w.X[keep]) and "inducing_forget" not in st.constraints_hyperparams
    # the reduced memory followed by new rows appends; the same memory again makes no call
    _prep(m, np.concatenate([w.X[keep], w.X[14:16]]), np.concatenate([w.Y[keep], w.Y[14:16]]))
    assert _kinds(eng) == ["prepare_sparse", "sparse_forget", "sparse_append"] and np.array_equal(eng.log[2][1], w.X[14:16])
    _prep(m, np.concatenate([w.X[keep], w.X[14:16]]), np.concatenate([w.Y[keep], w.Y[14:16]]))
    assert len(eng.log) == 3


def test_the_count_is_shared_with_the_appends_and_past_it_the_forget_is_refused(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=4, inducing_forget=True)
    _prep(m, w.X[:14], w.Y[:14])
    _prep(m, w.X[:16], w.Y[:16])                                      # 2 appended
    m.forget([0])                                                     # 3 changed
    m.forget([0])                                                     # 4 changed
    assert _kinds(eng) == ["prepare_sparse", "sparse_append", "sparse_forget", "sparse_forget"]
    assert np.array_equal(eng.log[3][1], w.X[1:2])                     # the second forget's row 0 is the first memory's row 1
    _refused(m, [0])                                                   # 5 > 4: no call, nothing changes
    assert len(eng.log) == 4 and np.array_equal(np.asarray(m.x_mem), w.X[2:16])
    _prep(m, w.X[2:17], w.Y[2:17])                                    # an append past the count rebuilds, on fresh rows ...
    assert _kinds(eng)[-1] == "prepare_sparse" and np.array_equal(eng.log[-1][1], w.X[2:17]) and m.inducing_idx == _rows(15, M)
    m.forget([0, 1, 2])                                                # ... and the count starts again
    assert _kinds(eng)[-1] == "sparse_forget" and len(m.x_mem) == 12
    m2, eng2 = _model(w, num_inducing_points=M, inducing_refresh_every=4, inducing_forget=True)
    _prep(m2, w.X[:14], w.Y[:14])
    m2.forget([0, 1, 2])
    _refused(m2, [0, 1])                                               # 3 + 2 > 4: refused as a whole
    assert _kinds(eng2) == ["prepare_sparse", "sparse_forget"] and len(m2.x_mem) == 11
    _prep(m2, w.X[3:15], w.Y[3:15])                                   # forgotten rows count for the appends too: 3 + 1 <= 4
    assert _kinds(eng2)[-1] == "sparse_append"
    _prep(m2, w.X[3:16], w.Y[3:16])                                   # 5 > 4
    assert _kinds(eng2)[-1] == "prepare_sparse"


def test_bad_indices_are_refused_without_a_call(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=16, inducing_forget=True)
    _prep(m, w.X[:10], w.Y[:10])
    for bad in ([], [3, 3], [4, 2], [-1], [10], list(range(10))):      # k < 1, repeated, unsorted, out of range, k = rows
        _refused(m, bad)
    with pytest.raises(TypeError):
        m.forget([1.5])
    assert _kinds(eng) == ["prepare_sparse"] and len(m.x_mem) == 10
    m.forget(list(range(9)))                                           # k < rows is the only bound
    assert _kinds(eng)[-1] == "sparse_forget" and len(m.x_mem) == 1


def test_inducing_idx_is_renumbered_list_kind(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8, inducing_forget=True)
    _prep(m, w.X[:14], w.Y[:14])
    assert m.inducing_idx == [0, 2, 4, 6, 9, 11, 13]
    m.forget([0, 3, 4])
    assert isinstance(m.inducing_idx, list) and m.inducing_idx == [-1, 1, -1, 3, 6, 8, 10]
    assert all(isinstance(v, int) for v in m.inducing_idx)
    m.forget([1, 10])                                                  # a departed entry stays -1
    assert m.inducing_idx == [-1, -1, -1, 2, 5, 7, -1]
    x = np.asarray(m.x_mem)
    for z, i in zip(eng.log[0][2], m.inducing_idx):                    # the live entries still name their inducing inputs
        assert i < 0 or np.array_equal(x[i], z)


def test_inducing_idx_is_renumbered_tensor_kind(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8, inducing_forget=True)
    _prep(m, w.X[:14], w.Y[:14])
    m.inducing_idx = torch.tensor([0, 13, 7, 3, 5, 9, 12], dtype=torch.int32)      # the kind the greedy selection leaves, unsorted
    m.forget([0, 3, 4])
    assert isinstance(m.inducing_idx, torch.Tensor) and m.inducing_idx.dtype == torch.int32
    assert m.inducing_idx.tolist() == [-1, 10, 4, -1, 2, 6, 9]
    m.forget([2])
    assert m.inducing_idx.tolist() == [-1, 9, 3, -1, -1, 5, 8]


def test_changed_hyper_parameters_refuse_the_forget(w):
    for key, val in (("covar_module.outputscale", np.array(0.3)), ("likelihood.noise", np.array([2e-3])),
                     ("covar_module.base_kernel.lengthscale", np.full((1, w.X.shape[1]), 1.7))):
        m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8, inducing_forget=True)
        _prep(m, w.X[:14], w.Y[:14])
        m.models[1].initialize(**{key: val})
        _refused(m, [0])
        assert _kinds(eng) == ["prepare_sparse"] and len(m.x_mem) == 14, key
        _prep(m, w.X[1:14], w.Y[1:14])                                 # the caller's prepare rebuilds under the new ones ...
        assert _kinds(eng) == ["prepare_sparse", "prepare_sparse"]
        m.forget([0])                                                  # ... after which rows can leave again
        assert _kinds(eng)[-1] == "sparse_forget"


def test_other_models_are_not_touched_by_the_option(w):
    Z = torch.as_tensor(w.X[[0, 5, 9]])
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8, inducing_forget=True)
    m.prepare_inference(torch.as_tensor(w.X[:14]), torch.as_tensor(w.Y[:14]), inducing_inputs=Z)
    _refused(m, [0])                                                   # explicit inducing inputs: not the config's choice
    assert _kinds(eng) == ["prepare_sparse"]
    _prep(m, w.X[:5], w.Y[:5])                                        # no more than M points: the exact model forgets by index
    m.forget([1])
    assert _kinds(eng)[-2:] == ["prepare", "forget"] and len(m.x_mem) == 4


def test_a_lost_pivot_rebuilds_and_the_caller_sees_a_successful_forget(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8, inducing_forget=True)
    _prep(m, w.X[:14], w.Y[:14])
    eng.lose_pivot = True
    m.forget([0, 2])
    keep = np.setdiff1d(np.arange(14), [0, 2])
    assert _kinds(eng) == ["prepare_sparse", "sparse_forget", "prepare_sparse"]
    assert np.array_equal(eng.log[2][1], w.X[keep]) and np.array_equal(eng.log[2][2], w.X[keep][_rows(12, M)])
    assert np.array_equal(np.asarray(m.x_mem), w.X[keep]) and np.array_equal(np.asarray(m.y_mem), w.Y[keep])
    assert m.inducing_idx == _rows(12, M) and m.is_sparse and eng.last_prepare_mode == 4
    eng.lose_pivot = False
    m.forget([0])                                                      # a fresh record and a fresh count
    assert _kinds(eng)[-1] == "sparse_forget" and len(m.x_mem) == 11


def test_an_engine_without_a_record_re_raises_and_the_memory_stays(w):
    m, eng = _model(w, num_inducing_points=M, inducing_refresh_every=8, inducing_forget=True)
    _prep(m, w.X[:14], w.Y[:14])
    idx = list(m.inducing_idx)
    eng.refuse_forget = True                                           # e.g. the shared engine was given other factors meanwhile
    _refused(m, [0])
    assert _kinds(eng) == ["prepare_sparse", "sparse_forget"] and len(m.x_mem) == 14 and m.inducing_idx == idx


def test_capped_memory_loop_is_forget_plus_append():
    """MemoryConfig.max_points_model with both options: after the first step every control step is a forget of the evicted row
    and an append of the new one -- no rebuild from the window."""
    N, steps = 12, 5
    w = synth.make_workload(N=N, D=2, A=1, H=3, B=1, seed=6)
    eng = SparseForgetStubEngine()
    c = make_controller(w, engine=eng, shard=False)
    c.memory.config.max_points_model = N
    c.memory.config.check_errors_for_storage = False
    cfg = c.transition_model.config
    cfg.num_inducing_points, cfg.inducing_refresh_every, cfg.inducing_forget = 5, 32, True
    np.random.seed(0)
    rng = np.random.default_rng(1)
    obs = w.mu0.copy()
    windows = []
    for s in range(steps):
        a = c.get_action(obs)
        windows.append(c.memory.get()[0].numpy().copy())
        assert len(windows[-1]) == N and np.array_equal(np.asarray(c.transition_model.x_mem), windows[-1])
        nxt = np.clip(obs + 0.05 * rng.standard_normal(obs.shape), 0.05, 0.95)
        c.add_memory(obs, a, nxt, 0.0)
        obs = nxt
    assert _kinds(eng) == ["prepare_sparse"] + ["sparse_forget", "sparse_append"] * (steps - 1), _kinds(eng)
    for s in range(1, steps):
        gone, new = eng.log[2 * s - 1], eng.log[2 * s]
        assert np.array_equal(gone[1], windows[s - 1][:1]) and np.array_equal(new[1], windows[s][-1:])
    assert c.transition_model._sparse_record["changed"] == 2 * (steps - 1)
