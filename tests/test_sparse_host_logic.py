"""CPU tests of the host side of the sparse model option (ModelConfig.num_inducing_points, prepare_inference's
`inducing_inputs`): which engine call the model makes and with which inducing inputs, the full memory it keeps, its `forget`
rule, and a capped memory together with the option.  No GPU: the engine is the stand-in of tests/sparse_stub_engine.py."""
import numpy as np
import pytest
import torch

from helpers import make_controller
from oracle import synth
from sparse_stub_engine import SparseStubEngine


def _model(w, **model_kw):
    from gp_mpc_amd import GpStateTransitionModel
    from gp_mpc_amd.config_classes import ModelConfig
    N, D, A, E, H, B = w.dims
    cfg = ModelConfig(gp_init={"noise_covar.noise": list(w.noises), "base_kernel.lengthscale": w.lengthscales.tolist(),
                               "outputscale": list(w.outputscales)}, **model_kw)
    eng = SparseStubEngine()
    return GpStateTransitionModel(cfg, dim_state=D, dim_action=A, engine=eng), eng


def _documented_rows(N, M):
    return [0] if M == 1 else [int(round(i * (N - 1) / (M - 1))) for i in range(M)]


@pytest.fixture(scope="module")
def w():
    return synth.make_workload(N=23, D=2, A=1, H=3, B=1, seed=4)


def test_config_validates_and_defaults_to_the_exact_model():
    from gp_mpc_amd.config_classes import ModelConfig
    c = ModelConfig()
    assert c.num_inducing_points is None and c.inducing_jitter == 1e-6
    assert ModelConfig(num_inducing_points=7, inducing_jitter=0.0).num_inducing_points == 7
    for bad in (0, -2, 2.5, True):
        with pytest.raises(ValueError):
            ModelConfig(num_inducing_points=bad)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ModelConfig(inducing_jitter=bad)


def test_default_config_never_calls_prepare_sparse(w):
    m, eng = _model(w)
    m.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    assert [k[0] for k in eng.log] == ["prepare"] and not m.is_sparse
    legacy, eng2 = _model(w)                      # a config object from before the option existed
    del legacy.config.num_inducing_points, legacy.config.inducing_jitter
    legacy.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    assert [k[0] for k in eng2.log] == ["prepare"]


@pytest.mark.parametrize("M", [1, 2, 7, 22])
def test_strided_selection_picks_the_documented_rows(w, M):
    m, eng = _model(w, num_inducing_points=M, inducing_jitter=3e-7)
    m.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    (kind, X, Z, jitter), = eng.log
    assert kind == "prepare_sparse" and m.is_sparse and jitter == 3e-7
    assert np.array_equal(X, w.X)
    assert np.array_equal(Z, w.X[_documented_rows(len(w.X), M)])
    # x_mem / y_mem stay the whole memory, and that is what save_state ships to training
    assert len(m.x_mem) == len(w.X) and np.array_equal(np.asarray(m.x_mem), w.X) and np.array_equal(np.asarray(m.y_mem), w.Y)
    st = m.save_state()
    assert np.array_equal(np.asarray(st.inputs), w.X) and np.array_equal(np.asarray(st.states_change), w.Y)
    assert "num_inducing_points" not in st.constraints_hyperparams and "inducing_jitter" not in st.constraints_hyperparams


@pytest.mark.parametrize("M", [23, 24, 100])
def test_memory_no_larger_than_m_falls_through_to_prepare(w, M):
    m, eng = _model(w, num_inducing_points=M)
    m.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    (kind, X), = eng.log
    assert kind == "prepare" and np.array_equal(X, w.X) and not m.is_sparse


def test_inducing_inputs_override(w):
    Z = np.random.default_rng(0).uniform(0.0, 1.0, size=(5, w.X.shape[1]))
    for kw in (dict(), dict(num_inducing_points=7), dict(num_inducing_points=100)):
        m, eng = _model(w, **kw)
        m.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y), inducing_inputs=torch.as_tensor(Z))
        (kind, X, Zgot, jitter), = eng.log
        assert kind == "prepare_sparse" and np.array_equal(Zgot, Z) and np.array_equal(X, w.X) and jitter == 1e-6
        assert m.is_sparse and len(m.x_mem) == len(w.X)
        m.prepare_inference(torch.as_tensor(w.X[:4]), torch.as_tensor(w.Y[:4]))      # without it: the config's rule again
        assert eng.log[-1][0] == "prepare" and not m.is_sparse


def test_forget_on_a_sparse_model_is_a_clear_error_and_changes_nothing(w):
    from gp_mpc_amd import GpmpcError, _lib
    m, eng = _model(w, num_inducing_points=7)
    m.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    eng.log.clear()
    with pytest.raises(GpmpcError) as ei:
        m.forget([0, 3])
    assert ei.value.code == _lib.GPMPC_ERR_ARG and "sparse" in str(ei.value)
    assert eng.log == [] and len(m.x_mem) == len(w.X) and m.is_sparse
    # the exact model of the same class still forgets
    m2, eng2 = _model(w)
    m2.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    m2.forget([0, 3])
    assert [k[0] for k in eng2.log] == ["prepare", "forget"] and len(m2.x_mem) == len(w.X) - 2


def test_capped_memory_and_sparse_model_together():
    """MemoryConfig.max_points_model with the option: the model cannot downdate, so every step re-prepares the window -- a
    sparse model of it, on the documented rows of the window."""
    N, M, steps = 12, 5, 4
    w = synth.make_workload(N=N, D=2, A=1, H=3, B=1, seed=6)
    eng = SparseStubEngine()
    c = make_controller(w, engine=eng, shard=False)
    c.memory.config.max_points_model = N
    c.memory.config.check_errors_for_storage = False
    c.transition_model.config.num_inducing_points = M
    np.random.seed(0)
    rng = np.random.default_rng(1)
    obs = w.mu0.copy()
    for s in range(steps):
        eng.log.clear()
        a = c.get_action(obs)
        x_mem = c.memory.get()[0].numpy()
        assert len(x_mem) == N
        assert [k[0] for k in eng.log] == ["prepare_sparse"], eng.log
        assert np.array_equal(eng.log[0][1], x_mem) and np.array_equal(eng.log[0][2], x_mem[_documented_rows(N, M)])
        assert np.array_equal(np.asarray(c.transition_model.x_mem), x_mem)
        nxt = np.clip(obs + 0.05 * rng.standard_normal(obs.shape), 0.05, 0.95)
        c.add_memory(obs, a, nxt, 0.0)
        obs = nxt
    assert s == steps - 1
