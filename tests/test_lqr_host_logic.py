"""Tier 1 (CPU): the host plumbing of `feedback_gains="lqr"` (GpStateTransitionModel) and `ControllerConfig(feedback_gain="lqr",
feedback_lqr_reg=...)` with the CPU stand-in engine of tests/lqr_stub_engine.py: what is called, with which gains and which
regularisation, and what stays refused."""
import numpy as np
import pytest
import torch

import feedback_rollout_ref as fb
import linear_moments_ref as lin
import lqr_gains_ref as lq
from lqr_stub_engine import LqrOracleEngine
from oracle import gpmpc_oracle as orc
from oracle import synth


def _factors(w):
    f = orc.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    return (f.X, f.lengthscales, f.variances, f.iK, f.beta)


def _model(w, propagation, eng):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    N, D, A, E, H, B = w.dims
    gp_init = {"noise_covar.noise": list(w.noises), "base_kernel.lengthscale": w.lengthscales.tolist(),
               "outputscale": list(w.outputscales)}
    model = GpStateTransitionModel(ModelConfig(gp_init=gp_init, uncertainty_propagation=propagation), D, A, engine=eng)
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    model.set_cost(lin.reward_config_of(w))
    return model


def _controller(w, propagation, optimize, candidate_optimizer, engine, feedback_gain, **kw):
    import gp_mpc_amd  # noqa: F401
    from gp_mpc_amd.config_classes import (Config, ControllerConfig, ActionsConfig, ObservationConfig, MemoryConfig, ModelConfig,
                                           TrainingConfig)
    from gp_mpc_amd import GpMpcController
    N, D, A, E, H, B = w.dims
    model = ModelConfig(gp_init={"noise_covar.noise": list(w.noises), "base_kernel.lengthscale": w.lengthscales.tolist(),
                                 "outputscale": list(w.outputscales)}, uncertainty_propagation=propagation)
    cfg = Config(observation_config=ObservationConfig(obs_var_norm=list(np.diag(w.S0))), reward_config=lin.reward_config_of(w),
                 actions_config=ActionsConfig(limit_action_change=False, max_change_action_norm=[0.3] * A),
                 model_config=model, memory_config=MemoryConfig(points_batch_memory=N + 8),
                 training_config=TrainingConfig(training_frequency=10 ** 9),
                 controller_config=ControllerConfig(len_horizon=H, restarts_optim=3, optimize=optimize,
                                                    candidate_optimizer=candidate_optimizer, cem_candidates=6,
                                                    cem_iterations=2, shard_over_ranks=False, feedback_gain=feedback_gain, **kw))
    c = GpMpcController(np.zeros(D), np.ones(D), np.zeros(A), np.ones(A), cfg, engine=engine)
    c.memory.model_inputs[:N] = torch.as_tensor(w.X)
    c.memory.model_targets[:N] = torch.as_tensor(w.Y)
    c.memory.len_mem_model = N
    return c


def test_model_routes_lqr_to_the_gain_design_and_the_feedback_rollout():
    w = synth.make_workload(20, 3, 1, 2, 2, seed=41)
    eng = LqrOracleEngine()
    model = _model(w, "linearized", eng)
    fa = _factors(w)
    out = model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, feedback_gains="lqr", lqr_reg=0.125)
    assert eng.calls == ["lqr_gains", "rollout_linear_feedback"] and eng.regs_seen == [0.125]
    assert set(out) == {"mu", "Sig", "J", "cost_mu", "cost_var", "gains"}
    assert eng.gains_seen[-1].shape == (2, 2, 1, 3)                       # per candidate: (B, H, A, D)
    K, _, _ = lq.gains(*fa, w.actions, w.mu0, w.W, w.W_T, reg=0.125)
    assert np.array_equal(eng.gains_seen[-1], K) and np.array_equal(out["gains"].numpy(), K)
    mu_ref, Sig_ref = fb.rollout(*fa, w.actions, K, w.mu0, w.S0)
    assert np.array_equal(out["Sig"].numpy(), Sig_ref) and np.array_equal(out["mu"].numpy(), mu_ref)
    # the default regularisation is zero; one sequence goes the same way
    mu, Sig = model.predict_trajectory(w.actions[1], w.mu0, w.S0, 2, 0, feedback_gains="lqr")
    assert eng.calls[-2:] == ["lqr_gains", "rollout_linear_feedback"] and eng.regs_seen[-1] == 0.0
    assert eng.gains_seen[-1].shape == (1, 2, 1, 3) and mu.shape == (3, 3) and Sig.shape == (3, 3, 3)
    # an array keeps the call of today
    n = eng.calls.count("lqr_gains")
    model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, stage_costs=False, feedback_gains=K)
    assert eng.calls.count("lqr_gains") == n and eng.calls[-1] == "rollout_linear_feedback"
    # a per-call propagation decides like the configured one
    mm = _model(w, "moment_matching", LqrOracleEngine())
    mm.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, propagation="linearized", feedback_gains="lqr")
    assert mm.engine.calls == ["lqr_gains", "rollout_linear_feedback"]


def test_model_refusals():
    w = synth.make_workload(20, 3, 1, 2, 2, seed=43)
    eng = LqrOracleEngine()
    model = _model(w, "linearized", eng)
    mm = _model(w, "moment_matching", LqrOracleEngine())
    with pytest.raises(ValueError, match="feedback_gains"):                # moment matching has no closed-loop rollout
        mm.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, feedback_gains="lqr")
    with pytest.raises(ValueError, match="feedback_gains"):
        mm.predict_trajectory(w.actions[0], w.mu0, w.S0, 2, 0, feedback_gains="lqr")
    with pytest.raises(ValueError, match="feedback_gains"):
        model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, propagation="moment_matching", feedback_gains="lqr")
    for name in ("LQR", "ilqr", ""):                                       # any other string
        with pytest.raises(ValueError, match="lqr"):
            model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, feedback_gains=name)
        with pytest.raises(ValueError, match="lqr"):
            mm.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, feedback_gains=name)
    ag = torch.as_tensor(w.actions).clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):                               # no autograd through the gain design either
        model.predict_trajectory_batch(ag, w.mu0, w.S0, 2, 0, feedback_gains="lqr")
    assert eng.calls == [] and mm.engine.calls == []
    with torch.no_grad():
        model.predict_trajectory_batch(ag, w.mu0, w.S0, 2, 0, feedback_gains="lqr")
    assert eng.calls == ["lqr_gains", "rollout_linear_feedback"]


def test_controller_config_fields():
    from gp_mpc_amd.config_classes import ControllerConfig
    assert ControllerConfig().feedback_lqr_reg == 0.0 and ControllerConfig().feedback_gain is None
    c = ControllerConfig(feedback_gain="lqr", feedback_lqr_reg=1e-3)
    assert c.feedback_gain == "lqr" and c.feedback_lqr_reg == 1e-3


@pytest.mark.parametrize("optimize,optimizer", [(False, None), (True, "cem")])
def test_controller_plans_under_lqr_gains(optimize, optimizer):
    w = synth.make_workload(20, 3, 1, 3, 1, seed=51)
    np.random.seed(5)
    eng = LqrOracleEngine()
    c = _controller(w, "linearized", optimize, optimizer, eng, "lqr", feedback_lqr_reg=0.5)
    a = c.get_action(w.mu0, w.S0)
    assert a.shape == (1,) and np.all(np.isfinite(a))
    assert "rollout" not in eng.calls and "rollout_linear" not in eng.calls
    # every evaluation is a gain design followed by the closed-loop rollout with (B, H, A, D) gains
    assert eng.calls[0::2] == ["lqr_gains"] * (len(eng.calls) // 2)
    assert eng.calls[1::2] == ["rollout_linear_feedback"] * (len(eng.calls) // 2)
    assert all(r == 0.5 for r in eng.regs_seen) and len(eng.regs_seen) == len(eng.gains_seen)
    assert all(g.ndim == 4 and g.shape[1:] == (3, 1, 3) for g in eng.gains_seen)
    if optimizer == "cem":                                                 # the cached trajectory is the winner's closed-loop one
        fa = _factors(w)
        acts = c.actions_mapper.mpc_to_model_batch(c.actions_mpc_previous_iter[None])
        state_mu, state_var = c.observation_state_mapper.get_state(obs=w.mu0, obs_var=w.S0, update_internals=False)
        K, _, _ = lq.gains(*fa, acts, np.asarray(state_mu), w.W, w.W_T, reg=0.5)
        _, Sig = fb.rollout(*fa, acts, K, np.asarray(state_mu), np.asarray(state_var))
        _, Sig_open = lin.rollout(*fa, acts, np.asarray(state_mu), np.asarray(state_var))
        # (the bounds of tests/test_feedback_rollout_reference.py: numpy rounds a batch of one differently)
        assert np.allclose(np.asarray(c.states_var_pred), Sig[0], rtol=1e-12, atol=1e-11)
        assert not np.allclose(np.asarray(c.states_var_pred)[1:], Sig_open[0, 1:], rtol=1e-3, atol=0)
    # an array-valued gain behaves as before: no gain design
    np.random.seed(5)
    eng2 = LqrOracleEngine()
    Kfix = 0.3 * np.random.default_rng(52).standard_normal((1, 3))
    _controller(w, "linearized", optimize, optimizer, eng2, Kfix).get_action(w.mu0, w.S0)
    assert "lqr_gains" not in eng2.calls and "rollout_linear_feedback" in eng2.calls
    assert all(np.array_equal(g, Kfix) for g in eng2.gains_seen)


def test_controller_refusals():
    w = synth.make_workload(20, 3, 1, 3, 1, seed=53)
    for optimize, optimizer in ((False, None), (True, "cem")):
        with pytest.raises(ValueError, match="feedback_gain"):                 # moment matching, at construction
            _controller(w, "moment_matching", optimize, optimizer, LqrOracleEngine(), "lqr")
        eng = LqrOracleEngine()
        c = _controller(w, "moment_matching", optimize, optimizer, eng, None)
        c.config.controller.feedback_gain = "lqr"                              # ... and at first use
        with pytest.raises(ValueError, match="feedback_gain"):
            c.get_action(w.mu0, w.S0)
        assert eng.calls == []
    for optimizer in (None, "cem_device", "lbfgs"):                            # the optimisers the linearised path refuses
        with pytest.raises(ValueError, match="cem"):
            _controller(w, "linearized", True, optimizer, LqrOracleEngine(), "lqr")
    eng = LqrOracleEngine()
    c = _controller(w, "linearized", False, None, eng, "ilqr")                 # an unknown string
    with pytest.raises(ValueError, match="lqr"):
        c.get_action(w.mu0, w.S0)
    assert eng.calls == []
