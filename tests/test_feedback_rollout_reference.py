"""Tier 1 (CPU): the numpy restatement of the closed-loop linearised rollout (tests/feedback_rollout_ref.py) -- the yardstick of
the GPU tests of gpmpc_rollout_linear_feedback -- tied to things it does not define itself: the open-loop restatement at zero
gains, the torch-autograd Jacobian of the closed-loop mean map, and the deadbeat gain that cancels the inherited covariance.
Then the host plumbing of `feedback_gains` / ControllerConfig.feedback_gain with a CPU stand-in engine.
"""
import numpy as np
import pytest
import torch

import feedback_rollout_ref as fb
import linear_moments_ref as lin
import linear_moments_torch_ref as lt
from oracle import gpmpc_oracle as orc
from oracle import synth


def _factors(w):
    f = orc.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    return f, (f.X, f.lengthscales, f.variances, f.iK, f.beta)


def _workload(N, D, A, H, B, time, seed):
    return synth.make_workload(N, D, A, H, B, include_time=time, seed=seed, time0=3.0, dynamics="contracting", dense_s0=0.02)


def deadbeat_gain(V, D, A):
    """K = -V_u^-T (I + V_s)^T: the gain with I + C_0 = I + V_s + K^T V_u = 0 (needs A = D and V_u regular)."""
    Vs, Vu = V[:D], V[D:D + A]
    return -np.linalg.solve(Vu.T, (np.eye(D) + Vs).T)


# -- 1. zero gains are the open loop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time", [False, True])
def test_zero_gains_reproduce_the_open_loop_recurrence(time):
    w = _workload(40, 3, 2, 4, 3, time, seed=61)
    _, fa = _factors(w)
    mu, Sig = fb.rollout(*fa, w.actions, np.zeros((3, 4, 2, 3)), w.mu0, w.S0, w.include_time, w.time0)
    mu_o, Sig_o = lin.rollout(*fa, w.actions, w.mu0, w.S0, w.include_time, w.time0)
    assert np.array_equal(mu, mu_o) and np.array_equal(Sig, Sig_o)
    # ... and the gains never move the mean
    K = np.random.default_rng(62).standard_normal((3, 4, 2, 3))
    mu_k, Sig_k = fb.rollout(*fa, w.actions, K, w.mu0, w.S0, w.include_time, w.time0)
    assert np.array_equal(mu_k, mu_o) and not np.allclose(Sig_k[:, 1:], Sig_o[:, 1:], rtol=1e-3, atol=0)
    # the three gain layouts are one recurrence
    mu_s, Sig_s = fb.rollout(*fa, w.actions, K[0], w.mu0, w.S0, w.include_time, w.time0)
    assert np.array_equal(Sig_s[0], Sig_k[0])
    _, Sig_c = fb.rollout(*fa, w.actions, K[0, 0], w.mu0, w.S0, w.include_time, w.time0)
    _, Sig_t = fb.rollout(*fa, w.actions, np.tile(K[0, 0], (3, 4, 1, 1)), w.mu0, w.S0, w.include_time, w.time0)
    assert np.array_equal(Sig_c, Sig_t) and np.array_equal(Sig_c[0, 1], Sig_k[0, 1])


# -- 2. an independent derivation: the covariance goes through the Jacobian of the closed-loop mean map -----------------------
@pytest.mark.parametrize("D,A,time", [(3, 1, False), (3, 2, True), (2, 2, False)])
def test_one_step_covariance_is_the_autograd_jacobian_sandwich(D, A, time):
    w = _workload(50, D, A, 1, 1, time, seed=71 + D + A)
    _, fa = _factors(w)
    K = np.random.default_rng(72).standard_normal((A, D))
    _, Sig = fb.rollout(*fa, w.actions, K, w.mu0, w.S0, w.include_time, w.time0)
    E = w.X.shape[1]
    m0 = np.concatenate([w.mu0, w.actions[0, 0], [w.time0] if time else []])
    _, _, _, v = lin.step(*fa, m0[None])
    ft = lt.factors_t(fa)
    mu_t, ubar, Kt = (torch.as_tensor(a) for a in (w.mu0, w.actions[0, 0], K))

    def closed_loop_mean(x):                        # x -> x + mean([x | ubar + K (x - mu) | time])
        cols = [x, ubar + Kt @ (x - mu_t)]
        if time:
            cols.append(torch.full((1,), float(w.time0), dtype=torch.float64))
        M, _, _, _ = lt.step(*ft, torch.cat(cols)[None])
        return x + M[0]
    J = torch.autograd.functional.jacobian(closed_loop_mean, mu_t.clone()).numpy()
    assert J.shape == (D, D) and E == D + A + int(time)
    want = J @ w.S0 @ J.T
    got = Sig[0, 1] - np.diag(v[0])
    # two fp64 evaluations of D x D products of O(1) factors with |S0|: rounding of a few ulp of |S0|, and diag v carries
    # the ~1e-12 absolute rounding of sigma2 - k^T iK k once on each side of the subtraction (the same v: it cancels)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(w.S0)), np.max(np.abs(got - want))
    # the open loop is a different matrix: the gains are felt
    _, Sig_o = lin.rollout(*fa, w.actions, w.mu0, w.S0, w.include_time, w.time0)
    assert np.max(np.abs(Sig_o[0, 1] - Sig[0, 1])) > 1e-3 * np.max(np.abs(w.S0))


# -- 3. the deadbeat gain removes the inherited covariance -------------------------------------------------------------------
def test_deadbeat_gain_leaves_the_model_variance_alone():
    w = synth.make_workload(50, 2, 2, 1, 4, seed=2, dynamics="contracting", dense_s0=0.02)
    _, fa = _factors(w)
    m0 = np.concatenate([w.mu0, w.actions[0, 0]])
    _, _, V, v = lin.step(*fa, m0[None])
    assert np.linalg.cond(V[0, 2:4]) < 5.0
    K = deadbeat_gain(V[0], 2, 2)
    _, Sig = fb.rollout(*fa, w.actions[:1], K, w.mu0, w.S0)
    resid = float(np.max(np.abs(Sig[0, 1] - np.diag(v[0]))))
    print("deadbeat residual", resid, "max|S0|", float(np.max(np.abs(w.S0))))
    # the error of C is eps cond(V_u) O(1) and enters Sigma_1 as 2 dC Sigma_0: ~1e-15 |S0| (3e-19 absolute measured in fp64)
    assert resid <= 1e-12 * np.max(np.abs(w.S0))
    # a wrong sign or a transposed gain leaves O(|S0|)
    for bad in (-K, K.T):
        _, Sb = fb.rollout(*fa, w.actions[:1], bad, w.mu0, w.S0)
        assert np.max(np.abs(Sb[0, 1] - np.diag(v[0]))) > 1e-2 * np.max(np.abs(w.S0))


# -- 4. costs: Sigma_z in the host mapper's formula --------------------------------------------------------------------------
def test_costs_at_zero_gains_are_the_open_loop_costs():
    w = _workload(40, 3, 2, 3, 2, False, seed=81)
    _, fa = _factors(w)
    mu, Sig = lin.rollout(*fa, w.actions, w.mu0, w.S0)
    for clip, smin, smax in ((False, None, None), (True, np.full(3, 0.05), np.full(3, 0.9))):
        cfg = lin.reward_config_of(w, clip, smin, smax)
        open_loop = lin.costs(cfg, mu, Sig, w.actions)
        closed = fb.costs(cfg, mu, Sig, w.actions, np.zeros((2, 3)))
        for a, b in zip(open_loop, closed):
            assert np.allclose(a, b, rtol=1e-14, atol=0)
    # a gain adds the action's share K Sigma K^T of the covariance: with a positive action weight the expected cost grows
    cfg = lin.reward_config_of(w)
    cm0, _, _ = fb.costs(cfg, mu, Sig, w.actions, np.zeros((2, 3)))
    cm1, _, _ = fb.costs(cfg, mu, Sig, w.actions, np.ones((2, 3)))
    assert np.all(cm1[:, :3] > cm0[:, :3]) and np.array_equal(cm1[:, 3], cm0[:, 3])


# -- 5. the engine's shape rules ------------------------------------------------------------------------------------------------
def test_gain_shape_rules():
    from gp_mpc_amd.engine import feedback_gains_layout
    B, H, A, D = 7, 5, 2, 3
    assert feedback_gains_layout((A, D), B, H, A, D) == (False, True)
    assert feedback_gains_layout((H, A, D), B, H, A, D) == (False, False)
    assert feedback_gains_layout((B, H, A, D), B, H, A, D) == (True, False)
    assert feedback_gains_layout(torch.Size((B, H, A, D)), B, H, A, D) == (True, False)
    for bad in ((D, A), (H, D, A), (B, A, D), (1, H, A, D), (B, 1, A, D), (B, H, D, A), (A * D,), ()):
        with pytest.raises(ValueError, match="feedback gains"):
            feedback_gains_layout(bad, B, H, A, D)


# -- 6. model and controller plumbing ------------------------------------------------------------------------------------------
def _model(w, propagation, eng):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    N, D, A, E, H, B = w.dims
    gp_init = {"noise_covar.noise": list(w.noises), "base_kernel.lengthscale": w.lengthscales.tolist(),
               "outputscale": list(w.outputscales)}
    model = GpStateTransitionModel(ModelConfig(gp_init=gp_init, uncertainty_propagation=propagation), D, A, engine=eng)
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    eng.set_cost(w.target, w.W, w.W_T, w.kappa)
    return model


def test_model_routes_to_the_feedback_rollout_only_with_gains():
    from feedback_stub_engine import FeedbackOracleEngine
    w = synth.make_workload(20, 3, 1, 2, 2, seed=41)
    K = np.random.default_rng(42).standard_normal((2, 2, 1, 3))
    eng = FeedbackOracleEngine()
    model = _model(w, "linearized", eng)
    _, fa = _factors(w)
    # without gains: the calls of today
    model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, stage_costs=False)
    model.predict_trajectory(w.actions[0], w.mu0, w.S0, 2, 0)
    model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, stage_costs=False, feedback_gains=None)
    assert eng.calls == ["rollout_linear"] * 3
    out = model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, stage_costs=False, feedback_gains=K)
    assert eng.calls[-1] == "rollout_linear_feedback" and set(out) == {"mu", "Sig"}
    assert np.array_equal(eng.gains_seen[-1], K)
    mu_ref, Sig_ref = fb.rollout(*fa, w.actions, K, w.mu0, w.S0)
    assert np.array_equal(out["Sig"].numpy(), Sig_ref) and np.array_equal(out["mu"].numpy(), mu_ref)
    mu, Sig = model.predict_trajectory(w.actions[1], w.mu0, w.S0, 2, 0, feedback_gains=K[1])
    assert eng.calls[-1] == "rollout_linear_feedback" and eng.gains_seen[-1].shape == (2, 1, 3)
    assert np.allclose(Sig.numpy(), Sig_ref[1], rtol=1e-12, atol=1e-11)          # (numpy rounds a batch of one differently)
    model.predict_trajectory(w.actions[1], w.mu0, w.S0, 2, 0, feedback_gains=torch.as_tensor(K[1, 0]))      # (A, D), a tensor
    assert eng.calls[-1] == "rollout_linear_feedback" and eng.gains_seen[-1].shape == (1, 3)
    # a per-call propagation decides like the configured one
    mm = _model(w, "moment_matching", FeedbackOracleEngine())
    mm.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, stage_costs=False, propagation="linearized", feedback_gains=K)
    assert mm.engine.calls == ["rollout_linear_feedback"]
    # moment matching has no closed-loop rollout
    with pytest.raises(ValueError, match="feedback_gains"):
        mm.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, stage_costs=False, feedback_gains=K)
    with pytest.raises(ValueError, match="feedback_gains"):
        mm.predict_trajectory(w.actions[0], w.mu0, w.S0, 2, 0, feedback_gains=K[0])
    with pytest.raises(ValueError, match="feedback_gains"):
        model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, stage_costs=False, propagation="moment_matching",
                                       feedback_gains=K)
    assert mm.engine.calls == ["rollout_linear_feedback"] and eng.calls.count("rollout") == 0
    # no autograd, for the gains as for the other inputs
    n_calls = len(eng.calls)
    Kg = torch.as_tensor(K).clone().requires_grad_(True)
    ag = torch.as_tensor(w.actions).clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, stage_costs=False, feedback_gains=Kg)
    with pytest.raises(NotImplementedError):
        model.predict_trajectory_batch(ag, w.mu0, w.S0, 2, 0, stage_costs=False, feedback_gains=K)
    assert len(eng.calls) == n_calls
    with torch.no_grad():
        model.predict_trajectory_batch(ag, w.mu0, w.S0, 2, 0, stage_costs=False, feedback_gains=Kg)
    assert eng.calls[-1] == "rollout_linear_feedback"


def _controller(w, propagation, optimize, candidate_optimizer, engine, feedback_gain):
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
                                                    cem_iterations=2, shard_over_ranks=False, feedback_gain=feedback_gain))
    c = GpMpcController(np.zeros(D), np.ones(D), np.zeros(A), np.ones(A), cfg, engine=engine)
    c.memory.model_inputs[:N] = torch.as_tensor(w.X)
    c.memory.model_targets[:N] = torch.as_tensor(w.Y)
    c.memory.len_mem_model = N
    return c


def test_controller_config_default():
    from gp_mpc_amd.config_classes import ControllerConfig
    assert ControllerConfig().feedback_gain is None
    K = np.ones((1, 3))
    assert ControllerConfig(feedback_gain=K).feedback_gain is K


@pytest.mark.parametrize("gain_shape", ["AD", "HAD"])
@pytest.mark.parametrize("optimize,optimizer", [(False, None), (True, "cem")])
def test_controller_plans_closed_loop(optimize, optimizer, gain_shape):
    from feedback_stub_engine import FeedbackOracleEngine
    w = synth.make_workload(20, 3, 1, 3, 1, seed=51)
    K = 0.3 * np.random.default_rng(52).standard_normal((1, 3) if gain_shape == "AD" else (3, 1, 3))
    np.random.seed(5)
    eng = FeedbackOracleEngine()
    c = _controller(w, "linearized", optimize, optimizer, eng, K)
    a = c.get_action(w.mu0, w.S0)
    assert a.shape == (1,) and np.all(np.isfinite(a))
    assert "rollout_linear_feedback" in eng.calls and "rollout" not in eng.calls and "rollout_linear" not in eng.calls
    assert all(np.array_equal(g, K) for g in eng.gains_seen)
    # the cached trajectory is a closed-loop one: that of the sequence the search cached (the winner's under "cem")
    if optimizer == "cem":
        _, fa = _factors(w)
        acts = c.actions_mapper.mpc_to_model_batch(c.actions_mpc_previous_iter[None])
        state_mu, state_var = c.observation_state_mapper.get_state(obs=w.mu0, obs_var=w.S0, update_internals=False)
        _, Sig = fb.rollout(*fa, acts, K, np.asarray(state_mu), np.asarray(state_var))
        _, Sig_open = lin.rollout(*fa, acts, np.asarray(state_mu), np.asarray(state_var))
        # numpy's batched products round differently alone and in the search's batch; the variance sigma2 - k^T iK k cancels
        # terms of ~1e4, so that rounding is ~1e-12 absolute (the bounds of tests/test_linear_moments_reference.py)
        assert np.allclose(np.asarray(c.states_var_pred), Sig[0], rtol=1e-12, atol=1e-11)
        assert not np.allclose(np.asarray(c.states_var_pred)[1:], Sig_open[0, 1:], rtol=1e-2, atol=0)
    # without a gain the controller makes the calls of today
    np.random.seed(5)
    eng2 = FeedbackOracleEngine()
    _controller(w, "linearized", optimize, optimizer, eng2, None).get_action(w.mu0, w.S0)
    assert "rollout_linear" in eng2.calls and "rollout_linear_feedback" not in eng2.calls


def test_controller_refuses_a_gain_under_moment_matching():
    from feedback_stub_engine import FeedbackOracleEngine
    w = synth.make_workload(20, 3, 1, 3, 1, seed=53)
    K = np.zeros((1, 3))
    for optimize, optimizer in ((False, None), (True, "cem")):
        with pytest.raises(ValueError, match="feedback_gain"):                 # at construction
            _controller(w, "moment_matching", optimize, optimizer, FeedbackOracleEngine(), K)
        # ... and at first use, when the configuration changes after construction
        eng = FeedbackOracleEngine()
        c = _controller(w, "moment_matching", optimize, optimizer, eng, None)
        c.config.controller.feedback_gain = K
        with pytest.raises(ValueError, match="feedback_gain"):
            c.get_action(w.mu0, w.S0)
        with pytest.raises(ValueError, match="feedback_gain"):
            c.evaluate_candidates(np.full((2, 3), 0.5), w.mu0, w.S0)
        assert eng.calls == []
    # the optimisers the linearised path refuses stay refused, with or without a gain
    for optimizer in (None, "cem_device", "lbfgs"):
        with pytest.raises(ValueError, match="cem"):
            _controller(w, "linearized", True, optimizer, FeedbackOracleEngine(), K)
