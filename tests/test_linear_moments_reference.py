"""Tier 1 (CPU): the numpy restatement of the linearised propagation (tests/linear_moments_ref.py) -- the yardstick of the GPU
tests of gpmpc_moments_linear / gpmpc_rollout_linear -- tied to things it does not define itself: the reference's own
predict_next_state_change at zero input variance (golden step_zero_var), finite differences of the posterior mean, and the
oracle's moment matching, with which it must agree to first order in the input covariance.  Then the host plumbing of
ModelConfig.uncertainty_propagation with a CPU stand-in engine.
"""
import numpy as np
import pytest
import torch

import linear_moments_ref as lin
from helpers import load, workload_of, rel_err
from oracle import gpmpc_oracle as orc
from oracle import synth


def _factors(w):
    f = orc.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    return f, (f.X, f.lengthscales, f.variances, f.iK, f.beta)


# -- 1. the reference's own step at Sigma = 0 ---------------------------------------------------------------------------------
def test_golden_step_zero_var():
    g = load("step_zero_var")
    w = workload_of(g)
    D = w.Y.shape[1]
    assert not np.any(g["in_var"])
    args = (w.X, w.lengthscales, w.outputscales, g["iK"], g["beta"], g["in_mean"][None])
    for Sigma in (None, g["in_var"][None]):
        M, S, V, v = lin.step(*args, Sigma)
        # the tolerances tests/test_gpu_predict.py applies to this golden: 1e-10 for the mean-type sums, 1e-7 for the covariance
        assert rel_err(M[0], g["M"].ravel()) < 1e-10
        assert rel_err(V[0], g["V"]) < 1e-10
        assert rel_err(np.diag(S[0]), np.diag(g["S"])[:D]) < 1e-7
        assert np.all(S[0][~np.eye(D, dtype=bool)] == 0.0)
        assert np.array_equal(np.diag(S[0]), v[0])


# -- 2. V is the Jacobian of the mean -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,A,time", [(1, 1, False), (3, 1, False), (3, 1, True)])
def test_jacobian_against_central_differences(D, A, time):
    w = synth.make_workload(50, D, A, 2, 1, include_time=time, seed=11 + D)
    f, fa = _factors(w)
    E = w.X.shape[1]
    rng = np.random.default_rng(12)
    m = w.X.min(axis=0) + (w.X.max(axis=0) - w.X.min(axis=0)) * rng.uniform(0.1, 0.9, size=(5, E))
    _, _, V, _ = lin.step(*fa, m, None, dtype=np.longdouble)
    # 4th-order central stencil in long double (eps 1e-19), h = 1e-3 of the input's lengthscale-relative unit: truncation
    # h^4 / 30 f^(5) ~ 3e-14 x (derivative growth <= a few / l^4, l >= 0.5), rounding 1e-19 / h = 1e-16 -- far inside 1e-9
    h = np.longdouble(1e-3)
    for e in range(E):
        step_e = h * np.longdouble(min(1.0, float(w.lengthscales[:, e].min())))
        d = np.zeros(E, dtype=np.longdouble)
        d[e] = step_e
        mm = np.asarray(m, dtype=np.longdouble)
        mean = lambda x: lin.mean_only(f.X, f.lengthscales, f.variances, f.beta, x)       # noqa: E731
        fd = (8 * (mean(mm + d) - mean(mm - d)) - (mean(mm + 2 * d) - mean(mm - 2 * d))) / (12 * step_e)
        scale = float(np.max(np.abs(V[:, e, :])))
        assert float(np.max(np.abs(fd - V[:, e, :]))) < 1e-9 * scale, e


# -- 3. first-order agreement with moment matching ----------------------------------------------------------------------------
@pytest.mark.parametrize("D,A,time", [(3, 1, False), (3, 1, True)])
def test_first_order_agreement_with_moment_matching(D, A, time):
    w = synth.make_workload(50, D, A, 2, 1, include_time=time, seed=21)
    f, fa = _factors(w)
    E = w.X.shape[1]
    rng = np.random.default_rng(22)
    m = w.X.min(axis=0) + (w.X.max(axis=0) - w.X.min(axis=0)) * rng.uniform(0.2, 0.8, size=(4, E))
    G = rng.standard_normal((E, E))
    Apd = G @ G.T / E + 0.1 * np.eye(E)                 # a fixed SPD matrix
    if time:
        Apd[-1, :] = Apd[:, -1] = 0.0                   # (the time input is known exactly, as in the rollouts)
    gaps = {}
    for eps in (1e-3, 1e-5):
        Sg = np.broadcast_to(eps * Apd, (4, E, E)).copy()
        Mm, Sm, Vm = orc.moment_match_step(f, m, Sg)
        Ml, Sl, Vl, _ = lin.step(*fa, m, Sg)
        gaps[eps] = (float(np.max(np.abs(Mm - Ml))), float(np.max(np.abs(Sm - Sl))))
    # the approximations agree to first order: the gap is O(eps) in M (the dropped 1/2 tr(H Sigma)) and O(eps^2) in S
    assert gaps[1e-3][0] > 0 and gaps[1e-3][1] > 0
    assert gaps[1e-5][0] * 50 <= gaps[1e-3][0], gaps
    assert gaps[1e-5][1] * 50 <= gaps[1e-3][1], gaps


# -- 4. the recurrence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time", [False, True])
def test_recurrence_against_hand_rolled_loop(time):
    w = synth.make_workload(40, 3, 1, 3, 2, include_time=time, seed=31, time0=4.0, dense_s0=0.02)
    f, fa = _factors(w)
    D, E = 3, w.X.shape[1]
    mu, Sig = lin.rollout(*fa, w.actions, w.mu0, w.S0, w.include_time, w.time0)
    assert mu.shape == (2, 4, 3) and Sig.shape == (2, 4, 3, 3)
    for b in range(2):
        m_t, S_t = w.mu0.copy(), w.S0.copy()
        assert np.array_equal(mu[b, 0], m_t) and np.array_equal(Sig[b, 0], S_t)
        for t in range(3):
            x = np.concatenate([m_t, w.actions[b, t], [w.time0 + t] if time else []])
            s = np.zeros((E, E))
            s[:D, :D] = S_t
            M, S, V, _ = lin.step(*fa, x[None], s[None])
            C = S_t @ V[0, :D]
            m_t, S_t = m_t + M[0], S_t + S[0] + C + C.T
            # the same fp64 formulas, batched or not: differences are rounding only.  The variance sigma2 - k^T iK k cancels
            # terms of size N k^2 / noise ~ 40 x 0.05^2 x 1e5 = 1e4, so its rounding is ~1e-12 absolute whatever S is
            assert np.allclose(mu[b, t + 1], m_t, rtol=1e-13, atol=0)
            assert np.allclose(Sig[b, t + 1], S_t, rtol=1e-12, atol=1e-11)
    # the costs of the restatement are the host mapper's: they agree with the oracle's batched formulas
    cm, cv, J = lin.costs(lin.reward_config_of(w), mu, Sig, w.actions)
    cm_o, cv_o = orc.stage_costs(mu, Sig, w.actions, w.target, w.W, w.W_T)
    assert rel_err(cm, cm_o) < 1e-12 and rel_err(cv, cv_o) < 1e-12
    assert rel_err(J, orc.lcb_objective(cm_o, cv_o, w.kappa)) < 1e-12


# -- 5. config, model and controller plumbing ---------------------------------------------------------------------------------
def _controller(w, propagation=None, optimize=False, candidate_optimizer=None, engine=None):
    import gp_mpc_amd  # noqa: F401
    from gp_mpc_amd.config_classes import (Config, ControllerConfig, ActionsConfig, RewardConfig, ObservationConfig,
                                           MemoryConfig, ModelConfig, TrainingConfig)
    from gp_mpc_amd import GpMpcController
    N, D, A, E, H, B = w.dims
    kw = {} if propagation is None else {"uncertainty_propagation": propagation}
    model = ModelConfig(gp_init={"noise_covar.noise": list(w.noises), "base_kernel.lengthscale": w.lengthscales.tolist(),
                                 "outputscale": list(w.outputscales)}, **kw)
    cfg = Config(observation_config=ObservationConfig(obs_var_norm=list(np.diag(w.S0))), reward_config=lin.reward_config_of(w),
                 actions_config=ActionsConfig(limit_action_change=False, max_change_action_norm=[0.3] * A),
                 model_config=model, memory_config=MemoryConfig(points_batch_memory=N + 8),
                 training_config=TrainingConfig(training_frequency=10 ** 9),
                 controller_config=ControllerConfig(len_horizon=H, restarts_optim=3, optimize=optimize,
                                                    candidate_optimizer=candidate_optimizer, cem_candidates=6,
                                                    cem_iterations=2, shard_over_ranks=False))
    c = GpMpcController(np.zeros(D), np.ones(D), np.zeros(A), np.ones(A), cfg, engine=engine)
    c.memory.model_inputs[:N] = torch.as_tensor(w.X)
    c.memory.model_targets[:N] = torch.as_tensor(w.Y)
    c.memory.len_mem_model = N
    return c


def test_config_default_and_values():
    from gp_mpc_amd.config_classes import ModelConfig
    assert ModelConfig().uncertainty_propagation == "moment_matching"
    assert ModelConfig(uncertainty_propagation="linearized").uncertainty_propagation == "linearized"
    with pytest.raises(ValueError):
        ModelConfig(uncertainty_propagation="unscented")


def test_model_routes_by_propagation():
    from linear_stub_engine import LinearOracleEngine
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    w = synth.make_workload(20, 3, 1, 2, 2, seed=41)
    gp_init = {"noise_covar.noise": list(w.noises), "base_kernel.lengthscale": w.lengthscales.tolist(),
               "outputscale": list(w.outputscales)}
    for configured in ("moment_matching", "linearized"):
        eng = LinearOracleEngine()
        model = GpStateTransitionModel(ModelConfig(gp_init=gp_init, uncertainty_propagation=configured), 3, 1, engine=eng)
        assert "uncertainty_propagation" not in model.save_state().constraints_hyperparams
        model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
        x, s = torch.as_tensor(w.X[:1].copy()), 1e-4 * torch.eye(4, dtype=torch.float64)[None]
        expected = "moments_linear" if configured == "linearized" else "moments"
        model.predict_next_state_change_batch(x, s)
        assert eng.calls[-1] == expected
        M, S, V = model.predict_next_state_change(x[0], s[0], propagation="linearized")
        assert eng.calls[-1] == "moments_linear" and M.shape == (1, 3) and S.shape == (3, 3) and V.shape == (4, 3)
        model.predict_next_state_change(x[0], s[0], propagation="moment_matching")
        assert eng.calls[-1] == "moments"
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        mu, Sig = model.predict_trajectory(w.actions[0], w.mu0, w.S0, 2, 0)
        assert eng.calls[-1] == ("rollout_linear" if configured == "linearized" else "rollout")
        assert mu.shape == (3, 3) and Sig.shape == (3, 3, 3)
        out = model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, stage_costs=False, propagation="linearized")
        assert eng.calls[-1] == "rollout_linear" and set(out) == {"mu", "Sig"}
        with pytest.raises(ValueError):
            model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, stage_costs=False, propagation="unscented")
        # no autograd on the linearised path: an input that requires grad is refused, not silently detached
        xg = x.clone().requires_grad_(True)
        ag = torch.as_tensor(w.actions).clone().requires_grad_(True)
        with pytest.raises(NotImplementedError):
            model.predict_next_state_change_batch(xg, s, propagation="linearized")
        with pytest.raises(NotImplementedError):
            model.predict_trajectory_batch(ag, w.mu0, w.S0, 2, 0, stage_costs=False, propagation="linearized")
        with torch.no_grad():
            model.predict_next_state_change_batch(xg, s, propagation="linearized")
            model.predict_trajectory_batch(ag, w.mu0, w.S0, 2, 0, stage_costs=False, propagation="linearized")


@pytest.mark.parametrize("optimize,optimizer", [(False, None), (True, "cem")])
def test_controller_searches_reach_the_linearised_rollout(optimize, optimizer):
    from linear_stub_engine import LinearOracleEngine
    w = synth.make_workload(20, 3, 1, 3, 1, seed=51)
    np.random.seed(5)
    eng = LinearOracleEngine()
    c = _controller(w, "linearized", optimize, optimizer, eng)
    a = c.get_action(w.mu0, w.S0)
    assert a.shape == (1,) and np.all(np.isfinite(a))
    assert "rollout_linear" in eng.calls and "rollout" not in eng.calls
    # the default configuration still goes through the moment-matched rollout
    eng2 = LinearOracleEngine()
    c2 = _controller(w, None, optimize, optimizer, eng2)
    c2.get_action(w.mu0, w.S0)
    assert "rollout" in eng2.calls and "rollout_linear" not in eng2.calls


@pytest.mark.parametrize("optimizer", [None, "cem_device", "lbfgs"])
def test_controller_refuses_optimisers_without_linearised_kernels(optimizer):
    from linear_stub_engine import LinearOracleEngine
    w = synth.make_workload(20, 3, 1, 3, 1, seed=52)
    with pytest.raises(ValueError, match="cem"):                       # at construction: the message names what is supported
        _controller(w, "linearized", True, optimizer, LinearOracleEngine())
    # ... and at first use, when the configuration changes after construction
    c = _controller(w, None, True, optimizer, LinearOracleEngine())
    c.transition_model.config.uncertainty_propagation = "linearized"
    with pytest.raises(ValueError, match="random shooting"):
        c.get_action(w.mu0, w.S0)
    with pytest.raises(ValueError, match="cem"):
        c.compute_mean_lcb_trajectory(np.full(3, 0.5), w.mu0, w.S0)
    with pytest.raises(ValueError, match="cem"):
        c.objective_and_gradient_batch(np.full((2, 3), 0.5), w.mu0, w.S0)
