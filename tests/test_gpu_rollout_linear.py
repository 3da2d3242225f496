"""Tier 2 (GPU): gpmpc_rollout_linear -- the horizon rollout on the linearised step (gpmpc_moments_linear) and its way up
through the engine, the transition model and the controller.

Checked against the long-double recurrence of tests/linear_moments_ref.py, against gpmpc_rollout where the two must coincide
(one step from a zero initial covariance), against the host SetpointStateRewardMapper for the costs, and against the contracts
of include/gpmpc.h: exact symmetry, bitwise batch invariance, errors.
"""
import numpy as np
import pytest
import torch

import linear_moments_ref as lin
from helpers import rel_err, record, make_controller
from oracle import synth

pytestmark = pytest.mark.gpu


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


def _workload(N, H, B, time, seed, D=3, A=1):
    # contracting dynamics keep a long rollout inside the memory's range; a dense initial covariance exercises every term
    return synth.make_workload(N, D, A, H, B, include_time=time, seed=seed, time0=3.0, dynamics="contracting", dense_s0=0.02)


def _prepared(engine, w):
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)
    iK, beta = (_np(t) for t in engine.factors())
    return (w.X, w.lengthscales, w.outputscales, iK, beta)


# H: 1, 5, 12; B: 1 (one row of one tile), 65 (two tiles), 130 (three); N: 50 (one partial column block) and 300 (two)
CASES = {
    "n50_h1_b65": (50, 1, 65, False),
    "n50_h5_b1_time": (50, 5, 1, True),
    "n50_h12_b130": (50, 12, 130, False),
    "n300_h5_b65_time": (300, 5, 65, True),
    "n300_h12_b1": (300, 12, 1, False),
}


# -- 1. the long-double recurrence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_trajectory_against_extended_precision(engine, case):
    N, H, B, time = CASES[case]
    w = _workload(N, H, B, time, seed=300 + N + H)
    fa = _prepared(engine, w)
    out = engine.rollout_linear(w.actions, w.mu0, w.S0, w.include_time, w.time0)
    mu, Sig = _np(out["mu"]), _np(out["Sig"])
    assert np.array_equal(mu[:, 0], np.broadcast_to(w.mu0, (B, 3))) and np.array_equal(Sig[:, 0], np.broadcast_to(w.S0, (B, 3, 3)))
    sel = np.unique(np.array([0, B // 2, B - 1]))                        # the long-double recurrence of a few candidates
    m64, S64 = lin.rollout(*fa, w.actions[sel], w.mu0, w.S0, w.include_time, w.time0)
    mld, Sld = lin.rollout(*fa, w.actions[sel], w.mu0, w.S0, w.include_time, w.time0, dtype=np.longdouble)
    errs = {"mu_hip": float(np.max(np.abs(mu[sel] - mld))), "mu_numpy": float(np.max(np.abs(m64 - mld))),
            "Sig_hip": float(np.max(np.abs(Sig[sel] - Sld))), "Sig_numpy": float(np.max(np.abs(S64 - Sld)))}
    scale = {"mu": float(np.max(np.abs(mld))), "Sig": float(np.max(np.abs(Sld)))}
    record(f"rollout_linear_extended[{case}]", **errs)
    print(case, errs, scale)
    # the rule of tests/test_gpu_predict.py: the HIP evaluation rounds like a plain fp64 evaluation of the same recurrence
    assert errs["mu_hip"] <= 3 * max(errs["mu_numpy"], 1e-12 * scale["mu"]), errs
    assert errs["Sig_hip"] <= 3 * max(errs["Sig_numpy"], 1e-12 * scale["Sig"]), errs
    assert torch.equal(out["Sig"][:, 1:], out["Sig"][:, 1:].transpose(2, 3))           # exactly symmetric


# -- 2. one step from a zero covariance is moment matching's first step ------------------------------------------------------
@pytest.mark.parametrize("N,time", [(50, False), (300, True)])
def test_first_step_from_zero_covariance_equals_rollout(engine, N, time):
    w = _workload(N, 1, 65, time, seed=310 + N)
    _prepared(engine, w)
    S0 = np.zeros((3, 3))
    a = engine.rollout_linear(w.actions, w.mu0, S0, w.include_time, w.time0, stage_costs=False)
    b = engine.rollout(w.actions, w.mu0, S0, w.include_time, w.time0, stage_costs=False)
    # two fp64 evaluations of the same sums in different orders (the bounds of tests/test_gpu_predict.py's closed-form checks);
    # moment matching's off-diagonal covariance beta_a^T L beta_b - M_a M_b is zero only to rounding
    assert rel_err(_np(a["mu"]), _np(b["mu"])) < 1e-10
    assert np.max(np.abs(_np(a["Sig"]) - _np(b["Sig"]))) < 1e-10 * float(np.max(w.outputscales))


# -- 3. costs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip,constraints", [(False, False), (True, False), (False, True), (True, True)])
def test_costs_match_the_host_mapper(engine, clip, constraints):
    w = _workload(50, 5, 65, False, seed=320)
    w.kappa = 3.0
    _prepared(engine, w)
    smin, smax = (np.full(3, 0.05), np.full(3, 0.9)) if constraints else (None, None)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa, clip, smin, smax)
    try:
        out = engine.rollout_linear(w.actions, w.mu0, w.S0)
        cfg = lin.reward_config_of(w, clip, smin, smax)
        cm, cv, J = lin.costs(cfg, _np(out["mu"]), _np(out["Sig"]), w.actions)
        # the device cost kernel against the host mapper on the SAME trajectory: fp64 rounding of O(D^3) sums
        assert rel_err(_np(out["cost_mu"]), cm) < 1e-12
        assert rel_err(_np(out["cost_var"]), cv) < 1e-11
        assert rel_err(_np(out["J"]), J) < 1e-11
        # the objective alone, without the caller keeping the trajectory: the same bits
        J_only = engine.rollout_linear(w.actions, w.mu0, w.S0, trajectories=False, stage_costs=False,
                                       out={"J": torch.empty(65, dtype=torch.float64, device=engine.device)})
        assert torch.equal(J_only["J"], out["J"])
    finally:
        engine.set_cost(w.target, w.W, w.W_T, w.kappa)


# -- 4. bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,time", [(50, True), (300, False)])
def test_batch_invariance(engine, N, time):
    w = _workload(N, 5, 130, time, seed=330 + N)
    _prepared(engine, w)
    full = engine.rollout_linear(w.actions, w.mu0, w.S0, w.include_time, w.time0)
    again = engine.rollout_linear(w.actions, w.mu0, w.S0, w.include_time, w.time0)
    keys = ("mu", "Sig", "cost_mu", "cost_var", "J")
    for k in keys:
        assert torch.equal(full[k], again[k]), k
    for i in (0, 63, 64, 129):
        one = engine.rollout_linear(w.actions[i:i + 1], w.mu0, w.S0, w.include_time, w.time0)
        for k in keys:
            assert torch.equal(one[k][0], full[k][i]), (k, i)
    perm = np.random.default_rng(331).permutation(130)
    mixed = engine.rollout_linear(w.actions[perm], w.mu0, w.S0, w.include_time, w.time0)
    for k in keys:
        assert torch.equal(mixed[k], full[k][torch.as_tensor(perm, device=engine.device)]), k
    for chunk in (1, 7, 64):
        engine.set_option("moments_linear_chunk_points", chunk)
        try:
            chunked = engine.rollout_linear(w.actions[:70], w.mu0, w.S0, w.include_time, w.time0)
            J_only = engine.rollout_linear(w.actions[:70], w.mu0, w.S0, w.include_time, w.time0, trajectories=False,
                                           stage_costs=False, out={"J": torch.empty(70, dtype=torch.float64, device=engine.device)})
        finally:
            engine.set_option("moments_linear_chunk_points", 0)
        for k in keys:
            assert torch.equal(chunked[k], full[k][:70]), (k, chunk)
        assert torch.equal(J_only["J"], full["J"][:70]), chunk


# -- 5. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_and_no_interference():
    from gp_mpc_amd import _lib as L
    eng = _fresh()
    try:
        w = _workload(50, 3, 4, False, seed=340)
        acts = eng._dev(w.actions)
        mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
        mu = torch.empty((4, 4, 3), dtype=torch.float64, device=eng.device)
        Sig = torch.empty((4, 4, 3, 3), dtype=torch.float64, device=eng.device)
        J = torch.empty(4, dtype=torch.float64, device=eng.device)
        hp = lambda a: a.ctypes.data                                        # noqa: E731

        def call(B=4, H=3, A=1, time=0, actions=acts.data_ptr(), m0=hp(mu0), J_ptr=None):
            return eng.lib.gpmpc_rollout_linear(eng._h, actions, m0, hp(S0), B, H, A, time, 0.0, mu.data_ptr(), Sig.data_ptr(),
                                                None, None, J_ptr, eng._stream())
        assert call() == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        assert call() == L.GPMPC_OK                                          # the plain trajectory needs no cost settings
        assert call(J_ptr=J.data_ptr()) == L.GPMPC_ERR_ARG and "set_cost" in eng.lib.gpmpc_last_error(eng._h).decode()
        with pytest.raises(RuntimeError) as ei:
            eng.rollout_linear(w.actions, w.mu0, w.S0)
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        for kw in (dict(B=0), dict(H=0), dict(A=-1), dict(A=2), dict(time=1), dict(actions=None), dict(m0=None)):
            assert call(**kw) == L.GPMPC_ERR_ARG, kw
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        assert call(J_ptr=J.data_ptr()) == L.GPMPC_OK
        # no interference: the moment-matched rollout gives the same bits before and after, the gpmpc_last_* state stays
        before = {k: v.clone() for k, v in eng.rollout(w.actions, w.mu0, w.S0).items()}
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path)
        lin_out = eng.rollout_linear(w.actions, w.mu0, w.S0)
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path) == state
        after = eng.rollout(w.actions, w.mu0, w.S0)
        for k in before:
            assert torch.equal(before[k], after[k]), k
        assert not torch.equal(lin_out["Sig"], before["Sig"])                # (a different approximation)
    finally:
        eng.close()


# -- 6. model and controller ---------------------------------------------------------------------------------------------------
def test_transition_model_linearized_trajectory(engine):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    w = synth.make_workload(60, 3, 1, 4, 5, seed=350, dense_s0=0.01)
    model = GpStateTransitionModel(ModelConfig(), 3, 1, engine=engine)
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    model.set_cost(lin.reward_config_of(w))
    ref = engine.rollout_linear(w.actions, w.mu0, w.S0)
    out = model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 4, 0, propagation="linearized")
    for k in ("mu", "Sig", "cost_mu", "cost_var", "J"):
        assert out[k].device.type == "cuda" and torch.equal(out[k], ref[k]), k
    mu, Sig = model.predict_trajectory(w.actions[2], w.mu0, w.S0, 4, 0, propagation="linearized")
    assert torch.equal(mu, ref["mu"][2].cpu()) and torch.equal(Sig, ref["Sig"][2].cpu())
    default = model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 4, 0)
    assert torch.equal(default["Sig"], engine.rollout(w.actions, w.mu0, w.S0)["Sig"])
    model.config.uncertainty_propagation = "linearized"
    assert torch.equal(model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 4, 0)["J"], ref["J"])
    with pytest.raises(NotImplementedError):
        model.predict_trajectory_batch(torch.as_tensor(w.actions).requires_grad_(True), w.mu0, w.S0, 4, 0)


def test_controller_cem_with_linearized_propagation(engine):
    w = synth.make_workload(40, 3, 1, 4, 1, seed=360)
    np.random.seed(7)
    c = make_controller(w, optimize=False, engine=engine, shard=False)
    c.config.controller.optimize = True
    c.config.controller.candidate_optimizer = "cem"
    c.config.controller.cem_candidates, c.config.controller.cem_iterations = 16, 2
    c.transition_model.config.uncertainty_propagation = "linearized"
    a = c.get_action(obs_mu=w.mu0)
    assert a.shape == (1,) and np.all(np.isfinite(a)) and 0.0 <= float(a[0]) <= 1.0
    assert c.num_rollouts == 32
    assert np.isfinite(c.best_candidate_J)
    # the cached trajectory is the linearised one of the winning sequence
    acts = c.actions_mapper.mpc_to_model_batch(c.actions_mpc_previous_iter[None])
    state_mu, state_var = c.observation_state_mapper.get_state(obs=w.mu0, obs_var=None, update_internals=False)
    ref = engine.rollout_linear(acts, state_mu, state_var)
    assert torch.equal(torch.as_tensor(c.states_mu_pred), ref["mu"][0].cpu())
    c.config.controller.candidate_optimizer = "cem_device"
    with pytest.raises(ValueError, match="cem"):
        c.get_action(obs_mu=w.mu0)
