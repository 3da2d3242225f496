"""Tier 2 (GPU): gpmpc_rollout_linear_feedback -- the linearised horizon rollout in closed loop, under the ancillary feedback
u = ubar_t + K_t (x - mu_t) -- and its way up through the engine, the transition model and the controller.

Checked against the long-double recurrence of tests/feedback_rollout_ref.py, against gpmpc_rollout_linear where the two must
coincide (the means always; everything without gains), against the host SetpointStateRewardMapper._quadratic with the full
state-action covariance for the costs, against the deadbeat gain that removes the inherited covariance, and against the contracts
of include/gpmpc.h: exact symmetry, bitwise invariance to the batch, the chunks and the gain layout, errors.
"""
import numpy as np
import pytest
import torch

import feedback_rollout_ref as fb
import linear_moments_ref as lin
from helpers import rel_err, record, make_controller
from oracle import synth

pytestmark = pytest.mark.gpu

KEYS = ("mu", "Sig", "cost_mu", "cost_var", "J")


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
    # as tests/test_gpu_rollout_linear.py: contracting dynamics, a dense initial covariance
    return synth.make_workload(N, D, A, H, B, include_time=time, seed=seed, time0=3.0, dynamics="contracting", dense_s0=0.02)


def _gains(w, seed, scale=1.0):
    N, D, A, E, H, B = w.dims
    return scale * np.random.default_rng(seed).standard_normal((B, H, A, D))


def _prepared(engine, w):
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)
    iK, beta = (_np(t) for t in engine.factors())
    return (w.X, w.lengthscales, w.outputscales, iK, beta)


# one, two and three row tiles (B = 1, 65, 130), one and two column blocks (N = 50, 300), A != D with A > 1
CASES = {
    "a_d3_a1_n50_h1_b65": (3, 1, 50, 1, 65, False),
    "b_d3_a2_n50_h5_b1_time": (3, 2, 50, 5, 1, True),
    "c_d3_a1_n50_h12_b130": (3, 1, 50, 12, 130, False),
    "d_d3_a2_n300_h5_b65_time": (3, 2, 300, 5, 65, True),
    "e_d5_a2_n300_h12_b1": (5, 2, 300, 12, 1, False),
}


# -- 1. the long-double recurrence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_trajectory_against_extended_precision(engine, case):
    D, A, N, H, B, time = CASES[case]
    w = _workload(N, H, B, time, seed=400 + N + H + A, D=D, A=A)
    fa = _prepared(engine, w)
    K = _gains(w, 401)
    out = engine.rollout_linear_feedback(w.actions, K, w.mu0, w.S0, w.include_time, w.time0)
    mu, Sig = _np(out["mu"]), _np(out["Sig"])
    assert np.array_equal(mu[:, 0], np.broadcast_to(w.mu0, (B, D))) and np.array_equal(Sig[:, 0], np.broadcast_to(w.S0, (B, D, D)))
    sel = np.unique(np.array([0, B // 2, B - 1]))
    args = (w.actions[sel], K[sel], w.mu0, w.S0, w.include_time, w.time0)
    m64, S64 = fb.rollout(*fa, *args)
    mld, Sld = fb.rollout(*fa, *args, dtype=np.longdouble)
    _, S_open = lin.rollout(*fa, w.actions[sel], w.mu0, w.S0, w.include_time, w.time0)
    errs = {"mu_hip": float(np.max(np.abs(mu[sel] - mld))), "mu_numpy": float(np.max(np.abs(m64 - mld))),
            "Sig_hip": float(np.max(np.abs(Sig[sel] - Sld))), "Sig_numpy": float(np.max(np.abs(S64 - Sld)))}
    scale = {"mu": float(np.max(np.abs(mld))), "Sig": float(np.max(np.abs(Sld)))}
    moved = float(np.max(np.abs(S_open - S64)))
    record(f"rollout_linear_feedback_extended[{case}]", gains_move_Sig_by=moved, **errs)
    print(case, errs, scale, "gains move Sig by", moved)
    # the rule of tests/test_gpu_predict.py: the HIP evaluation rounds like a plain fp64 evaluation of the same recurrence
    assert errs["mu_hip"] <= 3 * max(errs["mu_numpy"], 1e-12 * scale["mu"]), errs
    assert errs["Sig_hip"] <= 3 * max(errs["Sig_numpy"], 1e-12 * scale["Sig"]), errs
    assert moved > 1e4 * 3 * max(errs["Sig_numpy"], 1e-12 * scale["Sig"])     # a kernel that ignores the gains fails by far
    assert torch.equal(out["Sig"][:, 1:], out["Sig"][:, 1:].transpose(2, 3))           # exactly symmetric


# -- 2. means and the NULL form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,time,A", [(50, False, 2), (300, True, 1)])
def test_means_and_the_form_without_gains(engine, N, time, A):
    w = _workload(N, 5, 65, time, seed=410 + N, A=A)
    _prepared(engine, w)
    open_loop = engine.rollout_linear(w.actions, w.mu0, w.S0, w.include_time, w.time0)
    closed = engine.rollout_linear_feedback(w.actions, _gains(w, 411), w.mu0, w.S0, w.include_time, w.time0)
    assert torch.equal(closed["mu"], open_loop["mu"])                    # the gains never move the mean
    assert not torch.equal(closed["Sig"], open_loop["Sig"])
    # gains = NULL at the ABI: the call is gpmpc_rollout_linear
    none = {k: torch.full_like(v, float("nan")) for k, v in open_loop.items()}
    acts = engine._dev(w.actions)
    mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
    for per_candidate in (0, 1):
        rc = engine.lib.gpmpc_rollout_linear_feedback(
            engine._h, acts.data_ptr(), None, per_candidate, mu0.ctypes.data, S0.ctypes.data, 65, 5, A, int(time), float(w.time0),
            none["mu"].data_ptr(), none["Sig"].data_ptr(), none["cost_mu"].data_ptr(), none["cost_var"].data_ptr(),
            none["J"].data_ptr(), engine._stream())
        assert rc == 0
        for k in KEYS:
            assert torch.equal(none[k], open_loop[k]), (k, per_candidate)
    via_engine = engine.rollout_linear_feedback(w.actions, None, w.mu0, w.S0, w.include_time, w.time0)
    for k in KEYS:
        assert torch.equal(via_engine[k], open_loop[k]), k
    # all-zero gains run the closed-loop kernels: well-conditioned D x D sums of at most ~4 D fused operations per element
    zero = engine.rollout_linear_feedback(w.actions, np.zeros((5, A, 3)), w.mu0, w.S0, w.include_time, w.time0)
    assert torch.equal(zero["mu"], open_loop["mu"])
    S_open = _np(open_loop["Sig"])
    assert np.max(np.abs(_np(zero["Sig"]) - S_open)) <= 1e-12 * np.max(np.abs(S_open))
    assert rel_err(_np(zero["cost_mu"]), _np(open_loop["cost_mu"])) < 1e-12
    assert rel_err(_np(zero["cost_var"]), _np(open_loop["cost_var"])) < 1e-11
    assert rel_err(_np(zero["J"]), _np(open_loop["J"])) < 1e-11


# -- 3. costs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip,constraints", [(False, False), (True, False), (False, True), (True, True)])
def test_costs_match_the_host_mapper(engine, clip, constraints):
    w = _workload(50, 5, 65, False, seed=420, A=2)
    w.kappa = 3.0
    _prepared(engine, w)
    K = _gains(w, 421)
    smin, smax = (np.full(3, 0.05), np.full(3, 0.9)) if constraints else (None, None)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa, clip, smin, smax)
    try:
        out = engine.rollout_linear_feedback(w.actions, K, w.mu0, w.S0)
        cfg = lin.reward_config_of(w, clip, smin, smax)
        cm, cv, J = fb.costs(cfg, _np(out["mu"]), _np(out["Sig"]), w.actions, K)
        cm_open, _, _ = lin.costs(cfg, _np(out["mu"]), _np(out["Sig"]), w.actions)
        errs = {"cost_mu": rel_err(_np(out["cost_mu"]), cm), "cost_var": rel_err(_np(out["cost_var"]), cv),
                "J": rel_err(_np(out["J"]), J), "gains_move_cost_mu_by": rel_err(cm_open, cm)}
        print(clip, constraints, errs)
        # the device cost kernel against the host mapper on the SAME trajectory: fp64 rounding of O((D + A)^3) sums
        assert errs["cost_mu"] < 1e-12
        assert errs["cost_var"] < 1e-11
        assert errs["J"] < 1e-11
        assert errs["gains_move_cost_mu_by"] > 1e-9                       # (the action block of Sigma_z is felt)
        # the objective alone, without the caller keeping the trajectory: the same bits
        J_only = engine.rollout_linear_feedback(w.actions, K, w.mu0, w.S0, trajectories=False, stage_costs=False,
                                                out={"J": torch.empty(65, dtype=torch.float64, device=engine.device)})
        assert torch.equal(J_only["J"], out["J"])
    finally:
        engine.set_cost(w.target, w.W, w.W_T, w.kappa)


# -- 4. the deadbeat gain ----------------------------------------------------------------------------------------------------
def test_deadbeat_gain_leaves_the_model_variance_alone(engine):
    w = synth.make_workload(50, 2, 2, 1, 4, seed=2, dynamics="contracting", dense_s0=0.02)
    _prepared(engine, w)
    m0 = np.concatenate([w.mu0, w.actions[0, 0]])
    mom = engine.moments_linear(m0[None])
    V, v = _np(mom["V"])[0], np.diag(_np(mom["S"])[0])
    Vs, Vu = V[:2], V[2:4]
    K = -np.linalg.solve(Vu.T, (np.eye(2) + Vs).T)                       # I + V_s + K^T V_u = 0
    out = engine.rollout_linear_feedback(w.actions[:1], K, w.mu0, w.S0, stage_costs=False)
    S1 = _np(out["Sig"])[0, 1]
    resid = float(np.max(np.abs(S1 - np.diag(v))))
    record("rollout_linear_feedback_deadbeat", residual=resid, S0=float(np.max(np.abs(w.S0))))
    print("deadbeat residual", resid, "max|S0|", float(np.max(np.abs(w.S0))))
    # the error of C is eps cond(V_u) O(1), cond(V_u) < 5, and enters Sigma_1 as 2 dC Sigma_0: ~1e-15 |S0|
    assert resid <= 1e-12 * np.max(np.abs(w.S0))
    for bad in (-K, K.T):                                                # a wrong sign or a transposed gain leaves O(|S0|)
        Sb = _np(engine.rollout_linear_feedback(w.actions[:1], bad, w.mu0, w.S0, stage_costs=False)["Sig"])[0, 1]
        assert np.max(np.abs(Sb - np.diag(v))) > 1e-2 * np.max(np.abs(w.S0))


# -- 5. bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,time", [(50, True), (300, False)])
def test_batch_chunk_and_layout_invariance(engine, N, time):
    w = _workload(N, 5, 130, time, seed=430 + N, A=2)
    _prepared(engine, w)
    K = _gains(w, 431)
    call = lambda a, k, **kw: engine.rollout_linear_feedback(a, k, w.mu0, w.S0, w.include_time, w.time0, **kw)   # noqa: E731
    full = call(w.actions, K)
    again = call(w.actions, K)
    for k in KEYS:
        assert torch.equal(full[k], again[k]), k
    for i in (0, 63, 64, 129):
        one = call(w.actions[i:i + 1], K[i:i + 1])
        for k in KEYS:
            assert torch.equal(one[k][0], full[k][i]), (k, i)
    perm = np.random.default_rng(432).permutation(130)
    mixed = call(w.actions[perm], K[perm])
    for k in KEYS:
        assert torch.equal(mixed[k], full[k][torch.as_tensor(perm, device=engine.device)]), k
    # one (H, A, D) gain passed shared equals the same gain tiled per candidate, also across chunks
    shared = call(w.actions, K[3])
    tiled = call(w.actions, np.broadcast_to(K[3], K.shape).copy())
    for k in KEYS:
        assert torch.equal(shared[k], tiled[k]), k
    assert torch.equal(shared["Sig"][3], full["Sig"][3]) and not torch.equal(shared["Sig"][4], full["Sig"][4])
    for chunk in (1, 7, 64):
        engine.set_option("moments_linear_chunk_points", chunk)
        try:
            chunked = call(w.actions[:70], K[:70])
            J_only = call(w.actions[:70], K[:70], trajectories=False, stage_costs=False,
                          out={"J": torch.empty(70, dtype=torch.float64, device=engine.device)})
            chunked_shared = call(w.actions[:70], K[3])
        finally:
            engine.set_option("moments_linear_chunk_points", 0)
        for k in KEYS:
            assert torch.equal(chunked[k], full[k][:70]), (k, chunk)
            assert torch.equal(chunked_shared[k], shared[k][:70]), (k, chunk)
        assert torch.equal(J_only["J"], full["J"][:70]), chunk


# -- 6. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_and_no_interference():
    from gp_mpc_amd import _lib as L
    eng = _fresh()
    try:
        w = _workload(50, 3, 4, False, seed=440)
        acts = eng._dev(w.actions)
        gains = eng._dev(_gains(w, 441))
        mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
        mu = torch.empty((4, 4, 3), dtype=torch.float64, device=eng.device)
        Sig = torch.empty((4, 4, 3, 3), dtype=torch.float64, device=eng.device)
        J = torch.empty(4, dtype=torch.float64, device=eng.device)
        hp = lambda a: a.ctypes.data                                        # noqa: E731

        def call(B=4, H=3, A=1, time=0, actions=acts.data_ptr(), m0=hp(mu0), J_ptr=None, g=gains.data_ptr()):
            return eng.lib.gpmpc_rollout_linear_feedback(eng._h, actions, g, 1, m0, hp(S0), B, H, A, time, 0.0, mu.data_ptr(),
                                                         Sig.data_ptr(), None, None, J_ptr, eng._stream())
        assert call() == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        assert call() == L.GPMPC_OK                                          # the plain trajectory needs no cost settings
        assert call(J_ptr=J.data_ptr()) == L.GPMPC_ERR_ARG and "set_cost" in eng.lib.gpmpc_last_error(eng._h).decode()
        with pytest.raises(RuntimeError) as ei:
            eng.rollout_linear_feedback(w.actions, _gains(w, 441), w.mu0, w.S0)
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        for kw in (dict(B=0), dict(H=0), dict(A=-1), dict(A=2), dict(time=1), dict(actions=None), dict(m0=None)):
            assert call(**kw) == L.GPMPC_ERR_ARG, kw
            assert call(g=None, **kw) == L.GPMPC_ERR_ARG, kw                 # ... the errors of gpmpc_rollout_linear
        # gains with A < 1: a model whose inputs are the state alone
        w0 = synth.make_workload(50, 3, 0, 3, 4, seed=442)
        eng.prepare(w0.X, w0.Y, w0.lengthscales, w0.outputscales, w0.noises)
        assert call(A=0, g=None) == L.GPMPC_OK                              # (no action is read: any non-NULL pointer)
        assert call(A=0) == L.GPMPC_ERR_ARG and "A >= 1" in eng.lib.gpmpc_last_error(eng._h).decode()
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        for shape in ((3, 1), (4, 1, 3), (4, 3, 3, 1), (2, 3, 1, 3)):
            with pytest.raises(ValueError):
                eng.rollout_linear_feedback(w.actions, np.zeros(shape), w.mu0, w.S0, stage_costs=False)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        assert call(J_ptr=J.data_ptr()) == L.GPMPC_OK
        # no interference: the other rollouts give the same bits before and after, the gpmpc_last_* state stays
        before = {k: v.clone() for k, v in eng.rollout(w.actions, w.mu0, w.S0).items()}
        before_lin = {k: v.clone() for k, v in eng.rollout_linear(w.actions, w.mu0, w.S0).items()}
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path)
        fb_out = eng.rollout_linear_feedback(w.actions, _gains(w, 441), w.mu0, w.S0)
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path) == state
        after = eng.rollout(w.actions, w.mu0, w.S0)
        after_lin = eng.rollout_linear(w.actions, w.mu0, w.S0)
        for k in before:
            assert torch.equal(before[k], after[k]), k
            assert torch.equal(before_lin[k], after_lin[k]), k
        assert not torch.equal(fb_out["Sig"], before_lin["Sig"])
    finally:
        eng.close()


# -- 7. model and controller ---------------------------------------------------------------------------------------------------
def test_transition_model_feedback_gains(engine):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    w = synth.make_workload(60, 3, 1, 4, 5, seed=450, dense_s0=0.01)
    K = _gains(w, 451)
    model = GpStateTransitionModel(ModelConfig(uncertainty_propagation="linearized"), 3, 1, engine=engine)
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    model.set_cost(lin.reward_config_of(w))
    ref = engine.rollout_linear_feedback(w.actions, K, w.mu0, w.S0)
    out = model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 4, 0, feedback_gains=K)
    for k in KEYS:
        assert out[k].device.type == "cuda" and torch.equal(out[k], ref[k]), k
    mu, Sig = model.predict_trajectory(w.actions[2], w.mu0, w.S0, 4, 0, feedback_gains=K[2])
    assert torch.equal(mu, ref["mu"][2].cpu()) and torch.equal(Sig, ref["Sig"][2].cpu())
    assert torch.equal(model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 4, 0)["Sig"],
                       engine.rollout_linear(w.actions, w.mu0, w.S0)["Sig"])
    with pytest.raises(ValueError, match="feedback_gains"):
        model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 4, 0, propagation="moment_matching", feedback_gains=K)
    with pytest.raises(NotImplementedError):
        model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 4, 0, feedback_gains=torch.as_tensor(K).requires_grad_(True))


def test_controller_cem_plans_closed_loop(engine):
    w = synth.make_workload(40, 3, 1, 4, 1, seed=460)
    K = 0.3 * np.random.default_rng(461).standard_normal((4, 1, 3))
    np.random.seed(7)
    c = make_controller(w, optimize=False, engine=engine, shard=False)
    c.config.controller.optimize = True
    c.config.controller.candidate_optimizer = "cem"
    c.config.controller.cem_candidates, c.config.controller.cem_iterations = 16, 2
    c.transition_model.config.uncertainty_propagation = "linearized"
    c.config.controller.feedback_gain = K
    a = c.get_action(obs_mu=w.mu0)
    assert a.shape == (1,) and np.all(np.isfinite(a)) and 0.0 <= float(a[0]) <= 1.0
    assert c.num_rollouts == 32 and np.isfinite(c.best_candidate_J)
    # the cached trajectory is the closed-loop one of the winning sequence
    acts = c.actions_mapper.mpc_to_model_batch(c.actions_mpc_previous_iter[None])
    state_mu, state_var = c.observation_state_mapper.get_state(obs=w.mu0, obs_var=None, update_internals=False)
    ref = engine.rollout_linear_feedback(acts, K, state_mu, state_var)
    assert torch.equal(torch.as_tensor(c.states_mu_pred), ref["mu"][0].cpu())
    assert torch.equal(torch.as_tensor(c.states_var_pred), ref["Sig"][0].cpu())
    assert not torch.equal(ref["Sig"][0], engine.rollout_linear(acts, state_mu, state_var)["Sig"][0])
    c.transition_model.config.uncertainty_propagation = "moment_matching"
    with pytest.raises(ValueError, match="feedback_gain"):
        c.get_action(obs_mu=w.mu0)
