"""Tier 2 (GPU): gpmpc_lqr_gains -- the LQR feedback gains of the linearisation along every candidate's nominal trajectory -- and
its way up through the engine, the transition model and the controller.

Checked against the long-double restatement of tests/lqr_gains_ref.py (itself tied to independent derivations by
tests/test_lqr_gains_reference.py) under the accuracy rule of DESIGN.md 4.7 / 4.11.2, against gpmpc_rollout_linear and
gpmpc_rollout_linear_feedback where the entries must compose, and against the contracts of include/gpmpc.h: exact symmetry, bitwise
invariance to the batch, the chunks and the optional outputs, the degenerate cost, errors that write nothing.
"""
import numpy as np
import pytest
import torch

import lqr_gains_ref as lq
from helpers import record, make_controller
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
    # as tests/test_gpu_rollout_linear.py: contracting dynamics, a dense initial covariance
    return synth.make_workload(N, D, A, H, B, include_time=time, seed=seed, time0=3.0, dynamics="contracting", dense_s0=0.02)


def _weights(D, A, seed):
    """A full, ASYMMETRIC stage weight with cross terms whose symmetric part is positive definite, and such a terminal weight."""
    rng = np.random.default_rng(seed)
    n = D + A
    G, S = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    W = G @ G.T / n + np.eye(n) + 0.25 * (S - S.T)
    G, S = rng.standard_normal((D, D)), rng.standard_normal((D, D))
    W_T = G @ G.T / D + np.eye(D) + 0.25 * (S - S.T)
    return W, W_T


def _prepared(engine, w, W=None, W_T=None):
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    engine.set_cost(w.target, w.W if W is None else W, w.W_T if W_T is None else W_T, w.kappa)
    iK, beta = (_np(t) for t in engine.factors())
    return (w.X, w.lengthscales, w.outputscales, iK, beta)


# the smallest shapes that cross each boundary: H = 1 and 3 with and without time, one and two 256-column blocks (N = 50, 300),
# one candidate, a few, more than one 64-row tile (B = 1, 4, 70), A > 1, E > 8, and the compiled limits D = 16, A = 8
CASES = {
    "a_d3_a1_n50_h1_b1": (3, 1, 50, 1, 1, False),
    "b_d3_a1_n50_h1_b4_time": (3, 1, 50, 1, 4, True),
    "c_d3_a1_n50_h3_b70": (3, 1, 50, 3, 70, False),
    "d_d3_a1_n50_h3_b4_time": (3, 1, 50, 3, 4, True),
    "e_d3_a1_n300_h3_b4": (3, 1, 300, 3, 4, False),
    "f_d4_a2_n50_h3_b5": (4, 2, 50, 3, 5, False),
    "g_d6_a2_n50_h2_b2_time": (6, 2, 50, 2, 2, True),
    "h_d16_a8_n50_h2_b2": (16, 8, 50, 2, 2, False),
}


# -- 1. the long-double restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_gains_and_cost_to_go_against_extended_precision(engine, case):
    D, A, N, H, B, time = CASES[case]
    w = _workload(N, H, B, time, seed=600 + N + H + D, D=D, A=A)
    W, W_T = _weights(D, A, 601)
    fa = _prepared(engine, w, W, W_T)
    reg = 0.0 if H == 1 else 1e-3
    out = engine.lqr_gains(w.actions, w.mu0, w.include_time, w.time0, reg, want_cost_to_go=True, want_flags=True)
    K, P, flags = _np(out["gains"]), _np(out["P"]), _np(out["flags"])
    assert K.shape == (B, H, A, D) and P.shape == (B, H + 1, D, D) and flags.shape == (B,) and not flags.any()
    sel = np.unique(np.array([0, B // 2, B - 1]))
    args = (w.actions[sel], w.mu0, W, W_T, w.include_time, w.time0, reg)
    K64, P64, _ = lq.gains(*fa, *args)
    Kld, Pld, fld = lq.gains(*fa, *args, dtype=np.longdouble)
    assert not fld.any()
    errs = {"K_hip": float(np.max(np.abs(K[sel] - Kld))), "K_numpy": float(np.max(np.abs(K64 - Kld))),
            "P_hip": float(np.max(np.abs(P[sel] - Pld))), "P_numpy": float(np.max(np.abs(P64 - Pld)))}
    scale = {"K": float(np.max(np.abs(Kld))), "P": float(np.max(np.abs(Pld)))}
    record(f"lqr_gains_extended[{case}]", K_scale=scale["K"], P_scale=scale["P"], **errs)
    print(case, errs, scale)
    # the rule of DESIGN.md 4.7 / 4.11.2: the HIP evaluation rounds like a plain fp64 evaluation of the same recurrence
    assert errs["K_hip"] <= 3 * max(errs["K_numpy"], 1e-12 * scale["K"]), errs
    assert errs["P_hip"] <= 3 * max(errs["P_numpy"], 1e-12 * scale["P"]), errs
    assert scale["K"] > 1e-3                                               # (gains of a size that a zero output would miss by far)
    assert torch.equal(out["P"], out["P"].transpose(2, 3))                # exactly symmetric, the terminal matrix included
    assert np.array_equal(P[:, H], np.broadcast_to(0.5 * (W_T + W_T.T), (B, D, D)))


# -- 2. bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,time", [(50, True), (300, False)])
def test_batch_chunk_and_output_invariance(engine, N, time):
    w = _workload(N, 3, 70, time, seed=610 + N, A=1)
    W, W_T = _weights(3, 1, 611)
    _prepared(engine, w, W, W_T)
    call = lambda a, **kw: engine.lqr_gains(a, w.mu0, w.include_time, w.time0, 1e-3, **kw)        # noqa: E731
    full = call(w.actions, want_cost_to_go=True, want_flags=True)
    again = call(w.actions, want_cost_to_go=True, want_flags=True)
    for k in ("gains", "P", "flags"):
        assert torch.equal(full[k], again[k]), k
    for i in (0, 63, 64, 69):                                              # alone = at the first / last place of the batch
        one = call(w.actions[i:i + 1], want_cost_to_go=True, want_flags=True)
        for k in ("gains", "P", "flags"):
            assert torch.equal(one[k][0], full[k][i]), (k, i)
    swapped = np.concatenate([w.actions[69:], w.actions[1:69], w.actions[:1]])
    sw = call(swapped, want_cost_to_go=True)
    assert torch.equal(sw["gains"][0], full["gains"][69]) and torch.equal(sw["gains"][69], full["gains"][0])
    assert torch.equal(sw["P"][0], full["P"][69]) and torch.equal(sw["P"][69], full["P"][0])
    # the optional outputs do not change the gains' bits
    assert torch.equal(call(w.actions)["gains"], full["gains"])
    assert torch.equal(call(w.actions, want_flags=True)["gains"], full["gains"])
    for chunk in (1, 3, 0):
        engine.set_option("lqr_gains_chunk_points", chunk)
        try:
            chunked = call(w.actions, want_cost_to_go=True, want_flags=True)
        finally:
            engine.set_option("lqr_gains_chunk_points", 0)
        for k in ("gains", "P", "flags"):
            assert torch.equal(chunked[k], full[k]), (k, chunk)
    # ... nor does the chunking of the per-step pass it shares with gpmpc_moments_linear
    engine.set_option("moments_linear_chunk_points", 7)
    try:
        assert torch.equal(call(w.actions)["gains"], full["gains"])
    finally:
        engine.set_option("moments_linear_chunk_points", 0)


# -- 3. composition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,A,time", [(3, 1, True), (4, 2, False)])
def test_rollout_under_lqr_gains_is_the_two_calls(engine, D, A, time):
    w = _workload(50, 3, 5, time, seed=620 + D, D=D, A=A)
    _prepared(engine, w)
    both = engine.rollout_linear_lqr(w.actions, w.mu0, w.S0, w.include_time, w.time0, reg=1e-3)
    assert set(both) == {"J", "mu", "Sig", "cost_mu", "cost_var", "gains"} and both["gains"].device.type == "cuda"
    gains = engine.lqr_gains(w.actions, w.mu0, w.include_time, w.time0, 1e-3)["gains"]
    closed = engine.rollout_linear_feedback(w.actions, gains, w.mu0, w.S0, w.include_time, w.time0)
    assert torch.equal(both["gains"], gains)
    for k in closed:
        assert torch.equal(both[k], closed[k]), k
    open_loop = engine.rollout_linear(w.actions, w.mu0, w.S0, w.include_time, w.time0)
    assert torch.equal(both["mu"], open_loop["mu"])                        # the nominal trajectory, bit for bit
    assert not torch.equal(both["J"], open_loop["J"])                      # the gains reached the rollout (S0 is dense)
    assert not torch.equal(both["Sig"][:, 1:], open_loop["Sig"][:, 1:])
    # the default regularisation is zero
    assert torch.equal(engine.rollout_linear_lqr(w.actions, w.mu0, w.S0, w.include_time, w.time0)["gains"],
                       engine.lqr_gains(w.actions, w.mu0, w.include_time, w.time0)["gains"])


# -- 4. the degenerate cost ---------------------------------------------------------------------------------------------------------
def test_zero_cost_gives_zero_gains_and_counts_the_lost_pivots(engine):
    w = _workload(50, 3, 4, False, seed=630, D=4, A=2)
    _prepared(engine, w, np.zeros((6, 6)), np.zeros((4, 4)))
    out = engine.lqr_gains(w.actions, w.mu0, reg=0.0, want_cost_to_go=True, want_flags=True)
    assert bool((out["gains"] == 0).all()) and bool((out["P"] == 0).all())
    assert not bool(torch.isnan(out["gains"]).any()) and not bool(torch.isnan(out["P"]).any())
    assert _np(out["flags"]).tolist() == [3] * 4
    out = engine.lqr_gains(w.actions, w.mu0, reg=1e-6, want_cost_to_go=True, want_flags=True)
    assert bool((out["gains"] == 0).all()) and bool((out["P"] == 0).all()) and _np(out["flags"]).tolist() == [0] * 4
    # a weight that is not positive definite in the actions loses its pivots without a NaN, and reg restores them
    W = np.diag([1.0, 1.0, 1.0, 1.0, -50.0, -50.0])
    engine.set_cost(w.target, W, np.eye(4), w.kappa)
    out = engine.lqr_gains(w.actions, w.mu0, want_cost_to_go=True, want_flags=True)
    assert _np(out["flags"]).tolist() == [3] * 4 and bool((out["gains"] == 0).all()) and bool(torch.isfinite(out["P"]).all())
    out = engine.lqr_gains(w.actions, w.mu0, reg=60.0, want_flags=True)
    assert _np(out["flags"]).tolist() == [0] * 4 and bool(torch.isfinite(out["gains"]).all()) and bool((out["gains"] != 0).any())


# -- 5. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    from gp_mpc_amd import _lib as L
    eng = _fresh()
    try:
        w = _workload(50, 3, 4, False, seed=640)
        acts = eng._dev(w.actions)
        mu0 = np.ascontiguousarray(w.mu0)
        K = torch.full((4, 3, 1, 3), float("nan"), dtype=torch.float64, device=eng.device)
        P = torch.full((4, 4, 3, 3), float("nan"), dtype=torch.float64, device=eng.device)
        flags = torch.full((4,), -7, dtype=torch.int32, device=eng.device)

        def call(B=4, H=3, A=1, time=0, reg=0.0, actions=acts.data_ptr(), m0=mu0.ctypes.data, gains=K.data_ptr()):
            return eng.lib.gpmpc_lqr_gains(eng._h, actions, m0, B, H, A, time, 0.0, reg, gains, P.data_ptr(), flags.data_ptr(),
                                           eng._stream())

        def untouched():
            torch.cuda.synchronize()
            return bool(torch.isnan(K).all()) and bool(torch.isnan(P).all()) and bool((flags == -7).all())
        assert call() == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        assert call() == L.GPMPC_ERR_ARG and "set_cost" in eng.lib.gpmpc_last_error(eng._h).decode()      # no cost set
        with pytest.raises(RuntimeError) as ei:
            eng.lqr_gains(w.actions, w.mu0)
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        for kw in (dict(B=0), dict(H=0), dict(A=0), dict(A=-1), dict(A=2), dict(time=1), dict(actions=None), dict(m0=None),
                   dict(gains=None), dict(reg=-1e-3), dict(reg=float("nan")), dict(reg=float("inf"))):
            assert call(**kw) == L.GPMPC_ERR_ARG, kw
        assert untouched()
        # a cost for another (D, A): a model with two actions, the cost still loaded for one
        w2 = _workload(50, 3, 4, False, seed=641, A=2)
        eng.prepare(w2.X, w2.Y, w2.lengthscales, w2.outputscales, w2.noises)
        acts2 = eng._dev(w2.actions)
        assert call(A=2, actions=acts2.data_ptr()) == L.GPMPC_ERR_ARG and "set_cost" in eng.lib.gpmpc_last_error(eng._h).decode()
        # the compiled limit of the sweep: A <= 8
        w9 = synth.make_workload(50, 1, 9, 3, 4, seed=642)
        eng.prepare(w9.X, w9.Y, w9.lengthscales, w9.outputscales, w9.noises)
        eng.set_cost(w9.target, w9.W, w9.W_T, w9.kappa)
        acts9 = eng._dev(w9.actions)
        assert call(A=9, actions=acts9.data_ptr()) == L.GPMPC_ERR_LIMIT
        assert untouched()
        for value in (-1, (1 << 24) + 1):
            assert eng.lib.gpmpc_set_option(eng._h, b"lqr_gains_chunk_points", value) == L.GPMPC_ERR_ARG
        # ... and the call that is in order writes everything, and leaves the other entries and the gpmpc_last_* state alone
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        before = {k: v.clone() for k, v in eng.rollout_linear(w.actions, w.mu0, w.S0).items()}
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path)
        assert call() == L.GPMPC_OK
        torch.cuda.synchronize()
        assert bool(torch.isfinite(K).all()) and bool(torch.isfinite(P).all()) and bool((flags == 0).all())
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_prepare_mode, eng.last_grad_path) == state
        after = eng.rollout_linear(w.actions, w.mu0, w.S0)
        for k in before:
            assert torch.equal(before[k], after[k]), k
    finally:
        eng.close()


# -- 6. model and controller --------------------------------------------------------------------------------------------------------
def test_transition_model_lqr(engine):
    import linear_moments_ref as lin
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    w = synth.make_workload(60, 3, 1, 4, 5, seed=650, dense_s0=0.01)
    model = GpStateTransitionModel(ModelConfig(uncertainty_propagation="linearized"), 3, 1, engine=engine)
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    model.set_cost(lin.reward_config_of(w))
    ref = engine.rollout_linear_lqr(w.actions, w.mu0, w.S0, reg=1e-2)
    out = model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 4, 0, feedback_gains="lqr", lqr_reg=1e-2)
    assert set(out) == set(ref)
    for k in ref:
        assert out[k].device.type == "cuda" and torch.equal(out[k], ref[k]), k
    mu, Sig = model.predict_trajectory(w.actions[2], w.mu0, w.S0, 4, 0, feedback_gains="lqr", lqr_reg=1e-2)
    assert torch.equal(mu, ref["mu"][2].cpu()) and torch.equal(Sig, ref["Sig"][2].cpu())
    with pytest.raises(ValueError, match="feedback_gains"):
        model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 4, 0, propagation="moment_matching", feedback_gains="lqr")
    with pytest.raises(ValueError, match="lqr"):
        model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 4, 0, feedback_gains="dlqr")
    with pytest.raises(NotImplementedError):
        model.predict_trajectory_batch(torch.as_tensor(w.actions).requires_grad_(True), w.mu0, w.S0, 4, 0, feedback_gains="lqr")


def test_controller_random_shooting_plans_under_lqr_gains(engine):
    w = synth.make_workload(50, 3, 1, 3, 1, seed=660)

    def step(gain):
        np.random.seed(7)
        c = make_controller(w, optimize=False, restarts=16, engine=engine, shard=False)
        c.transition_model.config.uncertainty_propagation = "linearized"
        c.config.controller.feedback_gain = gain
        c.config.controller.feedback_lqr_reg = 1e-3
        a = c.get_action(obs_mu=w.mu0)
        return c, a
    c, a = step("lqr")
    assert a.shape == (1,) and np.all(np.isfinite(a)) and 0.0 <= float(a[0]) <= 1.0
    assert c.num_rollouts >= 16
    c_open, a_open = step(None)
    assert np.all(np.isfinite(a_open))
    # random shooting caches the LAST candidate's trajectory, and both runs drew the same candidates: one mean recurrence (the
    # gains never move it), another covariance from the first step on -- the cached trajectory is the closed-loop one
    S_closed, S_open = torch.as_tensor(c.states_var_pred), torch.as_tensor(c_open.states_var_pred)
    assert S_closed.shape == (4, 3, 3) and torch.equal(S_closed[0], S_open[0])
    assert torch.equal(torch.as_tensor(c.states_mu_pred), torch.as_tensor(c_open.states_mu_pred))
    for t in range(1, 4):
        assert not torch.equal(S_closed[t], S_open[t]), t
    assert np.isfinite(float(c.cost_traj_mean_lcb)) and float(c.cost_traj_mean_lcb) != float(c_open.cost_traj_mean_lcb)
