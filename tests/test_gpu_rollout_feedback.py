"""Tier 2 (GPU): gpmpc_rollout_feedback -- the moment-matched horizon rollout in closed loop, under the feedback policy
u = ubar_t + K_t (x - mu_t) -- and its way up through the engine and the transition model.

Checked against the long-double recurrence of tests/feedback_mm_ref.py (the committed oracle's moment_match_step fed the policy's
full input covariance), against gpmpc_rollout at zero gains, against the host SetpointStateRewardMapper._quadratic with the full
state-action covariance for the costs, and against the contracts of include/gpmpc.h: exact symmetry, bitwise invariance to the
batch, both chunk options and the gain layout, errors, no interference.

Tolerances.  Trajectory against long double: 1e-9 max|mu| and 1e-5 max|Sig|, what tests/test_gpu_moments.py holds gpmpc_moments
to.  Zero gains against gpmpc_rollout: mu 1e-10, Sig 1e-6 at H = 1 (test_state_block_matches_one_rollout_step) and 1e-5 over the
horizon; the costs follow from those: cost_mu is linear in Sig (1e-5), cost_var quadratic in it and J goes through both (2e-5).
Costs against the host mapper on the GPU's own trajectory: those of test_costs_match_the_host_mapper in
tests/test_gpu_rollout_linear_feedback.py (the same cost kernel).
"""
import numpy as np
import pytest
import torch

import feedback_mm_ref as fm
import linear_moments_ref as lin
from helpers import rel_err, record
from oracle import gpmpc_oracle as orc
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
    return synth.make_workload(N, D, A, H, B, include_time=time, seed=seed, time0=3.0, dynamics="contracting", dense_s0=0.02)


def _gains(w, seed):
    N, D, A, E, H, B = w.dims
    return np.random.default_rng(seed).standard_normal((B, H, A, D))


def _prepared(engine, w):
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)


def _null_gains_call(engine, w, per_candidate=0):
    """gains = NULL at the ABI, every output requested."""
    N, D, A, E, H, B = w.dims
    out = {"mu": (B, H + 1, D), "Sig": (B, H + 1, D, D), "cost_mu": (B, H + 1), "cost_var": (B, H + 1), "J": (B,)}
    out = {k: torch.full(s, float("nan"), dtype=torch.float64, device=engine.device) for k, s in out.items()}
    acts = engine._dev(w.actions)
    mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
    rc = engine.lib.gpmpc_rollout_feedback(
        engine._h, acts.data_ptr(), None, per_candidate, mu0.ctypes.data, S0.ctypes.data, B, H, A, int(w.include_time),
        float(w.time0), out["mu"].data_ptr(), out["Sig"].data_ptr(), out["cost_mu"].data_ptr(), out["cost_var"].data_ptr(),
        out["J"].data_ptr(), engine._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out


# -- 1. the long-double recurrence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(fm.CASES))
def test_trajectory_against_extended_precision(engine, case):
    D, A, N, H, B, time = fm.CASES[case]
    w, K = fm.case_workload(case)
    _prepared(engine, w)
    out = engine.rollout_feedback(w.actions, K, w.mu0, w.S0, w.include_time, w.time0)
    mu, Sig = _np(out["mu"]), _np(out["Sig"])
    sel, mu_ld, Sig_ld = fm.case_extended(case)
    errs = {"mu": float(np.max(np.abs(mu[sel] - mu_ld)) / np.max(np.abs(mu_ld))),
            "Sig": float(np.max(np.abs(Sig[sel] - Sig_ld)) / np.max(np.abs(Sig_ld)))}
    record(f"rollout_feedback_extended[{case}]", **errs)
    print(case, errs)
    assert np.array_equal(mu[:, 0], np.broadcast_to(w.mu0, (B, D))) and np.array_equal(Sig[:, 0], np.broadcast_to(w.S0, (B, D, D)))
    assert torch.equal(out["Sig"][:, 1:], out["Sig"][:, 1:].transpose(2, 3))           # exactly symmetric
    assert errs["mu"] <= fm.MU_TOL and errs["Sig"] <= fm.SIG_TOL, errs


# -- 2. zero gains: gpmpc_rollout to rounding, as an array and as NULL ---------------------------------------------------------
@pytest.mark.parametrize("case,sig_tol", [("a_d3_a1_n50_h1_b65", 1e-6), ("d_d3_a2_n130_h5_b65_time", 1e-5)])
def test_zero_gains_against_the_open_loop_rollout(engine, case, sig_tol):
    D, A, N, H, B, time = fm.CASES[case]
    w, _ = fm.case_workload(case)
    _prepared(engine, w)
    open_loop = {k: _np(v) for k, v in engine.rollout(w.actions, w.mu0, w.S0, w.include_time, w.time0).items()}
    zero = engine.rollout_feedback(w.actions, np.zeros((H, A, D)), w.mu0, w.S0, w.include_time, w.time0)
    errs = {k: rel_err(_np(zero[k]), open_loop[k]) for k in KEYS}
    record(f"rollout_feedback_zero_gains[{case}]", **errs)
    print(case, errs)
    assert errs["mu"] <= 1e-10 and errs["Sig"] <= sig_tol, errs
    assert errs["cost_mu"] <= 1e-5 and errs["cost_var"] <= 2e-5 and errs["J"] <= 2e-5, errs
    for per_candidate in (0, 1):
        null = _null_gains_call(engine, w, per_candidate)
        for k in KEYS:
            assert torch.equal(null[k], zero[k]), (k, per_candidate)
    via_engine = engine.rollout_feedback(w.actions, None, w.mu0, w.S0, w.include_time, w.time0)
    tiled = engine.rollout_feedback(w.actions, np.zeros((B, H, A, D)), w.mu0, w.S0, w.include_time, w.time0)
    for k in KEYS:
        assert torch.equal(via_engine[k], zero[k]) and torch.equal(tiled[k], zero[k]), k


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
        out = engine.rollout_feedback(w.actions, K, w.mu0, w.S0)
        cfg = lin.reward_config_of(w, clip, smin, smax)
        cm, cv, J = fm.costs(cfg, _np(out["mu"]), _np(out["Sig"]), w.actions, K)
        cm_open, _, _ = lin.costs(cfg, _np(out["mu"]), _np(out["Sig"]), w.actions)
        errs = {"cost_mu": rel_err(_np(out["cost_mu"]), cm), "cost_var": rel_err(_np(out["cost_var"]), cv),
                "J": rel_err(_np(out["J"]), J), "gains_move_cost_mu_by": rel_err(cm_open, cm)}
        print(clip, constraints, errs)
        assert errs["cost_mu"] < 1e-12
        assert errs["cost_var"] < 1e-11
        assert errs["J"] < 1e-11
        assert errs["gains_move_cost_mu_by"] > 1e-9                       # (the action block of Sigma_z is felt)
    finally:
        engine.set_cost(w.target, w.W, w.W_T, w.kappa)


# -- 4. bits -------------------------------------------------------------------------------------------------------------------
def test_batch_chunk_and_layout_invariance(engine):
    w = _workload(50, 5, 130, True, seed=480, A=2)
    _prepared(engine, w)
    K = _gains(w, 481)
    call = lambda a, k, **kw: engine.rollout_feedback(a, k, w.mu0, w.S0, w.include_time, w.time0, **kw)   # noqa: E731
    J_of = lambda a, k: call(a, k, trajectories=False, stage_costs=False,                                 # noqa: E731
                             out={"J": torch.empty(a.shape[0], dtype=torch.float64, device=engine.device)})["J"]
    full = call(w.actions, K)
    again = call(w.actions, K)
    for k in KEYS:
        assert torch.equal(full[k], again[k]), k
    for i in (0, 7, 8, 64, 129):                                          # alone and in the batch
        one = call(w.actions[i:i + 1], K[i:i + 1])
        for k in KEYS:
            assert torch.equal(one[k][0], full[k][i]), (k, i)
    rev = call(w.actions[::-1].copy(), K[::-1].copy())                    # the reversed batch
    for k in KEYS:
        assert torch.equal(rev[k], full[k].flip(0)), k
    # one (H, A, D) gain passed shared equals the same gain tiled per candidate
    shared = call(w.actions, K[3])
    tiled = call(w.actions, np.broadcast_to(K[3], K.shape).copy())
    for k in KEYS:
        assert torch.equal(shared[k], tiled[k]), k
    assert torch.equal(shared["Sig"][3], full["Sig"][3]) and not torch.equal(shared["Sig"][4], full["Sig"][4])
    # trajectories NULL: J keeps its bits
    assert torch.equal(J_of(w.actions, K), full["J"])
    for option, values in (("rollout_feedback_chunk_points", (1, 7, 64)), ("moments_chunk_points", (3,))):
        for chunk in values:
            engine.set_option(option, chunk)
            try:
                chunked = call(w.actions[:70], K[:70])
                J_only = J_of(w.actions[:70], K[:70])
                chunked_shared = call(w.actions[:70], K[3])
            finally:
                engine.set_option(option, 0)
            for k in KEYS:
                assert torch.equal(chunked[k], full[k][:70]), (k, option, chunk)
                assert torch.equal(chunked_shared[k], shared[k][:70]), (k, option, chunk)
            assert torch.equal(J_only, full["J"][:70]), (option, chunk)
    engine.set_option("rollout_feedback_chunk_points", 7)                  # both at once
    engine.set_option("moments_chunk_points", 3)
    try:
        both = call(w.actions[:20], K[:20])
    finally:
        engine.set_option("rollout_feedback_chunk_points", 0)
        engine.set_option("moments_chunk_points", 0)
    for k in KEYS:
        assert torch.equal(both[k], full[k][:20]), k


# -- 5. errors and no interference ---------------------------------------------------------------------------------------------
def test_errors_and_no_interference():
    from gp_mpc_amd import _lib as L
    eng = _fresh()
    try:
        w = _workload(50, 3, 4, False, seed=440)
        acts = eng._dev(w.actions)
        gains = eng._dev(_gains(w, 441))
        mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=eng.device)      # noqa: E731
        mu, Sig, cm, cv, J = nan(4, 4, 3), nan(4, 4, 3, 3), nan(4, 4), nan(4, 4), nan(4)
        hp = lambda a: a.ctypes.data                                        # noqa: E731

        def call(B=4, H=3, A=1, time=0, actions=acts.data_ptr(), m0=hp(mu0), s0=hp(S0), costs=False, g=gains.data_ptr()):
            c = (cm.data_ptr(), cv.data_ptr(), J.data_ptr()) if costs else (None, None, None)
            return eng.lib.gpmpc_rollout_feedback(eng._h, actions, g, 1, m0, s0, B, H, A, time, 0.0, mu.data_ptr(), Sig.data_ptr(),
                                                  *c, eng._stream())

        def untouched():
            torch.cuda.synchronize()
            return all(bool(torch.isnan(t).all()) for t in (mu, Sig, cm, cv, J))

        assert call() == L.GPMPC_ERR_ARG and "prepare" in eng.lib.gpmpc_last_error(eng._h).decode()       # no cached model
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        assert call(costs=True) == L.GPMPC_ERR_ARG and "set_cost" in eng.lib.gpmpc_last_error(eng._h).decode()
        with pytest.raises(RuntimeError) as ei:
            eng.rollout_feedback(w.actions, _gains(w, 441), w.mu0, w.S0)
        assert type(ei.value).__name__ == "GpmpcError" and ei.value.code == L.GPMPC_ERR_ARG
        for kw in (dict(B=0), dict(H=0), dict(A=-1), dict(A=2), dict(time=1), dict(actions=None), dict(m0=None), dict(s0=None)):
            assert call(**kw) == L.GPMPC_ERR_ARG, kw
            assert call(g=None, **kw) == L.GPMPC_ERR_ARG, kw
        assert untouched()
        # gains with A < 1: a model whose inputs are the state alone
        w0 = synth.make_workload(50, 3, 0, 3, 4, seed=442)
        eng.prepare(w0.X, w0.Y, w0.lengthscales, w0.outputscales, w0.noises)
        assert call(A=0) == L.GPMPC_ERR_ARG and "A >= 1" in eng.lib.gpmpc_last_error(eng._h).decode()
        assert untouched()
        assert call(A=0, g=None) == L.GPMPC_OK                              # (no action is read: any non-NULL pointer)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(mu).all()) and bool(torch.isfinite(Sig).all()) and bool(torch.isnan(J).all())
        mu.fill_(float("nan"))
        Sig.fill_(float("nan"))
        # (the compiled limits D <= GPMPC_MAX_D, E <= GPMPC_MAX_E cannot be exceeded by a cached model: gpmpc_prepare refuses it)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        assert call() == L.GPMPC_OK                                          # the plain trajectory needs no cost settings
        for shape in ((3, 1), (4, 1, 3), (4, 3, 3, 1), (2, 3, 1, 3)):
            with pytest.raises(ValueError):
                eng.rollout_feedback(w.actions, np.zeros(shape), w.mu0, w.S0, stage_costs=False)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        assert call(costs=True) == L.GPMPC_OK
        # no interference: the other entries give the same bits before and after, the gpmpc_last_* state stays
        K = _gains(w, 441)
        m_in = np.concatenate([np.tile(w.mu0, (4, 1)), w.actions[:, 0]], axis=1)
        v_in = np.zeros((4, 4, 4))
        v_in[:, :3, :3] = w.S0

        def others():
            res = [eng.rollout(w.actions, w.mu0, w.S0), eng.rollout_linear_feedback(w.actions, K, w.mu0, w.S0),
                   eng.moments(m_in, v_in)]
            return [{k: v.clone() for k, v in r.items()} for r in res]
        before = others()
        state = (eng.last_rollout_path, eng.last_cluster, eng.last_pair_groups, eng.last_prepare_mode, eng.last_grad_path)
        fb_out = eng.rollout_feedback(w.actions, K, w.mu0, w.S0)
        assert (eng.last_rollout_path, eng.last_cluster, eng.last_pair_groups, eng.last_prepare_mode, eng.last_grad_path) == state
        for b, a in zip(before, others()):
            for k in b:
                assert torch.equal(b[k], a[k]), k
        assert not torch.equal(fb_out["Sig"], before[0]["Sig"]) and not torch.equal(fb_out["mu"], before[0]["mu"])
    finally:
        eng.close()


# -- 6. plumbing ---------------------------------------------------------------------------------------------------------------
def test_lqr_form_and_transition_model(engine):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    w = synth.make_workload(60, 3, 1, 4, 5, seed=450, dense_s0=0.01)
    K = _gains(w, 451)
    for propagation in ("moment_matching", "linearized"):                  # always moment-matched
        model = GpStateTransitionModel(ModelConfig(uncertainty_propagation=propagation), 3, 1, engine=engine)
        model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
        model.set_cost(lin.reward_config_of(w))
        # rollout_feedback_lqr is lqr_gains followed by rollout_feedback
        fused = engine.rollout_feedback_lqr(w.actions, w.mu0, w.S0, reg=0.25)
        g = engine.lqr_gains(w.actions, w.mu0, reg=0.25)["gains"]
        apart = engine.rollout_feedback(w.actions, g, w.mu0, w.S0)
        assert torch.equal(fused["gains"], g) and bool(torch.any(g != 0))
        for k in KEYS:
            assert torch.equal(fused[k], apart[k]), k
        # the model methods are the engine's calls
        ref = engine.rollout_feedback(w.actions, K, w.mu0, w.S0)
        out = model.predict_trajectory_feedback_batch(w.actions, K, w.mu0, w.S0, 4, 0)
        for k in KEYS:
            assert out[k].device.type == "cuda" and torch.equal(out[k], ref[k]), k
        mu, Sig = model.predict_trajectory_feedback(w.actions[2], K[2], w.mu0, w.S0, 4, 0)
        assert torch.equal(mu, ref["mu"][2].cpu()) and torch.equal(Sig, ref["Sig"][2].cpu())
        out = model.predict_trajectory_feedback_batch(w.actions, "lqr", w.mu0, w.S0, 4, 0, lqr_reg=0.25)
        for k in KEYS + ("gains",):
            assert torch.equal(out[k], fused[k]), k
        with pytest.raises(NotImplementedError):
            model.predict_trajectory_feedback_batch(w.actions, torch.as_tensor(K).requires_grad_(True), w.mu0, w.S0, 4, 0)
    mm = GpStateTransitionModel(ModelConfig(), 3, 1, engine=engine)
    with pytest.raises(ValueError, match="feedback_gains"):
        mm.predict_trajectory_batch(w.actions, w.mu0, w.S0, 4, 0, stage_costs=False, feedback_gains=K)


def test_on_a_sparse_model(engine):
    D, A, N, H, B, M = 3, 2, 130, 5, 9, 32
    w = _workload(N, H, B, True, seed=470, D=D, A=A)
    K = _gains(w, 471)
    Z = np.ascontiguousarray(w.X[::4][:M])
    engine.prepare_sparse(w.X, w.Y, Z, w.lengthscales, w.outputscales, w.noises)
    try:
        iK, beta = (_np(t) for t in engine.factors())
        assert iK.shape == (D, M, M)
        f = orc.Factors(Z, np.zeros((M, D)), w.lengthscales, w.outputscales, w.noises, iK=iK, beta=beta)
        out = engine.rollout_feedback(w.actions, K, w.mu0, w.S0, w.include_time, w.time0, stage_costs=False)
        mu, Sig = fm.rollout(f, w.actions, K, w.mu0, w.S0, w.include_time, w.time0)
        errs = {"mu": float(np.max(np.abs(_np(out["mu"]) - mu)) / np.max(np.abs(mu))),
                "Sig": float(np.max(np.abs(_np(out["Sig"]) - Sig)) / np.max(np.abs(Sig)))}
        record("rollout_feedback_sparse", **errs)
        print(errs)
        assert np.all(np.isfinite(Sig)) and errs["mu"] <= fm.MU_TOL and errs["Sig"] <= fm.SIG_TOL, errs
    finally:
        engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
