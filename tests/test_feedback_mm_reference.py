"""Tier 1 (CPU): the numpy restatement of the closed-loop moment-matched rollout (tests/feedback_mm_ref.py) -- the yardstick of
the GPU tests of gpmpc_rollout_feedback -- tied to things it does not define itself: the committed open-loop oracle at zero gains
and the long-double oracle on every GPU case.  Then the host plumbing of GpStateTransitionModel.predict_trajectory_feedback(_batch)
with the CPU stand-in engine of tests/feedback_mm_stub_engine.py.
"""
import os
import re

import numpy as np
import pytest
import torch

import feedback_mm_ref as fm
import linear_moments_ref as lin
from feedback_mm_stub_engine import FeedbackMmOracleEngine
from oracle import gpmpc_oracle as orc
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_declared():
    from gp_mpc_amd import _lib
    with open(os.path.join(ROOT, "include", "gpmpc.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint\s+gpmpc_rollout_feedback\s*\(", header) and "gpmpc_rollout_feedback" in _lib.SIGNATURES
    assert _lib.SIGNATURES["gpmpc_rollout_feedback"] == _lib.SIGNATURES["gpmpc_rollout_linear_feedback"]
    assert _lib.ABI_VERSION >= 28


# -- 1. zero gains are the committed open-loop oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("time", [False, True])
def test_zero_gains_reproduce_predict_trajectory(time):
    w = synth.make_workload(40, 3, 2, 4, 3, include_time=time, seed=61, time0=3.0, dynamics="contracting", dense_s0=0.02)
    f = orc.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    mu, Sig = fm.rollout(f, w.actions, np.zeros((4, 2, 3)), w.mu0, w.S0, w.include_time, w.time0)
    mu_o, Sig_o = orc.predict_trajectory(f, w.actions, w.mu0, w.S0, w.include_time, w.time0)
    assert np.max(np.abs(mu - mu_o)) <= 1e-15 and np.max(np.abs(Sig - Sig_o)) <= 1e-15
    # the three gain layouts are one recurrence
    K = np.random.default_rng(62).standard_normal((3, 4, 2, 3))
    mu_k, Sig_k = fm.rollout(f, w.actions, K, w.mu0, w.S0, w.include_time, w.time0)
    mu_s, Sig_s = fm.rollout(f, w.actions[:1], K[0], w.mu0, w.S0, w.include_time, w.time0)
    assert np.allclose(mu_s[0], mu_k[0], rtol=0, atol=1e-14) and np.allclose(Sig_s[0], Sig_k[0], rtol=0, atol=1e-14)
    _, Sig_c = fm.rollout(f, w.actions, K[0, 0], w.mu0, w.S0, w.include_time, w.time0)
    _, Sig_t = fm.rollout(f, w.actions, np.tile(K[0, 0], (3, 4, 1, 1)), w.mu0, w.S0, w.include_time, w.time0)
    assert np.array_equal(Sig_c, Sig_t)


# -- 2. every GPU case: fp64 against long double, and the gains are felt far beyond the GPU tolerance ------------------------
@pytest.mark.parametrize("case", list(fm.CASES))
def test_fp64_recurrence_against_extended_precision(case):
    w, K = fm.case_workload(case)
    sel, mu_ld, Sig_ld = fm.case_extended(case)
    f = orc.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    mu, Sig = fm.rollout(f, w.actions[sel], K[sel], w.mu0, w.S0, w.include_time, w.time0)
    mu_o, Sig_o = orc.predict_trajectory(f, w.actions[sel], w.mu0, w.S0, w.include_time, w.time0)
    s_mu, s_Sig = float(np.max(np.abs(mu_ld))), float(np.max(np.abs(Sig_ld)))
    figures = {"mu_err": float(np.max(np.abs(mu - mu_ld))) / s_mu, "Sig_err": float(np.max(np.abs(Sig - Sig_ld))) / s_Sig,
               "gains_move_mu_by": float(np.max(np.abs(mu - mu_o))) / s_mu,
               "gains_move_Sig_by": float(np.max(np.abs(Sig - Sig_o))) / s_Sig}
    print(case, figures)
    assert np.all(np.isfinite(Sig)) and np.all(np.isfinite(mu))
    assert figures["Sig_err"] <= 1e-6 and figures["mu_err"] <= 1e-11, figures
    # a kernel that ignores the gains or the action block fails by far
    assert figures["gains_move_Sig_by"] >= 100 * fm.SIG_TOL and figures["gains_move_mu_by"] >= 100 * fm.MU_TOL, figures


# -- 3. host logic -------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("propagation", ["moment_matching", "linearized"])
def test_model_methods_dispatch(propagation):
    w = synth.make_workload(20, 3, 1, 2, 2, seed=41)
    eng = FeedbackMmOracleEngine()
    model = _model(w, propagation, eng)                       # always moment-matched, whatever is configured
    f = eng.f
    K = np.random.default_rng(42).standard_normal((2, 2, 1, 3))
    out = model.predict_trajectory_feedback_batch(w.actions, K, w.mu0, w.S0, 2, 0)
    assert eng.calls == ["rollout_feedback"] and set(out) == {"mu", "Sig", "J", "cost_mu", "cost_var"}
    assert np.array_equal(eng.gains_seen[-1], K)
    mu_ref, Sig_ref = fm.rollout(f, w.actions, K, w.mu0, w.S0)
    assert np.array_equal(out["mu"].numpy(), mu_ref) and np.array_equal(out["Sig"].numpy(), Sig_ref)
    # the gain layouts reach the engine as they are
    for gains in (K[0], K[0, 0], torch.as_tensor(K)):
        model.predict_trajectory_feedback_batch(w.actions, gains, w.mu0, w.S0, 2, 0, stage_costs=False)
        assert eng.calls[-1] == "rollout_feedback" and eng.gains_seen[-1].shape == tuple(np.shape(gains))
    # one sequence
    mu, Sig = model.predict_trajectory_feedback(w.actions[1], K[1], w.mu0, w.S0, 2, 0)
    assert eng.calls[-1] == "rollout_feedback" and mu.shape == (3, 3) and Sig.shape == (3, 3, 3)
    assert np.allclose(mu.numpy(), mu_ref[1], rtol=0, atol=1e-14) and np.allclose(Sig.numpy(), Sig_ref[1], rtol=0, atol=1e-14)
    # "lqr": the gain design, then the moment-matched closed loop with (B, H, A, D) gains
    eng.calls.clear()
    out = model.predict_trajectory_feedback_batch(w.actions, "lqr", w.mu0, w.S0, 2, 0, lqr_reg=0.125)
    assert eng.calls == ["lqr_gains", "rollout_feedback"] and eng.regs_seen[-1] == 0.125
    assert set(out) == {"mu", "Sig", "J", "cost_mu", "cost_var", "gains"} and eng.gains_seen[-1].shape == (2, 2, 1, 3)
    assert np.array_equal(out["gains"].numpy(), eng.gains_seen[-1])
    mu, Sig = model.predict_trajectory_feedback(w.actions[0], "lqr", w.mu0, w.S0, 2, 0)
    assert eng.calls[-2:] == ["lqr_gains", "rollout_feedback"] and eng.regs_seen[-1] == 0.0
    assert "rollout_linear_feedback" not in eng.calls and "rollout" not in eng.calls


def test_model_refusals():
    w = synth.make_workload(20, 3, 1, 2, 2, seed=43)
    eng = FeedbackMmOracleEngine()
    model = _model(w, "moment_matching", eng)
    K = np.zeros((2, 1, 3))
    for bad in ("LQR", "ilqr", "", None):
        with pytest.raises(ValueError, match="lqr"):
            model.predict_trajectory_feedback_batch(w.actions, bad, w.mu0, w.S0, 2, 0)
    with pytest.raises(ValueError, match="len_horizon"):
        model.predict_trajectory_feedback_batch(w.actions, K, w.mu0, w.S0, 3, 0)
    ag = torch.as_tensor(w.actions).clone().requires_grad_(True)
    kg = torch.as_tensor(K).clone().requires_grad_(True)
    for args in ((ag, K), (w.actions, kg), (ag, "lqr")):
        with pytest.raises(NotImplementedError):
            model.predict_trajectory_feedback_batch(*args, w.mu0, w.S0, 2, 0)
    with pytest.raises(NotImplementedError):
        model.predict_trajectory_feedback(ag[0], K, w.mu0, w.S0, 2, 0)
    assert eng.calls == []
    with torch.no_grad():
        model.predict_trajectory_feedback_batch(ag, kg, w.mu0, w.S0, 2, 0)
    assert eng.calls == ["rollout_feedback"]
    # costs need set_cost; the gain design too
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    bare = GpStateTransitionModel(ModelConfig(), 3, 1, engine=FeedbackMmOracleEngine())
    bare.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    with pytest.raises(RuntimeError, match="set_cost"):
        bare.predict_trajectory_feedback_batch(w.actions, K, w.mu0, w.S0, 2, 0)
    with pytest.raises(RuntimeError, match="set_cost"):
        bare.predict_trajectory_feedback_batch(w.actions, "lqr", w.mu0, w.S0, 2, 0, stage_costs=False)
    # the existing feedback_gains= argument stays refused under moment matching, and now names the new methods
    eng.calls.clear()
    with pytest.raises(ValueError, match="feedback_gains") as ei:
        model.predict_trajectory_batch(w.actions, w.mu0, w.S0, 2, 0, feedback_gains=K)
    assert "predict_trajectory_feedback" in str(ei.value)
    with pytest.raises(ValueError, match="feedback_gains"):
        model.predict_trajectory(w.actions[0], w.mu0, w.S0, 2, 0, feedback_gains="lqr")
    assert eng.calls == []


def test_engine_gain_layouts():
    from gp_mpc_amd.engine import feedback_gains_layout, HipEngine
    assert feedback_gains_layout((1, 3), 2, 4, 1, 3) == (False, True)
    assert feedback_gains_layout((4, 1, 3), 2, 4, 1, 3) == (False, False)
    assert feedback_gains_layout((2, 4, 1, 3), 2, 4, 1, 3) == (True, False)
    for shape in ((3, 1), (2, 1, 3), (2, 4, 3, 1)):
        with pytest.raises(ValueError, match="feedback gains"):
            feedback_gains_layout(shape, 2, 4, 1, 3)
    assert callable(HipEngine.rollout_feedback) and callable(HipEngine.rollout_feedback_lqr)
