"""Tier 1 (CPU): the host layers above gpmpc_rollout_feedback_backward without a GPU.  HipEngine.rollout_feedback_backward and
rollout_feedback_grad run against the recording stand-in for the library of tests/engine_call_cases.py: they hand the C ABI what
rollout_linear_feedback_backward / rollout_linear_feedback_grad hand it for the same arguments (tests/golden/engine_calls.json),
under the new entry's name.  GpStateTransitionModel.feedback_objective_and_gradient_batch runs against the CPU stand-in engine of
tests/feedback_mm_grad_stub_engine.py.
"""
import json
import os

import numpy as np
import pytest
import torch

import engine_call_cases as cases
import feedback_mm_torch_ref as fmt
import linear_moments_ref as lin
from feedback_mm_grad_stub_engine import FeedbackMmGradOracleEngine
from oracle import synth

_GAINS = "feedback gains must have shape (A, D) = (1, 2), (H, A, D) = (3, 1, 2) or (B, H, A, D) = (2, 3, 1, 2), got (3, 2, 1)"
_OLD = {"rollout_linear_feedback_backward": "rollout_feedback_backward", "rollout_linear_feedback_grad": "rollout_feedback_grad"}
MIRRORED = [c for c in cases.CASES if c[3] in _OLD]
ARGS = ["actions", "gains", "gains_per_candidate", "mu0", "S0", "B", "H", "A", "include_time", "time0", "mu_bar", "Sig_bar",
        "cost_mu_bar", "cost_var_bar", "J_bar", "actions_bar_out", "gains_bar_out", "mu0_bar_out", "S0_bar_out", "stream"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "engine_calls.json")) as fh:
        return json.load(fh)


def _run(method, *args, E=3, cost=(cases.D, cases.A), **kw):
    return json.loads(json.dumps(cases.run_case(("", E, cost, method, args, kw))))


# -- 1. the engine -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MIRRORED, ids=[c[0] for c in MIRRORED])
def test_engine_hands_over_what_the_linearised_counterpart_does(case, golden):
    cid, E, cost, method, args, kw = case
    rec = json.loads(json.dumps(cases.run_case((cid, E, cost, _OLD[method], args, kw))))
    want = json.loads(json.dumps(golden[cid]).replace("gpmpc_rollout_linear_feedback", "gpmpc_rollout_feedback"))
    assert rec == want
    assert '"?"' not in json.dumps(rec)


def test_the_21_arguments_in_order():
    rec = _run("rollout_feedback_backward", "@actions", "@gains_BHAD", "@mu0", "@S0", True, 1.5, E=4, mu_bar="@mu_bar",
               Sig_bar="@Sig_bar", cost_mu_bar="@cost_mu_bar", cost_var_bar="@cost_var_bar", J_bar="@J_bar")
    (call,) = rec["calls"]
    assert call["fn"] == "gpmpc_rollout_feedback_backward" and len(call["args"]) + 1 == 21 == len(ARGS) + 1
    got = dict(zip(ARGS, call["args"]))
    B, H, D, A = cases.B, cases.H, cases.D, cases.A
    assert got["actions"] == ["in", "actions"] and got["gains"] == ["in", "gains_BHAD"] and got["gains_per_candidate"] == 1
    assert got["mu0"][:2] == ["host", "mu0"] and got["S0"][:2] == ["host", "S0"]
    assert (got["B"], got["H"], got["A"], got["include_time"], got["time0"]) == (B, H, A, 1, 1.5)
    for k in ("mu_bar", "Sig_bar", "cost_mu_bar", "cost_var_bar", "J_bar"):
        assert got[k] == ["in", k], k
    assert got["actions_bar_out"] == ["out", "actions_bar"] and got["gains_bar_out"] == ["out", "gains_bar"]
    assert got["mu0_bar_out"] == ["out", "mu0_bar"] and got["S0_bar_out"] == ["out", "S0_bar"] and got["stream"] is None
    assert rec["result"] == {"actions_bar": [[B, H, A], "torch.float64"], "gains_bar": [[B, H, A, D], "torch.float64"],
                             "mu0_bar": [[B, D], "torch.float64"], "S0_bar": [[B, D, D], "torch.float64"]}


def test_flags_select_null_outputs_and_shared_gains_are_expanded():
    base = ("@actions", "@gains_AD", "@mu0", "@S0")
    rec = _run("rollout_feedback_backward", *base, J_bar="@J_bar", want_gains=False, want_initial=False)
    got = dict(zip(ARGS, rec["calls"][0]["args"]))
    assert set(rec["result"]) == {"actions_bar"}
    assert got["gains_bar_out"] is None and got["mu0_bar_out"] is None and got["S0_bar_out"] is None
    assert got["gains_per_candidate"] == 0 and got["gains"][:2] == ["dev", [cases.H, cases.A, cases.D]]      # (A, D) -> (H, A, D)
    assert [got[k] for k in ("mu_bar", "Sig_bar", "cost_mu_bar", "cost_var_bar")] == [None] * 4 and got["J_bar"] == ["in", "J_bar"]
    rec = _run("rollout_feedback_backward", *base, want_gains=False)
    got = dict(zip(ARGS, rec["calls"][0]["args"]))
    assert set(rec["result"]) == {"actions_bar", "mu0_bar", "S0_bar"} and got["gains_bar_out"] is None
    assert got["mu0_bar_out"] == ["out", "mu0_bar"] and got["S0_bar_out"] == ["out", "S0_bar"]
    rec = _run("rollout_feedback_backward", *base, want_initial=False)
    assert set(rec["result"]) == {"actions_bar", "gains_bar"}
    # gains None: the zero-gain policy, no gains_bar whatever want_gains says
    rec = _run("rollout_feedback_backward", "@actions", None, "@mu0", "@S0")
    got = dict(zip(ARGS, rec["calls"][0]["args"]))
    assert got["gains"] is None and got["gains_per_candidate"] == 0 and got["gains_bar_out"] is None
    assert set(rec["result"]) == {"actions_bar", "mu0_bar", "S0_bar"}


def test_bad_gains_shape_raises_the_existing_text():
    for method in ("rollout_feedback_backward", "rollout_feedback_grad"):
        rec = _run(method, "@actions", "@bad_gains", "@mu0", "@S0")
        assert rec["raises"] == _GAINS
        assert [c["fn"] for c in rec["calls"]] == []             # a rejected call never reaches the library


def test_grad_is_the_forward_with_J_only_then_the_backward_with_ones():
    rec = _run("rollout_feedback_grad", "@actions", "@gains_HAD", "@mu0", "@S0")
    fwd, bwd = rec["calls"]
    assert fwd["fn"] == "gpmpc_rollout_feedback" and bwd["fn"] == "gpmpc_rollout_feedback_backward"
    assert fwd["args"][-6:-1] == [None, None, None, None, ["out", "J"]]                 # mu, Sig, cost_mu, cost_var, J
    got = dict(zip(ARGS, bwd["args"]))
    assert got["J_bar"] == ["dev", [cases.B], [1.0] * cases.B]
    assert [got[k] for k in ("mu_bar", "Sig_bar", "cost_mu_bar", "cost_var_bar", "mu0_bar_out", "S0_bar_out")] == [None] * 6
    assert got["actions_bar_out"] == ["out", "grad"] and got["gains_bar_out"] == ["out", "gains_grad"]
    assert set(rec["result"]) == {"J", "grad", "gains_grad"}


# -- 2. the model method -----------------------------------------------------------------------------------------------------------
def _model(w, eng, cost=True):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    N, D, A, E, H, B = w.dims
    gp_init = {"noise_covar.noise": list(w.noises), "base_kernel.lengthscale": w.lengthscales.tolist(),
               "outputscale": list(w.outputscales)}
    model = GpStateTransitionModel(ModelConfig(gp_init=gp_init), D, A, engine=eng)
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    if cost:
        model.set_cost(lin.reward_config_of(w))
    return model


def test_model_method_reduces_gains_grad_per_layout():
    w = synth.make_workload(20, 3, 1, 2, 3, seed=45, dynamics="contracting", dense_s0=0.02)
    N, D, A, E, H, B = w.dims
    eng = FeedbackMmGradOracleEngine()
    model = _model(w, eng)
    rng = np.random.default_rng(46)
    fa = eng._factors()
    cfg = eng._reward_config()
    for shape, axes in (((B, H, A, D), None), ((H, A, D), 0), ((A, D), (0, 1))):
        K = rng.standard_normal(shape)
        eng.calls.clear()
        out = model.feedback_objective_and_gradient_batch(w.actions, K, w.mu0, w.S0, 0)
        assert eng.calls[0] == "rollout_feedback_grad" and "lqr_gains" not in eng.calls
        assert np.array_equal(eng.gains_seen[-1], K)             # the gains reach the engine as given
        assert set(out) == {"J", "grad", "gains_grad"}
        assert out["J"].shape == (B,) and out["grad"].shape == (B, H, A) and out["gains_grad"].shape == shape
        ga, gK, _, _ = fmt.rollout_vjp(fa, cfg, w.actions, K, w.mu0, w.S0, J_bar=np.ones(B))
        J = eng.rollout_feedback(w.actions, K, w.mu0, w.S0, trajectories=False)["J"]
        assert torch.equal(out["J"], J)
        assert np.array_equal(out["grad"].numpy(), ga)
        want = gK if axes is None else gK.sum(axis=axes)
        assert np.allclose(out["gains_grad"].numpy(), want, rtol=1e-13, atol=1e-18) and np.any(want)
    # ... which is the gradient of the summed objective wrt the shared gain itself
    K = rng.standard_normal((A, D))
    Kt = torch.tensor(K, requires_grad=True)
    ft = fmt.factors_t(fa)
    at = fmt._t(w.actions)
    mu, Sig = fmt.rollout(*ft, at, Kt.expand(B, H, A, D), fmt._t(w.mu0).expand(B, -1), fmt._t(w.S0).expand(B, -1, -1))
    shared = torch.autograd.grad(fmt.costs(cfg, mu, Sig, at, Kt.expand(B, H, A, D))[2].sum(), Kt)[0].numpy()
    out = model.feedback_objective_and_gradient_batch(w.actions, K, w.mu0, w.S0, 0)
    assert np.max(np.abs(out["gains_grad"].numpy() - shared)) <= 1e-12 * np.max(np.abs(shared))


def test_model_method_refusals():
    w = synth.make_workload(20, 3, 1, 2, 2, seed=47)
    eng = FeedbackMmGradOracleEngine()
    model = _model(w, eng)
    for bad in ("lqr", "LQR", "", None):
        with pytest.raises(ValueError, match="feedback_gains"):
            model.feedback_objective_and_gradient_batch(w.actions, bad, w.mu0, w.S0, 0)
    with pytest.raises(ValueError, match="feedback gains must have shape"):
        model.feedback_objective_and_gradient_batch(w.actions, np.zeros((2, 3, 1)), w.mu0, w.S0, 0)
    assert "rollout_feedback" not in eng.calls and "lqr_gains" not in eng.calls
    bare = _model(w, FeedbackMmGradOracleEngine(), cost=False)
    with pytest.raises(RuntimeError, match="set_cost"):
        bare.feedback_objective_and_gradient_batch(w.actions, np.zeros((1, 3)), w.mu0, w.S0, 0)
    # model-level autograd stays off
    with pytest.raises(NotImplementedError):
        model.predict_trajectory_feedback_batch(torch.as_tensor(w.actions).requires_grad_(True), np.zeros((1, 3)), w.mu0, w.S0, 2, 0)
