"""Tier 1 (CPU): the mathematics of gpmpc_rollout_linear_feedback_backward without a GPU.  The fp64 torch restatement of the
closed-loop linearised rollout (tests/feedback_rollout_torch_ref.py) is tied to the numpy one (tests/feedback_rollout_ref.py);
then a numpy statement of the entry's closed form (include/gpmpc.h) is checked against torch autograd of that restatement -- both
fp64 evaluations of the same algebra: 1e-9 of the largest magnitude of each array, the bound of
tests/test_linear_backward_reference.py.  At zero gains the closed form is the open-loop one, and the gains still have a
gradient.  Last, the central-difference figures that the GPU test's bound is built on are re-measured.
"""
import os
import re

import numpy as np
import pytest

import feedback_rollout_ref as fb
import feedback_rollout_torch_ref as fbt
import linear_moments_ref as lin
import linear_moments_torch_ref as ref
from oracle import gpmpc_oracle as orc
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
KEYS = ("actions_bar", "gains_bar", "mu0_bar", "S0_bar")


def _factors(w):
    f = orc.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    return (f.X, f.lengthscales, f.variances, f.iK, f.beta)


def _close(got, want, what, tol=TOL):
    scale = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got - want)))
    print(what, "err", err, "scale", scale)
    assert err <= tol * max(scale, 1e-300), (what, err, scale)


def _workload(D, A, time, seed, N=40, H=3, B=2):
    w = synth.make_workload(N, D, A, H, B, include_time=time, seed=seed, time0=2.0, dynamics="contracting", dense_s0=0.02)
    w.kappa = 2.0
    return w


# -- 0. the interface exists ----------------------------------------------------------------------------------------------------
def test_header_and_bindings_declare_the_entry():
    from gp_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    name = "gpmpc_rollout_linear_feedback_backward"
    assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert name in _lib.SIGNATURES
    # gpmpc_rollout_linear_backward's arguments plus gains_dev, gains_per_candidate and gains_bar_out_dev
    assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES["gpmpc_rollout_linear_backward"][1]) + 3
    assert _lib.ABI_VERSION >= 18


# -- 1. the torch restatement is the numpy one ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,A,time", [(3, 1, False), (3, 1, True), (4, 2, False)])
def test_torch_forward_equals_numpy_restatement(D, A, time):
    w = _workload(D, A, time, seed=61)
    fa = _factors(w)
    K = np.random.default_rng(62).standard_normal((2, 3, A, D))
    cfg = lin.reward_config_of(w)
    out = fbt.rollout_forward(fa, cfg, w.actions, K, w.mu0, w.S0, w.include_time, w.time0)
    mu, Sig = fb.rollout(*fa, w.actions, K, w.mu0, w.S0, w.include_time, w.time0)
    # the scales of tests/test_linear_backward_reference.py: Sig on the scale of the terms v = sigma2 - k^T iK k cancels
    assert float(np.max(np.abs(out["mu"] - mu))) <= 1e-12 * float(np.max(np.abs(mu)))
    assert float(np.max(np.abs(out["Sig"] - Sig))) <= 1e-12 * (float(np.max(np.abs(Sig))) + 1e4 * float(np.max(w.outputscales)) ** 2)
    cm, cv, J = fb.costs(cfg, out["mu"], out["Sig"], w.actions, K)
    for k, x in (("cost_mu", cm), ("cost_var", cv), ("J", J)):
        assert float(np.max(np.abs(out[k] - x))) <= 1e-12 * float(np.max(np.abs(x))), k
    # the shared layouts are the broadcast
    one = fbt.rollout_forward(fa, cfg, w.actions, K[0], w.mu0, w.S0, w.include_time, w.time0)
    assert np.array_equal(one["Sig"][0], out["Sig"][0]) and np.array_equal(one["J"][0], out["J"][0])


# -- 2. the sweep -----------------------------------------------------------------------------------------------------------------
def _bars(mode, rng, B, H, D):
    if mode == "J":
        return dict(J_bar=np.ones(B))
    return dict(mu_bar=rng.standard_normal((B, H + 1, D)), Sig_bar=rng.standard_normal((B, H + 1, D, D)),
                cost_mu_bar=rng.standard_normal((B, H + 1)), cost_var_bar=rng.standard_normal((B, H + 1)),
                J_bar=rng.uniform(0.5, 1.5, size=B))


@pytest.mark.parametrize("mode", ["J", "all", "constraints"])
@pytest.mark.parametrize("D,A,time", [(3, 1, False), (3, 1, True), (4, 2, False)])
def test_sweep_closed_form_against_autograd(D, A, time, mode):
    B, H = 2, 3
    w = _workload(D, A, time, seed=81)
    fa = _factors(w)
    rng = np.random.default_rng(82)
    K = rng.standard_normal((B, H, A, D))                        # gains of scale 1
    smin, smax = (np.full(D, 0.05), np.full(D, 0.9)) if mode == "constraints" else (None, None)
    cfg = lin.reward_config_of(w, False, smin, smax)
    cost = dict(target=w.target, W=w.W, W_T=w.W_T, kappa=w.kappa, constraints=(smin, smax) if smin is not None else None)
    bars = _bars(mode, rng, B, H, D)
    args = (w.actions, K, w.mu0, w.S0, w.include_time, w.time0)
    got = fbt.rollout_backward_closed(fa, cost, *args, **bars)
    want = fbt.rollout_vjp(fa, cfg, *args, **bars)
    for g, x, name in zip(got, want, KEYS):
        _close(g, x, name)
    assert np.array_equal(got[3], np.transpose(got[3], (0, 2, 1)))
    assert np.any(got[1])


def test_stage_cost_partials_with_an_asymmetric_weight():
    """W is not assumed symmetric: the stage partials against autograd of the quadratic cost with a full, asymmetric W."""
    import torch
    rng = np.random.default_rng(90)
    D, A = 3, 2
    n = D + A
    W, target = rng.standard_normal((n, n)), rng.standard_normal(n)
    mu, act, K = rng.standard_normal(D), rng.standard_normal(A), rng.standard_normal((A, D))
    L = rng.standard_normal((D, D))
    Sg = L @ L.T + 0.1 * np.eye(D)
    wm, wv = 0.7, -0.3
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)      # noqa: E731
    mt, St, at, Kt = t(mu), t(Sg), t(act), t(K)
    e = torch.cat((mt, at)) - torch.tensor(target)
    G = torch.cat((torch.eye(D, dtype=torch.float64), Kt), dim=0)
    Sz, Wt = G @ St @ G.T, torch.tensor(W)
    TS = Wt @ Sz
    obj = wm * (torch.trace(Sz @ Wt) + e @ Wt @ e) + wv * (torch.trace(2 * TS @ TS) + 4 * e @ TS @ Wt @ e)
    want = torch.autograd.grad(obj, (mt, St, at, Kt))
    gm, gS, gu, gK = fbt.cost_partials_feedback_closed((target, W, None), mu, Sg, act, K, wm, wv)
    _close(gm, want[0].numpy(), "mu")
    _close(0.5 * (gS + gS.T), 0.5 * (want[1] + want[1].T).numpy(), "Sigma")
    _close(gu, want[2].numpy(), "action")
    _close(gK, want[3].numpy(), "K")


# -- 3. zero gains ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["J", "all"])
def test_zero_gains_are_the_open_loop_and_the_gains_still_have_a_gradient(mode):
    B, H, D, A = 2, 3, 3, 1
    w = _workload(D, A, True, seed=91)
    fa = _factors(w)
    rng = np.random.default_rng(92)
    cfg = lin.reward_config_of(w)
    cost = dict(target=w.target, W=w.W, W_T=w.W_T, kappa=w.kappa, constraints=None)
    bars = _bars(mode, rng, B, H, D)
    Z = np.zeros((B, H, A, D))
    rest = (w.mu0, w.S0, w.include_time, w.time0)
    got = fbt.rollout_backward_closed(fa, cost, w.actions, Z, *rest, **bars)
    open_loop = ref.rollout_backward_closed(fa, cost, w.actions, *rest, **bars)
    for g, x, name in zip((got[0], got[2], got[3]), open_loop, ("actions_bar", "mu0_bar", "S0_bar")):
        _close(g, x, name, 1e-12)
    want = fbt.rollout_vjp(fa, cfg, w.actions, Z, *rest, **bars)
    assert np.max(np.abs(want[1])) > 0 and np.max(np.abs(got[1])) > 0
    _close(got[1], want[1], "gains_bar")


# -- 4. central differences: the figures behind the GPU test's bound --------------------------------------------------------------
def test_central_difference_figures_of_the_shared_case():
    w, K = fbt.fd_workload()
    fa = _factors(w)
    cfg = lin.reward_config_of(w)
    cost = dict(target=w.target, W=w.W, W_T=w.W_T, kappa=w.kappa, constraints=None)
    a_bar, K_bar, _, _ = fbt.rollout_backward_closed(fa, cost, w.actions, K, w.mu0, w.S0, J_bar=np.ones(1))
    h = fbt.FD_STEP

    def J(actions, gains):
        mu, Sig = fb.rollout(*fa, actions, gains, w.mu0, w.S0)
        return fb.costs(cfg, mu, Sig, actions, gains)[2][0]

    def differences(x, which):
        fd = np.zeros(x.size)
        for i in range(x.size):
            hi, lo = x.copy().reshape(-1), x.copy().reshape(-1)
            hi[i] += h
            lo[i] -= h
            hi, lo = hi.reshape(x.shape), lo.reshape(x.shape)
            fd[i] = ((J(hi, K) - J(lo, K)) if which == "actions" else (J(w.actions, hi) - J(w.actions, lo))) / (2 * h)
        return fd.reshape(x.shape)
    for which, x, grad in (("actions", w.actions, a_bar), ("gains", K, K_bar)):
        fd = differences(x, which)
        fig = float(np.max(np.abs(fd - grad)) / np.max(np.abs(fd)))
        print(f"central differences, step {h:g}, {which}: relative discrepancy {fig:.3e} (recorded {fbt.FD_CPU_DISCREPANCY[which]:.3e})")
        assert fig <= fbt.FD_CPU_DISCREPANCY[which], (which, fig)
