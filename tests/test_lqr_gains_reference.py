"""Tier 1 (CPU): the numpy restatement of gpmpc_lqr_gains (tests/lqr_gains_ref.py) -- the yardstick of the GPU tests -- tied to
things it does not define itself: the closed form of a one-step horizon on a torch-autograd Jacobian, the cost-to-go summed from
its definition, first-order optimality of the gains by autograd through that definition, the symmetric part of an asymmetric
weight, the deadbeat gain of the closed-loop rollout's restatement, and the degenerate cost.
"""
import numpy as np
import pytest
import torch

import feedback_rollout_ref as fb
import linear_moments_ref as lin
import linear_moments_torch_ref as lt
import lqr_gains_ref as lq
from oracle import gpmpc_oracle as orc
from oracle import synth

SHAPES = [(3, 1, False), (3, 1, True), (4, 2, False)]          # D, A, time


def _factors(w):
    f = orc.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    return (f.X, f.lengthscales, f.variances, f.iK, f.beta)


def _workload(D, A, H, B, time, seed, N=40):
    return synth.make_workload(N, D, A, H, B, include_time=time, seed=seed, time0=3.0, dynamics="contracting", dense_s0=0.02)


def _weights(D, A, seed, asymmetric=False):
    """A full stage weight with cross terms whose symmetric part is positive definite, and a full terminal weight."""
    rng = np.random.default_rng(seed)
    n = D + A
    G = rng.standard_normal((n, n))
    W = G @ G.T / n + np.eye(n)
    if asymmetric:
        S = rng.standard_normal((n, n))
        W = W + 0.5 * (S - S.T)
    G = rng.standard_normal((D, D))
    W_T = G @ G.T / D + np.eye(D)
    if asymmetric:
        S = rng.standard_normal((D, D))
        W_T = W_T + 0.5 * (S - S.T)
    return W, W_T


# -- 1. H = 1: the closed form on an autograd Jacobian --------------------------------------------------------------------------
@pytest.mark.parametrize("D,A,time", SHAPES)
def test_one_step_gain_is_the_closed_form_on_the_autograd_jacobian(D, A, time):
    w = _workload(D, A, 1, 2, time, seed=501 + D + A)
    fa = _factors(w)
    W, W_T = _weights(D, A, 502)
    reg = 0.25
    K, P, flags = lq.gains(*fa, w.actions, w.mu0, W, W_T, w.include_time, w.time0, reg)
    ft = lt.factors_t(fa)
    for b in range(2):
        def nxt(x, u):                                 # x, u -> x + mean([x | u | time])
            cols = [x, u]
            if time:
                cols.append(torch.full((1,), float(w.time0), dtype=torch.float64))
            M, _, _, _ = lt.step(*ft, torch.cat(cols)[None])
            return x + M[0]
        Aj, Bj = torch.autograd.functional.jacobian(nxt, (torch.as_tensor(w.mu0), torch.as_tensor(w.actions[b, 0])))
        Aj, Bj = Aj.numpy(), Bj.numpy()
        Ws = 0.5 * (W + W.T)
        R, N = Ws[D:, D:], Ws[:D, D:]
        want = -np.linalg.solve(R + Bj.T @ W_T @ Bj + reg * np.eye(A), N.T + Bj.T @ W_T @ Aj)
        assert K.shape == (2, 1, A, D) and flags[b] == 0
        assert np.max(np.abs(K[b, 0] - want)) <= 1e-12 * np.max(np.abs(want)), np.max(np.abs(K[b, 0] - want))
        assert np.array_equal(P[b, 1], W_T)


# -- 2. the cost-to-go from its definition, 3. optimality ------------------------------------------------------------------------
@pytest.mark.parametrize("D,A,time", SHAPES)
def test_cost_to_go_is_the_summed_cost_and_the_gains_are_stationary(D, A, time):
    w = _workload(D, A, 3, 2, time, seed=511 + D + A)
    fa = _factors(w)
    W, W_T = _weights(D, A, 512)
    _, At, Bt = lq.linearisation(*fa, w.actions, w.mu0, w.include_time, w.time0)
    K, P, flags = lq.sweep(At, Bt, W, W_T)
    assert not flags.any()
    t = torch.as_tensor
    for b in range(2):
        P0 = lq.cost_to_go(t(At[b]), t(Bt[b]), t(K[b]), t(W), t(W_T)).numpy()
        assert np.max(np.abs(P0 - P[b, 0])) <= 1e-10 * np.max(np.abs(P[b, 0]))
        assert np.array_equal(P[b], np.transpose(P[b], (0, 2, 1)))

        def grad_at(Kv):
            Kv = t(Kv).clone().requires_grad_(True)
            torch.trace(lq.cost_to_go(t(At[b]), t(Bt[b]), Kv, t(W), t(W_T))).backward()
            return Kv.grad.numpy()
        g0, gs = grad_at(np.zeros_like(K[b])), grad_at(K[b])
        print(D, A, time, "grad at 0: max", np.max(np.abs(g0)), "min", np.min(np.abs(g0)), "at the gains:", np.max(np.abs(gs)))
        # tr P_0 is a smooth function of the gains with its minimum at the sweep's: the gradient there is rounding, ~1e-16 of
        # its size elsewhere times the length of the sums
        assert np.max(np.abs(gs)) <= 1e-9 * np.max(np.abs(g0))
        # every entry of every K_t is felt: six orders above the bound, so that no entry passes by being idle
        assert np.min(np.abs(g0)) >= 1e-3 * np.max(np.abs(g0))
        # ... and a wrong sign or a transposed gain (where the shape allows one) is far from stationary
        assert np.max(np.abs(grad_at(-K[b]))) > 0.5 * np.max(np.abs(g0))
        if D == A:
            assert np.max(np.abs(grad_at(np.transpose(K[b], (0, 2, 1))))) > 1e-3 * np.max(np.abs(g0))


# -- 4. cross terms ---------------------------------------------------------------------------------------------------------------
def test_an_asymmetric_weight_is_its_symmetric_part():
    D, A = 4, 2
    w = _workload(D, A, 3, 2, False, seed=521)
    fa = _factors(w)
    W, W_T = _weights(D, A, 522, asymmetric=True)
    assert not np.allclose(W, W.T) and not np.allclose(W_T, W_T.T)
    K, P, flags = lq.gains(*fa, w.actions, w.mu0, W, W_T)
    Ks, Ps, _ = lq.gains(*fa, w.actions, w.mu0, 0.5 * (W + W.T), 0.5 * (W_T + W_T.T))
    assert np.array_equal(K, Ks) and np.array_equal(P, Ps) and not flags.any()
    # the cross block N is felt, and a one-sided reading of W (its upper or lower triangle doubled) is another matrix
    Wn = 0.5 * (W + W.T)
    Wn[:D, D:] = 0.0
    Wn[D:, :D] = 0.0
    Kn, _, _ = lq.gains(*fa, w.actions, w.mu0, Wn, W_T)
    assert np.max(np.abs(Kn - K)) > 1e-2 * np.max(np.abs(K))
    Wu = np.triu(W) + np.triu(W, 1).T
    Ku, _, _ = lq.gains(*fa, w.actions, w.mu0, Wu, W_T)
    assert np.max(np.abs(Ku - K)) > 1e-3 * np.max(np.abs(K))
    # the definition agrees: the summed cost of the policy under the asymmetric W is P_0
    _, At, Bt = lq.linearisation(*fa, w.actions, w.mu0)
    t = torch.as_tensor
    P0 = lq.cost_to_go(t(At[0]), t(Bt[0]), t(K[0]), t(W), t(W_T)).numpy()
    assert np.max(np.abs(P0 - P[0, 0])) <= 1e-10 * np.max(np.abs(P[0, 0]))


# -- 5. the deadbeat gain of the closed-loop rollout ------------------------------------------------------------------------------
def test_terminal_identity_cost_gives_the_deadbeat_gain():
    w = synth.make_workload(50, 2, 2, 1, 4, seed=2, dynamics="contracting", dense_s0=0.02)       # the workload of the deadbeat test
    fa = _factors(w)
    m0 = np.concatenate([w.mu0, w.actions[0, 0]])
    _, _, V, v = lin.step(*fa, m0[None])
    Vs, Vu = V[0, :2], V[0, 2:4]
    assert np.linalg.cond(Vu) < 5.0
    deadbeat = -np.linalg.solve(Vu.T, (np.eye(2) + Vs).T)
    K, P, flags = lq.gains(*fa, w.actions[:1], w.mu0, np.zeros((4, 4)), np.eye(2))
    # Huu = B^T B has the squared condition of V_u (< 25): rounding of ~25 eps
    assert flags[0] == 0 and np.max(np.abs(K[0, 0] - deadbeat)) <= 1e-12 * np.max(np.abs(deadbeat))
    assert np.max(np.abs(P[0, 0])) <= 1e-12                          # the state is driven to the nominal one: no cost is left
    _, Sig = fb.rollout(*fa, w.actions[:1], K, w.mu0, w.S0)
    resid = float(np.max(np.abs(Sig[0, 1] - np.diag(v[0]))))
    print("deadbeat residual", resid, "max|S0|", float(np.max(np.abs(w.S0))))
    assert resid <= 1e-12 * np.max(np.abs(w.S0))                     # the bound of tests/test_feedback_rollout_reference.py


# -- 6. the degenerate cost -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,A,time", SHAPES)
def test_zero_cost_gives_zero_gains_and_counts_the_lost_pivots(D, A, time):
    w = _workload(D, A, 3, 2, time, seed=531)
    fa = _factors(w)
    Z, ZT = np.zeros((D + A, D + A)), np.zeros((D, D))
    for dtype in (np.float64, np.longdouble):
        K, P, flags = lq.gains(*fa, w.actions, w.mu0, Z, ZT, w.include_time, w.time0, 0.0, dtype=dtype)
        assert np.all(K == 0) and np.all(P == 0) and np.array_equal(flags, [3, 3])
        assert not np.isnan(K).any() and not np.isnan(P).any()
        K, P, flags = lq.gains(*fa, w.actions, w.mu0, Z, ZT, w.include_time, w.time0, 1e-6, dtype=dtype)
        assert np.all(K == 0) and np.all(P == 0) and np.array_equal(flags, [0, 0])


# -- 7. the two dtypes are one recurrence -----------------------------------------------------------------------------------------
def test_float64_and_long_double_agree():
    w = _workload(4, 2, 3, 2, False, seed=541)
    fa = _factors(w)
    W, W_T = _weights(4, 2, 542)
    K, P, _ = lq.gains(*fa, w.actions, w.mu0, W, W_T)
    Kl, Pl, _ = lq.gains(*fa, w.actions, w.mu0, W, W_T, dtype=np.longdouble)
    assert Kl.dtype == np.longdouble and Pl.dtype == np.longdouble
    assert np.max(np.abs(K - Kl)) <= 1e-12 * np.max(np.abs(Kl)) and np.max(np.abs(P - Pl)) <= 1e-12 * np.max(np.abs(Pl))
