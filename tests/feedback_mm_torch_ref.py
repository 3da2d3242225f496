"""fp64 torch restatement of the closed-loop moment-matched rollout of tests/feedback_mm_ref.py -- a port of
oracle.gpmpc_oracle.moment_match_step at a full input covariance, the rollout under u = ubar_t + K_t (x - mu_t), the closed-loop
costs of tests/feedback_rollout_torch_ref.costs -- so that torch autograd gives the vector-Jacobian products wrt the actions, the
gains and the initial state; and a numpy statement of the reverse sweep that gpmpc_rollout_feedback_backward implements
(include/gpmpc.h).  TEST CODE ONLY.

Conventions of the entry: gains_bar is (B, H, A, D), per candidate, whatever the layout of the gains; the covariance gradients are
symmetric parts; clip_lower_bound_cost_to_0 is pass-through for J; the time input is not differentiated.
"""
import math

import numpy as np
import torch

import feedback_rollout_torch_ref as fbt
import linear_moments_torch_ref as ref
from feedback_rollout_torch_ref import broadcast_gains, costs  # noqa: F401  (costs: re-exported for the tests)
from linear_moments_torch_ref import T64, _t, factors_t  # noqa: F401


# -- the forward, in torch -------------------------------------------------------------------------------------------------------
def step(X, ls, os_, iK, beta, m, s):
    """oracle.gpmpc_oracle.moment_match_step, line for line: m (P, E), s (P, E, E) -> M (P, D), S (P, D, D), V (P, E, D)."""
    N, E = X.shape
    D = ls.shape[0]
    eye = torch.eye(E, dtype=T64)
    inp = X[None, :, :] - m[:, None, :]
    Ms, Vs = [], []
    for a in range(D):
        iL = 1.0 / ls[a]
        iN = inp * iL
        Bm = iL[None, :, None] * s * iL[None, None, :] + eye
        t = torch.linalg.solve(Bm, iN.transpose(1, 2)).transpose(1, 2)
        lb = torch.exp(-0.5 * torch.sum(iN * t, dim=-1)) * beta[a]
        tiL = t * iL
        c = os_[a] / torch.sqrt(torch.linalg.det(Bm))
        Ms.append(torch.sum(lb, dim=-1) * c)
        Vs.append(torch.einsum('bne,bn->be', tiL, lb) * c[:, None])
    M, V = torch.stack(Ms, dim=1), torch.stack(Vs, dim=2)
    logv = torch.log(os_)
    k = [logv[a] - 0.5 * torch.sum((inp / ls[a]) ** 2, dim=-1) for a in range(D)]
    rows = [[None] * D for _ in range(D)]
    for a in range(D):
        for b in range(a, D):
            R = s * (1.0 / ls[a] ** 2 + 1.0 / ls[b] ** 2)[None, None, :] + eye
            Q = torch.linalg.solve(R, s) / 2.0
            Xa = inp / ls[a] ** 2
            Xb = -inp / ls[b] ** 2
            XaQ = Xa @ Q
            XbQ = Xb @ Q
            Xs = torch.sum(XaQ * Xa, dim=-1)
            X2s = torch.sum(XbQ * Xb, dim=-1)
            maha = -2.0 * (XaQ @ Xb.transpose(1, 2)) + Xs[:, :, None] + X2s[:, None, :]
            Lm = torch.exp(k[a][:, :, None] + k[b][:, None, :] + maha)
            sab = torch.einsum('i,bij,j->b', beta[a], Lm, beta[b])
            if a == b:
                sab = sab - torch.einsum('ij,bij->b', iK[a], Lm)
            sab = sab / torch.sqrt(torch.linalg.det(R))
            if a == b:
                sab = sab + os_[a]
            rows[a][b] = sab
            rows[b][a] = sab
    S = torch.stack([torch.stack(r, dim=1) for r in rows], dim=1) - M[:, :, None] * M[:, None, :]
    return M, S, V


def model_input(mu_t, Sig_t, act_t, K_t, E, include_time, time):
    """mu_t (B, D), Sig_t (B, D, D), act_t (B, A), K_t (B, A, D) -> x (B, E), Sigma_in = G Sig_t G^T (B, E, E), G = [I ; K ; 0]."""
    B, D = mu_t.shape
    A = act_t.shape[1]
    cols = [mu_t, act_t]
    if include_time:
        cols.append(torch.full((B, 1), float(time), dtype=T64))
    G = torch.cat((torch.eye(D, dtype=T64).expand(B, D, D), K_t, torch.zeros((B, E - D - A, D), dtype=T64)), dim=1)
    return torch.cat(cols, dim=1), G @ Sig_t @ G.transpose(1, 2)


def rollout(X, ls, os_, iK, beta, actions, gains, mu0, S0, include_time=False, time0=0.0):
    """actions (B, H, A), gains (B, H, A, D), mu0 (B, D), S0 (B, D, D) torch tensors -> mu (B, H + 1, D), Sig (B, H + 1, D, D):
    tests/feedback_mm_ref.rollout."""
    B, H, A = actions.shape
    D, E = beta.shape[0], X.shape[1]
    mus, Sigs = [mu0], [S0]
    for t in range(H):
        x, s = model_input(mus[-1], Sigs[-1], actions[:, t], gains[:, t], E, include_time, float(time0) + float(t))
        M, S, V = step(X, ls, os_, iK, beta, x, s)
        C = s[:, :D, :] @ V
        mus.append(mus[-1] + M)
        Sigs.append(S + Sigs[-1] + C + C.transpose(1, 2))
    return torch.stack(mus, dim=1), torch.stack(Sigs, dim=1)


def rollout_forward(fa, cfg, actions, gains, mu0, S0, include_time=False, time0=0.0):
    """numpy in, numpy out: mu, Sig and (with cfg) cost_mu, cost_var, J of the torch restatement."""
    ft = factors_t(fa)
    at = _t(actions)
    B, H, A = at.shape
    Kt = _t(broadcast_gains(gains, B, H, A, fa[4].shape[0]))
    mu, Sig = rollout(*ft, at, Kt, _t(mu0).expand(B, -1), _t(S0).expand(B, -1, -1), include_time, time0)
    out = {"mu": mu.numpy(), "Sig": Sig.numpy()}
    if cfg is not None:
        cm, cv, J = costs(cfg, mu, Sig, at, Kt)
        out.update(cost_mu=cm.numpy(), cost_var=cv.numpy(), J=J.numpy())
    return out


# -- autograd ---------------------------------------------------------------------------------------------------------------------
def step_vjp(fa, m, s, M_bar=None, S_bar=None, V_bar=None):
    """Autograd of <M_bar, M> + <S_bar, S> + <V_bar, V> -> mu_bar (P, E), G (P, E, E) as autograd gives it (not symmetrised)."""
    ft = factors_t(fa)
    mt = _t(m).clone().requires_grad_(True)
    st = _t(s).clone().requires_grad_(True)
    M, S, V = step(*ft, mt, st)
    obj = torch.zeros((), dtype=T64)
    for bar, val in ((M_bar, M), (S_bar, S), (V_bar, V)):
        if bar is not None:
            obj = obj + torch.sum(_t(bar) * val)
    gm, gs = torch.autograd.grad(obj, (mt, st))
    return gm.numpy(), gs.numpy()


def rollout_vjp(fa, cfg, actions, gains, mu0, S0, include_time=False, time0=0.0, mu_bar=None, Sig_bar=None, cost_mu_bar=None,
                cost_var_bar=None, J_bar=None):
    """Autograd of sum_t <mu_bar_t, mu_t> + <Sig_bar_t, Sig_t> + cost_mu_bar_t cost_mu_t + cost_var_bar_t cost_var_t + J_bar J
    -> actions_bar (B, H, A), gains_bar (B, H, A, D), mu0_bar (B, D), S0_bar (B, D, D) (symmetric part), numpy."""
    ft = factors_t(fa)
    at = _t(actions).clone().requires_grad_(True)
    B, H, A = at.shape
    Kt = _t(broadcast_gains(gains, B, H, A, fa[4].shape[0])).clone().requires_grad_(True)
    m0 = _t(mu0).expand(B, -1).clone().requires_grad_(True)
    s0 = _t(S0).expand(B, -1, -1).clone().requires_grad_(True)
    mu, Sig = rollout(*ft, at, Kt, m0, s0, include_time, time0)
    obj = torch.zeros((), dtype=T64)
    if mu_bar is not None:
        obj = obj + torch.sum(_t(mu_bar) * mu)
    if Sig_bar is not None:
        obj = obj + torch.sum(_t(Sig_bar) * Sig)
    if cost_mu_bar is not None or cost_var_bar is not None or J_bar is not None:
        cm, cv, J = costs(cfg, mu, Sig, at, Kt)
        for bar, val in ((cost_mu_bar, cm), (cost_var_bar, cv), (J_bar, J)):
            if bar is not None:
                obj = obj + torch.sum(_t(bar) * val)
    grads = torch.autograd.grad(obj, (at, Kt, m0, s0), allow_unused=True)
    ga, gK, gm, gS = (torch.zeros_like(x) if g is None else g for g, x in zip(grads, (at, Kt, m0, s0)))
    return ga.numpy(), gK.numpy(), gm.numpy(), (0.5 * (gS + gS.transpose(1, 2))).numpy()


# -- the reverse sweep, in numpy -----------------------------------------------------------------------------------------------------
def _sym(G):
    return 0.5 * (G + np.swapaxes(G, -1, -2))


def rollout_backward_closed(fa, cost, actions, gains, mu0, S0, include_time=False, time0=0.0, mu_bar=None, Sig_bar=None,
                            cost_mu_bar=None, cost_var_bar=None, J_bar=None):
    """The reverse sweep of gpmpc_rollout_feedback_backward, candidate by candidate -> actions_bar, gains_bar (B, H, A, D),
    mu0_bar, S0_bar.  cost: None or a dict(target, W, W_T, kappa, constraints = None | (smin, smax)).  The step formula of
    gpmpc_moments_backward is `step_vjp` (its symmetric part); everything else -- the chaining over the horizon -- is numpy."""
    X, ls, os_, iK, beta = fa
    ft = factors_t(fa)
    actions = np.asarray(actions, dtype=np.float64)
    B, H, A = actions.shape
    D, E = beta.shape[0], X.shape[1]
    Ks = broadcast_gains(gains, B, H, A, D)
    cost_on = cost_mu_bar is not None or cost_var_bar is not None or J_bar is not None
    a_bar, K_bar, m0_bar, S0_bar = np.zeros((B, H, A)), np.zeros((B, H, A, D)), np.zeros((B, D)), np.zeros((B, D, D))
    for b in range(B):
        # forward, keeping every step's model input and V
        mus, Sigs, xs, ss, Vs, Gs = [np.asarray(mu0, dtype=np.float64)], [np.asarray(S0, dtype=np.float64)], [], [], [], []
        for t in range(H):
            G = np.zeros((E, D))
            G[:D] = np.eye(D)
            G[D:D + A] = Ks[b, t]
            x = np.concatenate([mus[-1], actions[b, t], [time0 + t] if include_time else []])
            s = G @ Sigs[-1] @ G.T
            M, S, V = (v.numpy()[0] for v in step(*ft, _t(x)[None], _t(s)[None]))
            C = s[:D, :] @ V
            xs.append(x)
            ss.append(s)
            Vs.append(V)
            Gs.append(G)
            mus.append(mus[-1] + M)
            Sigs.append(Sigs[-1] + S + C + C.T)

        def seeds(t):
            gm, gS, gu, gK = np.zeros(D), np.zeros((D, D)), np.zeros(A), np.zeros((A, D))
            if cost_on:
                terminal = t == H
                if terminal:
                    W, e, Sz = cost["W_T"], mus[t] - cost["target"][:D], Sigs[t]
                else:
                    G = Gs[t][:D + A]
                    W, e, Sz = cost["W"], np.concatenate([mus[t], actions[b, t]]) - cost["target"], G @ Sigs[t] @ G.T
                TS = W @ Sz
                cv = np.trace(2.0 * TS @ TS) + 4.0 * e @ TS @ W @ e            # the closed-loop cost variance
                wm = (cost_mu_bar[b, t] if cost_mu_bar is not None else 0.0) + (J_bar[b] / (H + 1) if J_bar is not None else 0.0)
                wv = (cost_var_bar[b, t] if cost_var_bar is not None else 0.0) \
                    + (J_bar[b] * (-cost["kappa"] / (2.0 * math.sqrt(cv))) / (H + 1) if J_bar is not None else 0.0)
                arrays = (cost["target"], cost["W"], cost["W_T"])
                if terminal:
                    gm, gS, _ = ref.cost_partials_closed(arrays, mus[t], Sigs[t], None, True, wm, wv, None)
                else:
                    gm, gS, gu, gK = fbt.cost_partials_feedback_closed(arrays, mus[t], Sigs[t], actions[b, t], Ks[b, t], wm, wv,
                                                                       cost.get("constraints"))
            if mu_bar is not None:
                gm = gm + mu_bar[b, t]
            if Sig_bar is not None:
                gS = gS + Sig_bar[b, t]
            return gm, _sym(gS), gu, gK

        lam, Lam, _, _ = seeds(H)
        for t in range(H - 1, -1, -1):
            gm, gS, gu, gK = seeds(t)
            G, V, s = Gs[t], Vs[t], ss[t]
            R = s[:D, :]
            Cb = 2.0 * Lam
            Vb = R.T @ Cb
            Vb[D + A:] = 0.0                                       # the time row
            Rb = Cb @ V.T
            x_bar, P = step_vjp(fa, xs[t][None], s[None], lam[None], Lam[None], Vb[None])
            x_bar, P = x_bar[0], _sym(P[0])
            Rext = np.zeros((E, E))
            Rext[:D] = Rb
            Z = P + _sym(Rext)
            a_bar[b, t] = x_bar[D:D + A] + gu
            K_bar[b, t] = (2.0 * Z @ G @ Sigs[t])[D:D + A] + gK
            lam = lam + x_bar[:D] + gm
            Lam = Lam + _sym(G.T @ Z @ G) + gS
        m0_bar[b], S0_bar[b] = lam, Lam
    return a_bar, K_bar, m0_bar, S0_bar


# -- measured on the CPU by tests/test_feedback_mm_backward_reference.py, which re-measures each figure and holds it to its bound ----
# forward: torch restatement vs numpy feedback_mm_ref.rollout, absolute, the worse of the two cases (bound 1e-10 of max|mu| ~ 0.9
# and of max|Sig| + max outputscale ~ 0.05); measured 1.347e-13, 1.049e-12
FORWARD_CPU_DISCREPANCY = dict(mu=1.4e-13, Sig=1.1e-12)
# the step's vjp vs the reference-autograd goldens moments_grad_full_var*.npz, of each array's maximum (bound 1e-8); measured
# 3.436e-10, 9.242e-11
STEP_GOLDEN_DISCREPANCY = dict(mu_bar=3.4e-10, G=9.2e-11)
# rollout_vjp (trajectory cotangents) vs long-double central differences along one random direction per input, h = 1e-5, of the
# directional derivative (bound 3e-6): the worse of the two cases; measured 1.167e-9, 5.542e-7, 3.119e-11, 4.226e-10
FD_STEP = 1e-5
FD_CPU_DISCREPANCY = dict(actions=1.2e-9, gains=5.5e-7, mu0=3.1e-11, S0=4.2e-10)
# rollout_backward_closed vs rollout_vjp, of each array's maximum, the worst array of the four runs (bound 1e-9); measured 1.333e-10
CLOSED_CPU_DISCREPANCY = 1.3e-10
