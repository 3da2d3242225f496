"""Numpy restatement of gpmpc_lqr_gains (include/gpmpc.h), in a dtype of the caller's choice (float64: what a plain fp64
evaluation rounds to; longdouble: the yardstick), built on tests/linear_moments_ref.step.  TEST CODE ONLY.

Nominal trajectory: model input [mu_t | ubar_t | time0 + t], mu_0 = mu0, mu_{t+1} = mu_t + M; with V (E, D) the mean Jacobian,
    A_t = I + V_s^T (D, D),   B_t = V_u^T (D, A)
Cost: W_s = (W + W^T) / 2 = (Q | N ; N^T | R), P_H = (W_T + W_T^T) / 2.  Sweep, for t = H-1 .. 0:
    F = P_{t+1} A_t,  Huu = R + B_t^T P_{t+1} B_t + reg I,  Hux = N^T + B_t^T F,  K_t = -Huu^-1 Hux,  P_t = Q + A_t^T F + Hux^T K_t
A Cholesky pivot of Huu that is <= 0 or not finite: K_t = 0, P_t = sym(Q + A_t^T F), and the candidate's flag counts the step.
"""
import numpy as np

import linear_moments_ref as lin


def linearisation(X, ls, os_, iK, beta, actions, mu0, include_time=False, time0=0.0, dtype=np.float64):
    """actions (B, H, A) -> mu (B, H + 1, D), A_t (B, H, D, D), B_t (B, H, D, A) along every candidate's nominal trajectory."""
    actions = np.asarray(actions, dtype=dtype)
    B, H, A = actions.shape
    D = np.asarray(beta).shape[0]
    E = np.asarray(X).shape[1]
    mu = np.empty((B, H + 1, D), dtype=dtype)
    At = np.empty((B, H, D, D), dtype=dtype)
    Bt = np.empty((B, H, D, A), dtype=dtype)
    mu[:, 0] = np.asarray(mu0, dtype=dtype)
    for t in range(H):
        m = np.zeros((B, E), dtype=dtype)
        m[:, :D] = mu[:, t]
        m[:, D:D + A] = actions[:, t]
        if include_time:
            m[:, -1] = dtype(time0) + dtype(t)
        M, _, V, _ = lin.step(X, ls, os_, iK, beta, m, None, dtype=dtype)
        mu[:, t + 1] = mu[:, t] + M
        At[:, t] = np.eye(D, dtype=dtype)[None] + np.transpose(V[:, :D, :], (0, 2, 1))
        Bt[:, t] = np.transpose(V[:, D:D + A, :], (0, 2, 1))
    return mu, At, Bt


def cholesky(S):
    """Lower factor of a symmetric matrix in its own dtype, or None at a pivot that is <= 0 or not finite."""
    n = S.shape[0]
    L = np.zeros_like(S)
    for k in range(n):
        d = S[k, k] - np.sum(L[k, :k] * L[k, :k])
        if not (d > 0 and np.isfinite(d)):
            return None
        L[k, k] = np.sqrt(d)
        for i in range(k + 1, n):
            L[i, k] = (S[i, k] - np.sum(L[i, :k] * L[k, :k])) / L[k, k]
    return L


def cho_solve(L, Bm):
    """(L L^T)^-1 Bm by forward and back substitution, in L's dtype."""
    n = L.shape[0]
    Y = np.zeros_like(Bm)
    for i in range(n):
        Y[i] = (Bm[i] - L[i, :i] @ Y[:i]) / L[i, i]
    Xs = np.zeros_like(Bm)
    for i in range(n - 1, -1, -1):
        Xs[i] = (Y[i] - L[i + 1:, i] @ Xs[i + 1:]) / L[i, i]
    return Xs


def sweep(At, Bt, W, W_T, reg=0.0, dtype=np.float64):
    """A_t (B, H, D, D), B_t (B, H, D, A) -> gains (B, H, A, D), P (B, H + 1, D, D), flags (B,)."""
    At, Bt = np.asarray(At, dtype=dtype), np.asarray(Bt, dtype=dtype)
    B, H, D, A = Bt.shape
    W, W_T = np.asarray(W, dtype=dtype), np.asarray(W_T, dtype=dtype)
    half = dtype(0.5)
    Ws = half * (W + W.T)
    Q, N, R = Ws[:D, :D], Ws[:D, D:], Ws[D:, D:]
    K = np.zeros((B, H, A, D), dtype=dtype)
    P = np.empty((B, H + 1, D, D), dtype=dtype)
    flags = np.zeros(B, dtype=np.int32)
    P[:, H] = half * (W_T + W_T.T)
    for b in range(B):
        for t in range(H - 1, -1, -1):
            a, bm, Pn = At[b, t], Bt[b, t], P[b, t + 1]
            F = Pn @ a
            Huu = R + bm.T @ Pn @ bm + dtype(reg) * np.eye(A, dtype=dtype)
            Huu = half * (Huu + Huu.T)
            Hux = N.T + bm.T @ F
            Pt = Q + a.T @ F
            L = cholesky(Huu)
            if L is None:
                flags[b] += 1
            else:
                K[b, t] = -cho_solve(L, Hux)
                Pt = Pt + Hux.T @ K[b, t]
            P[b, t] = half * (Pt + Pt.T)
    return K, P, flags


def gains(X, ls, os_, iK, beta, actions, mu0, W, W_T, include_time=False, time0=0.0, reg=0.0, dtype=np.float64):
    """gpmpc_lqr_gains: actions (B, H, A) -> gains (B, H, A, D), P (B, H + 1, D, D), flags (B,)."""
    _, At, Bt = linearisation(X, ls, os_, iK, beta, actions, mu0, include_time, time0, dtype)
    return sweep(At, Bt, W, W_T, reg, dtype)


def cost_to_go(At, Bt, K, W, W_T):
    """The cost-to-go matrix P_0 of the policy delta u_t = K_t delta x_t FROM ITS DEFINITION, in torch (differentiable in K):
    column i of X_t is the deviation that started as unit vector i, X_{t+1} = (A_t + B_t K_t) X_t, and
    P_0 = sum_t [X_t ; K_t X_t]^T W_s [X_t ; K_t X_t] + X_H^T P_H X_H.  At (H, D, D), Bt (H, D, A), K (H, A, D) of one candidate."""
    import torch
    H, D = At.shape[0], At.shape[1]
    Ws = 0.5 * (W + W.T)
    Xd = torch.eye(D, dtype=At.dtype)
    P0 = torch.zeros((D, D), dtype=At.dtype)
    for t in range(H):
        Z = torch.cat((Xd, K[t] @ Xd), dim=0)
        P0 = P0 + Z.T @ Ws @ Z
        Xd = (At[t] + Bt[t] @ K[t]) @ Xd
    return P0 + Xd.T @ (0.5 * (W_T + W_T.T)) @ Xd
