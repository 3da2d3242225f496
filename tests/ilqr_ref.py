"""Numpy restatement of the clamped iLQR of gpmpc_ilqr_* (include/gpmpc.h), in a dtype of the caller's choice (float64: what a
plain fp64 evaluation rounds to; longdouble: the yardstick), built on tests/lqr_gains_ref.linearisation and
tests/linear_moments_ref.  TEST CODE ONLY.

Dynamics x_{t+1} = x_t + mean(x_t, u_t, t); cost c = (sum_{t<H} e_t^T W_s e_t + e_H^T P_H e_H) / (H + 1), e_t = [x_t | u_t] - target.
Backward sweep, t = H-1 .. 0 (K_t, P_t as lqr_gains_ref.sweep):
    p_H = P_H e_H,  q = W_s e_t,  g_x = q_x + A_t^T p_{t+1},  g_u = q_u + B_t^T p_{t+1},  k_t = -Huu^-1 g_u,  p_t = g_x + Hux^T k_t,
    dV = sum_t g_u^T k_t / (H + 1),  step = max |clip(ubar_t + k_t) - ubar_t|
Forward pass for alpha: u_t = clip(ubar_t + alpha k_t + K_t (x_t - xbar_t)).  The sweep and the forward pass take the dynamics as
arrays / a function, so they run on dynamics that are not a GP.
"""
import numpy as np

import linear_moments_ref as lin
import lqr_gains_ref as lq


def sweep(At, Bt, e, eH, W, W_T, reg=0.0, dtype=np.float64):
    """A_t (B, H, D, D), B_t (B, H, D, A), e (B, H, D + A), eH (B, D), reg a scalar or (B,) -> dict K (B, H, A, D), k (B, H, A),
    P (B, H + 1, D, D), dV (B,) (already / (H + 1)), flags (B,)."""
    At, Bt, e, eH = (np.asarray(v, dtype=dtype) for v in (At, Bt, e, eH))
    B, H, D, A = Bt.shape
    reg = np.broadcast_to(np.asarray(reg, dtype=dtype), (B,))
    W, W_T = np.asarray(W, dtype=dtype), np.asarray(W_T, dtype=dtype)
    half = dtype(0.5)
    Ws = half * (W + W.T)
    Q, N, R = Ws[:D, :D], Ws[:D, D:], Ws[D:, D:]
    K = np.zeros((B, H, A, D), dtype=dtype)
    k = np.zeros((B, H, A), dtype=dtype)
    P = np.empty((B, H + 1, D, D), dtype=dtype)
    dV = np.zeros(B, dtype=dtype)
    flags = np.zeros(B, dtype=np.int32)
    P[:, H] = half * (W_T + W_T.T)
    for b in range(B):
        p = P[b, H] @ eH[b]
        for t in range(H - 1, -1, -1):
            a, bm, Pn = At[b, t], Bt[b, t], P[b, t + 1]
            F = Pn @ a
            Huu = R + bm.T @ Pn @ bm + reg[b] * np.eye(A, dtype=dtype)
            Huu = half * (Huu + Huu.T)
            Hux = N.T + bm.T @ F
            Pt = Q + a.T @ F
            q = Ws @ e[b, t]
            gx = q[:D] + a.T @ p
            gu = q[D:] + bm.T @ p
            L = lq.cholesky(Huu)
            if L is None:
                flags[b] += 1
                p = gx
            else:
                K[b, t] = -lq.cho_solve(L, Hux)
                k[b, t] = -lq.cho_solve(L, gu[:, None])[:, 0]
                Pt = Pt + Hux.T @ K[b, t]
                p = gx + Hux.T @ k[b, t]
                dV[b] += gu @ k[b, t]
            P[b, t] = half * (Pt + Pt.T)
    return {"K": K, "k": k, "P": P, "dV": dV / dtype(H + 1), "flags": flags}


def errors(mu, actions, target, dtype=np.float64):
    """mu (B, H + 1, D), actions (B, H, A) -> e (B, H, D + A), eH (B, D)."""
    mu, actions, target = (np.asarray(v, dtype=dtype) for v in (mu, actions, target))
    D = mu.shape[-1]
    e = np.concatenate([mu[:, :-1], actions], axis=-1) - target
    return e, mu[:, -1] - target[:D]


def cost(mu, actions, target, W, W_T, dtype=np.float64):
    """The certainty-equivalent cost (B,) of stored trajectories."""
    e, eH = errors(mu, actions, target, dtype)
    W, W_T = np.asarray(W, dtype=dtype), np.asarray(W_T, dtype=dtype)
    Ws, PH = dtype(0.5) * (W + W.T), dtype(0.5) * (W_T + W_T.T)
    H = e.shape[1]
    # element-wise products and sums along a trajectory's own axes: the same trajectory gets the same bits in any batch
    stage = np.sum(e[..., :, None] * Ws * e[..., None, :], axis=(-2, -1))
    term = np.sum(eH[..., :, None] * PH * eH[..., None, :], axis=(-2, -1))
    return (np.sum(stage, axis=-1) + term) / dtype(H + 1)


def step_size(actions, k, dtype=np.float64):
    actions, k = np.asarray(actions, dtype=dtype), np.asarray(k, dtype=dtype)
    return np.max(np.abs(np.clip(actions + k, 0, 1) - actions), axis=(1, 2))


def gp_mean(fa, include_time=False, time0=0.0, dtype=np.float64):
    """mean(x (P, D), u (P, A), t) -> M (P, D): the GP posterior mean of the cached factors (X, ls, os, iK, beta)."""
    X, ls, os_, iK, beta = fa

    def mean(x, u, t):
        m = np.concatenate([x, u] + ([np.full((x.shape[0], 1), dtype(time0) + dtype(t), dtype=dtype)] if include_time else []),
                           axis=-1)
        return lin.step(X, ls, os_, iK, beta, m, None, dtype=dtype)[0]      # the very operations of lqr_gains_ref.linearisation
    return mean


def forward(mean, actions, K, k, mu_nom, mu0, alphas, dtype=np.float64, clip=True):
    """The closed-loop forward pass for every step size: dict trial_actions (B, L, H, A), trial_mu (B, L, H + 1, D)."""
    actions, K, k, mu_nom = (np.asarray(v, dtype=dtype) for v in (actions, K, k, mu_nom))
    B, H, A = actions.shape
    D = mu_nom.shape[-1]
    alphas = np.asarray(alphas, dtype=dtype)
    L = alphas.size
    ta = np.empty((B, L, H, A), dtype=dtype)
    tm = np.empty((B, L, H + 1, D), dtype=dtype)
    for l in range(L):
        x = np.broadcast_to(np.asarray(mu0, dtype=dtype), (B, D)).copy()
        tm[:, l, 0] = x
        for t in range(H):
            u = actions[:, t] + alphas[l] * k[:, t] + np.einsum("bad,bd->ba", K[:, t], x - mu_nom[:, t])
            if clip:
                u = np.clip(u, 0, 1)
            ta[:, l, t] = u
            x = x + mean(x, u, t)
            tm[:, l, t + 1] = x
    return {"trial_actions": ta, "trial_mu": tm}


def backward(fa, actions, mu0, target, W, W_T, include_time=False, time0=0.0, reg=0.0, dtype=np.float64):
    """gpmpc_ilqr_backward on the GP of `fa`: dict gains, ff, mu, cost, dV, step, flags."""
    mu, At, Bt = lq.linearisation(*fa, actions, mu0, include_time, time0, dtype)
    e, eH = errors(mu, actions, target, dtype)
    s = sweep(At, Bt, e, eH, W, W_T, reg, dtype)
    return {"gains": s["K"], "ff": s["k"], "mu": mu, "cost": cost(mu, actions, target, W, W_T, dtype), "dV": s["dV"],
            "step": step_size(actions, s["k"], dtype), "flags": s["flags"], "P": s["P"]}


def accept_rule(cost_, trial_cost, step, reg, status, accepts, reg0, reg_factor, reg_max, tol):
    """Steps 2-5 of gpmpc_ilqr_step for every candidate from the numbers given (arrays over the candidates; trial_cost (B, L)):
    -> (chosen, accepts, reg, status, new_cost); chosen = -2 marks a candidate that was finished already (nothing changes)."""
    cost_, step, reg = (np.array(v, dtype=np.float64) for v in (cost_, step, reg))
    status, accepts = np.array(status, dtype=np.int64), np.array(accepts, dtype=np.int64)
    trial_cost = np.asarray(trial_cost, dtype=np.float64)
    chosen = np.full(cost_.shape[0], -2, dtype=np.int64)
    for b in range(cost_.shape[0]):
        if status[b] != 0:
            continue
        chosen[b] = -1
        if not np.isfinite(cost_[b]):
            status[b] = 3
            continue
        if step[b] <= tol:
            status[b] = 1
            continue
        best = -1
        for l in range(trial_cost.shape[1]):
            c = trial_cost[b, l]
            if np.isfinite(c) and (best < 0 or c < trial_cost[b, best]):
                best = l
        if best >= 0 and trial_cost[b, best] < cost_[b]:
            cost_[b] = trial_cost[b, best]
            reg[b] = max(reg[b] / reg_factor, reg0)
            accepts[b] += 1
            chosen[b] = best
        else:
            reg[b] = reg[b] * reg_factor
            if reg[b] > reg_max:
                status[b] = 2
    return chosen, accepts, reg, status, cost_


def init(x0, L, reg0, dtype=np.float64):
    x0 = np.asarray(x0, dtype=dtype)
    B = x0.shape[0]
    return {"actions": np.clip(x0, 0, 1), "cost": np.zeros(B, dtype=dtype), "reg": np.full(B, reg0, dtype=np.float64),
            "status": np.zeros(B, dtype=np.int64), "accepts": np.zeros(B, dtype=np.int64), "chosen": np.full(B, -1, dtype=np.int64),
            "L": int(L)}


def step(st, mean, linearise, mu0, target, W, W_T, reg0=1e-3, reg_factor=10.0, reg_max=1e6, tol=1e-9, dtype=np.float64):
    """One gpmpc_ilqr_step on the state dict `st`, in place.  `linearise(actions) -> (mu, A_t, B_t)`, `mean` as in `forward`."""
    running = st["status"] == 0
    actions = st["actions"]
    mu, At, Bt = linearise(actions)
    e, eH = errors(mu, actions, target, dtype)
    s = sweep(At, Bt, e, eH, W, W_T, st["reg"], dtype)
    c = cost(mu, actions, target, W, W_T, dtype)
    alphas = [0.5 ** l for l in range(st["L"])]
    f = forward(mean, actions, s["K"], s["k"], mu, mu0, alphas, dtype)
    B, L = actions.shape[0], st["L"]
    tc = cost(f["trial_mu"].reshape((B * L,) + f["trial_mu"].shape[2:]), f["trial_actions"].reshape((B * L,) + actions.shape[1:]),
              target, W, W_T, dtype).reshape(B, L)
    for key, val in (("gains", s["K"]), ("ff", s["k"]), ("mu", mu), ("dV", s["dV"]), ("flags", s["flags"]),
                     ("step", step_size(actions, s["k"], dtype)), ("trial_cost", tc), ("trial_actions", f["trial_actions"])):
        if key in st:
            st[key] = np.where(running.reshape((-1,) + (1,) * (np.ndim(val) - 1)), val, st[key])
        else:
            st[key] = val
    st["cost"] = np.where(running, c, st["cost"])
    chosen, accepts, reg, status, newc = accept_rule(st["cost"], st["trial_cost"], st["step"], st["reg"], st["status"],
                                                      st["accepts"], reg0, reg_factor, reg_max, tol)
    for b in range(B):
        if chosen[b] >= 0:
            st["actions"][b] = st["trial_actions"][b, chosen[b]]
        if chosen[b] != -2:
            st["chosen"][b] = chosen[b]
    st["accepts"], st["reg"], st["status"], st["cost"] = accepts, reg, status, newc.astype(dtype)
    return st


def gp_problem(fa, mu0, include_time=False, time0=0.0, dtype=np.float64):
    """(mean, linearise) of the GP of `fa` for `step`."""
    return (gp_mean(fa, include_time, time0, dtype),
            lambda actions: lq.linearisation(*fa, actions, mu0, include_time, time0, dtype))
