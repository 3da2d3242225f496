"""Numpy restatement of the closed-loop linearised rollout of gpmpc_rollout_linear_feedback (include/gpmpc.h), in a dtype of the
caller's choice, built on tests/linear_moments_ref.step, plus its stage and terminal costs by the package's host
SetpointStateRewardMapper._quadratic with the full state-action covariance.  TEST CODE ONLY.

Policy u = ubar_t + K_t (x - mu_t), x ~ N(mu_t, Sigma_t).  Per step, with G = [I_D ; K_t ; 0] (E x D):
    model input mean [mu_t | ubar_t | time0 + t] (the gains never move it), model input covariance G Sigma_t G^T
    M, S, V = step(mean, covariance)              S = V^T (G Sigma_t G^T) V + diag v = C^T Sigma_t C + diag v
    C = G^T V = V_s + K_t^T V_u,   T = Sigma_t C
    mu_{t+1} = mu_t + M,   Sigma_{t+1} = Sigma_t + S + T + T^T
"""
import numpy as np

import linear_moments_ref as lin


def broadcast_gains(gains, B, H, A, D, dtype=np.float64):
    """(A, D), (H, A, D) or (B, H, A, D) -> (B, H, A, D)."""
    g = np.asarray(gains, dtype=dtype)
    if g.shape not in ((A, D), (H, A, D), (B, H, A, D)):
        raise ValueError(f"gains of shape {g.shape}")
    return np.broadcast_to(g, (B, H, A, D))


def rollout(X, ls, os_, iK, beta, actions, gains, mu0, S0, include_time=False, time0=0.0, dtype=np.float64):
    """actions (B, H, A), gains (A, D) / (H, A, D) / (B, H, A, D) -> mu (B, H + 1, D), Sig (B, H + 1, D, D)."""
    actions = np.asarray(actions, dtype=dtype)
    B, H, A = actions.shape
    D = np.asarray(beta).shape[0]
    E = np.asarray(X).shape[1]
    K = broadcast_gains(gains, B, H, A, D, dtype)
    mu = np.empty((B, H + 1, D), dtype=dtype)
    Sig = np.empty((B, H + 1, D, D), dtype=dtype)
    mu[:, 0] = np.asarray(mu0, dtype=dtype)
    Sig[:, 0] = np.asarray(S0, dtype=dtype)
    for t in range(H):
        m = np.zeros((B, E), dtype=dtype)
        m[:, :D] = mu[:, t]
        m[:, D:D + A] = actions[:, t]
        if include_time:
            m[:, -1] = dtype(time0) + dtype(t)
        Kt = K[:, t]                                                  # (B, A, D)
        KS = Kt @ Sig[:, t]                                           # (B, A, D)
        s = np.zeros((B, E, E), dtype=dtype)                          # G Sigma G^T by blocks; the time row and column stay zero
        s[:, :D, :D] = Sig[:, t]
        s[:, D:D + A, :D] = KS
        s[:, :D, D:D + A] = np.transpose(KS, (0, 2, 1))
        s[:, D:D + A, D:D + A] = KS @ np.transpose(Kt, (0, 2, 1))
        M, S, V, _ = lin.step(X, ls, os_, iK, beta, m, s, dtype=dtype)
        C = V[:, :D, :] + np.transpose(Kt, (0, 2, 1)) @ V[:, D:D + A, :]
        T = Sig[:, t] @ C
        mu[:, t + 1] = mu[:, t] + M
        Sig[:, t + 1] = Sig[:, t] + S + T + np.transpose(T, (0, 2, 1))
    return mu, Sig


def costs(cfg, mu, Sig, actions, gains):
    """cost_mu, cost_var (B, H + 1) and J (B,) of stored closed-loop trajectories, in float64: the stage cost is
    SetpointStateRewardMapper._quadratic with Sigma_z = [I ; K_t] Sigma_t [I ; K_t]^T; the constraint term (state marginals),
    the terminal cost and the LCB rule are the open-loop ones (tests/linear_moments_ref.costs)."""
    import torch
    from gp_mpc_amd.control_objects.states_reward_mappers.setpoint_distance_reward_mapper import (SetpointStateRewardMapper,
                                                                                                    normal_cdf)
    mapper = SetpointStateRewardMapper(cfg)
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.float64))         # noqa: E731
    actions = np.asarray(actions, dtype=np.float64)
    B, H, A = actions.shape
    D = mu.shape[-1]
    K = broadcast_gains(gains, B, H, A, D)
    cm, cv = np.empty((B, H + 1)), np.empty((B, H + 1))
    for b in range(B):
        for k in range(H):
            m_t, S_t = t(mu[b, k]), t(Sig[b, k])
            err = torch.cat((m_t, t(actions[b, k]))) - cfg.target_state_action_norm
            G = torch.cat((torch.eye(D, dtype=torch.float64), t(K[b, k])), dim=0)
            c_mu, c_var = mapper._quadratic(err, G @ S_t @ G.T, cfg.weight_matrix_cost)
            if cfg.use_constraints:
                sd = S_t.diag()                     # (the variance where a std is expected: kept, as get_reward keeps it)
                c_mu = c_mu + (1 - normal_cdf(cfg.state_max, m_t, sd)).sum(-1) + normal_cdf(cfg.state_min, m_t, sd).sum(-1)
            cm[b, k], cv[b, k] = float(c_mu), float(c_var)
        r, v = mapper.get_reward_terminal(t(mu[b, H]), t(Sig[b, H]))
        cm[b, H], cv[b, H] = -float(r), float(v)
    ucb = -cm + float(cfg.exploration_factor) * np.sqrt(cv)
    if cfg.clip_lower_bound_cost_to_0:
        ucb = np.minimum(ucb, 0.0)
    return cm, cv, -ucb.mean(axis=-1)
