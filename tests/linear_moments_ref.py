"""Numpy restatement of the linearised (first-order Taylor) propagation of gpmpc_moments_linear / gpmpc_rollout_linear, in a
dtype of the caller's choice (float64: what a plain fp64 evaluation rounds to; longdouble: the yardstick), plus the stage and
terminal costs of a trajectory by the package's host SetpointStateRewardMapper.  TEST CODE ONLY.

Per input mean m (E), covariance Sigma (E, E) and output a, with the cached X, lengthscales l, outputscales sigma2, iK, beta:
    k_aj = sigma2_a exp(-1/2 sum_e (m_e - x_je)^2 / l_ae^2)
    M_a = sum_j k_aj beta_aj,   V[e, a] = (1 / l_ae^2) sum_j beta_aj k_aj (x_je - m_e),   v_a = sigma2_a - k_a^T iK_a k_a
    S = V^T Sigma V + diag(v)
"""
import numpy as np


def step(X, ls, os_, iK, beta, m, Sigma=None, dtype=np.float64):
    """m (P, E), Sigma (P, E, E) or None -> M (P, D), S (P, D, D), V (P, E, D), v (P, D), all in `dtype`."""
    X, ls, os_, beta, m = (np.asarray(v, dtype=dtype) for v in (X, ls, os_, beta, m))
    P, E = m.shape
    D = beta.shape[0]
    M = np.empty((P, D), dtype=dtype)
    V = np.empty((P, E, D), dtype=dtype)
    v = np.empty((P, D), dtype=dtype)
    for a in range(D):
        diff = X[None, :, :] - m[:, None, :]                       # (P, N, E): x_je - m_e, per element
        sc = diff / ls[a]
        k = os_[a] * np.exp(-0.5 * np.sum(sc * sc, axis=-1))        # (P, N)
        bk = k * beta[a]
        M[:, a] = np.sum(bk, axis=-1)
        V[:, :, a] = np.sum(bk[:, :, None] * diff, axis=1) / (ls[a] * ls[a])
        v[:, a] = os_[a] - np.sum((k @ np.asarray(iK[a], dtype=dtype)) * k, axis=-1)
    S = np.zeros((P, D, D), dtype=dtype)
    if Sigma is not None:
        Sg = np.asarray(Sigma, dtype=dtype)
        S = np.transpose(V, (0, 2, 1)) @ Sg @ V
    S = S + v[:, :, None] * np.eye(D, dtype=dtype)[None]
    return M, S, V, v


def mean_only(X, ls, os_, beta, m, dtype=np.longdouble):
    """The posterior mean alone (P, D): what the finite differences of V difference."""
    X, ls, os_, beta, m = (np.asarray(v, dtype=dtype) for v in (X, ls, os_, beta, m))
    out = np.empty((m.shape[0], beta.shape[0]), dtype=dtype)
    for a in range(beta.shape[0]):
        sc = (X[None, :, :] - m[:, None, :]) / ls[a]
        out[:, a] = (os_[a] * np.exp(-0.5 * np.sum(sc * sc, axis=-1))) @ beta[a]
    return out


def rollout(X, ls, os_, iK, beta, actions, mu0, S0, include_time=False, time0=0.0, dtype=np.float64):
    """The recurrence of predict_trajectory with the step above: actions (B, H, A) -> mu (B, H + 1, D), Sig (B, H + 1, D, D)."""
    actions = np.asarray(actions, dtype=dtype)
    B, H, A = actions.shape
    D = np.asarray(beta).shape[0]
    E = np.asarray(X).shape[1]
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
        s = np.zeros((B, E, E), dtype=dtype)
        s[:, :D, :D] = Sig[:, t]
        M, S, V, _ = step(X, ls, os_, iK, beta, m, s, dtype=dtype)
        T = Sig[:, t] @ V[:, :D, :]
        mu[:, t + 1] = mu[:, t] + M
        Sig[:, t + 1] = Sig[:, t] + S + T + np.transpose(T, (0, 2, 1))
    return mu, Sig


def reward_config_of(w, clip=False, state_min=None, state_max=None):
    """The package's RewardConfig for a synthetic workload (diagonal weights)."""
    from gp_mpc_amd.config_classes import RewardConfig
    D = w.Y.shape[1]
    kw = {}
    if state_min is not None:
        kw = dict(use_constraints=True, state_min=list(state_min), state_max=list(state_max))
    return RewardConfig(target_state_norm=list(w.target[:D]), weight_state=list(np.diag(w.W)[:D]),
                        weight_state_terminal=list(np.diag(w.W_T)), target_action_norm=list(w.target[D:]),
                        weight_action=list(np.diag(w.W)[D:]), exploration_factor=w.kappa, clip_lower_bound_cost_to_0=clip, **kw)


def costs(cfg, mu, Sig, actions):
    """cost_mu, cost_var (B, H + 1) and J (B,) of stored trajectories by the host SetpointStateRewardMapper
    (get_rewards_trajectory) and the LCB rule of compute_mean_lcb_trajectory, in float64."""
    import torch
    from gp_mpc_amd.control_objects.states_reward_mappers.setpoint_distance_reward_mapper import SetpointStateRewardMapper
    mapper = SetpointStateRewardMapper(cfg)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))       # noqa: E731
    cm, cv = [], []
    for b in range(mu.shape[0]):
        r, v = mapper.get_rewards_trajectory(t(mu[b]), t(Sig[b]), t(actions[b]))
        cm.append(-r.numpy())
        cv.append(v.numpy())
    cm, cv = np.stack(cm), np.stack(cv)
    ucb = -cm + float(cfg.exploration_factor) * np.sqrt(cv)
    if cfg.clip_lower_bound_cost_to_0:
        ucb = np.minimum(ucb, 0.0)
    return cm, cv, -ucb.mean(axis=-1)
