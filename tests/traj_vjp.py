"""Numpy vector-Jacobian product of a whole trajectory with general cotangents (the checker of gpmpc_rollout_backward).

Built from oracle.adjoint's forward_step / backward_step / cost_terms, one candidate at a time: the gradients of
    sum_t <mu_bar_t, mu_t> + <Sig_bar_t, Sig_t> + cm_bar_t cm_t + cv_bar_t cv_t + J_bar J
with respect to the actions (H, A), the initial mean (D) and the initial covariance (D, D, its symmetric part), where
J = mean_t (cm_t - kappa sqrt(cv_t)) is the LCB of compute_mean_lcb_trajectory (clip_to_zero: pass-through).  The cost
cotangents weigh the stage-cost partials as wm_t = cm_bar_t + J_bar / (H+1), wv_t = cv_bar_t + J_bar (-kappa / (2 sqrt(cv_t)))
/ (H+1); with J_bar = 1 alone this is oracle.adjoint.lcb_and_gradient.
"""
import numpy as np

from oracle import adjoint


def _sym(G):
    return 0.5 * (G + np.swapaxes(G, -1, -2))


def traj_vjp(f, actions, mu0, S0, target, W, W_T, kappa, mu_bar=None, Sig_bar=None, cm_bar=None, cv_bar=None, J_bar=0.0,
             include_time=False, time0=0.0, state_min=None, state_max=None):
    """One candidate: actions (H, A) -> (d/d actions (H, A), d/d mu0 (D,), sym d/d S0 (D, D)).  Cotangents None = 0."""
    H, A = actions.shape
    D = mu0.shape[0]
    E = f.X.shape[1]
    mu_bar = np.zeros((H + 1, D)) if mu_bar is None else np.asarray(mu_bar, float)
    Sig_bar = np.zeros((H + 1, D, D)) if Sig_bar is None else np.asarray(Sig_bar, float)
    cm_bar = np.zeros(H + 1) if cm_bar is None else np.asarray(cm_bar, float)
    cv_bar = np.zeros(H + 1) if cv_bar is None else np.asarray(cv_bar, float)
    J_bar = float(J_bar)
    mu, Sig = np.asarray(mu0, float).copy(), np.asarray(S0, float).copy()
    recs, mus, Sigs = [], [mu], [Sig]
    for t in range(H):
        m = np.zeros(E)
        m[:D] = mu
        m[D:D + A] = actions[t]
        if include_time:
            m[-1] = time0 + t
        M, dS, r = adjoint.forward_step(f, m, Sig)
        recs.append(r)
        mu, Sig = mu + M, Sig + dS
        mus.append(mu)
        Sigs.append(Sig)
    n = H + 1

    def weights(t, cv):
        wm = cm_bar[t] + J_bar / n
        wv = cv_bar[t] + (J_bar * (-kappa / (2.0 * np.sqrt(cv))) / n if J_bar != 0.0 else 0.0)
        return wm, wv

    grad = np.zeros((H, A))
    _, cvT, dmT, dvT = adjoint.cost_terms(mus[H], Sigs[H], None, target, W_T)
    wm, wv = weights(H, cvT)
    mb = wm * dmT[0] + wv * dvT[0] + mu_bar[H]
    Sb = _sym(wm * dmT[1] + wv * dvT[1]) + _sym(Sig_bar[H])
    for t in range(H - 1, -1, -1):
        mb, Sb, m_bar = adjoint.backward_step(f, recs[t], mb, Sb)
        _, cv, dm, dv = adjoint.cost_terms(mus[t], Sigs[t], actions[t], target, W, state_min, state_max)
        wm, wv = weights(t, cv)
        grad[t] = m_bar[D:D + A] + wm * dm[2] + wv * dv[2]
        mb = mb + wm * dm[0] + wv * dv[0] + mu_bar[t]
        Sb = Sb + _sym(wm * dm[1] + wv * dv[1]) + _sym(Sig_bar[t])
    return grad, mb, _sym(Sb)


def golden_seeds(gg, s, b):
    """Upstream set s, candidate b of a traj_grad_* golden as the library's cotangents: the reference's rewards are -cost_mu,
    its reward variances cost_var."""
    return dict(mu_bar=gg["mu_bar"][s, b], Sig_bar=gg["Sig_bar"][s, b], cm_bar=-gg["rewards_bar"][s, b],
                cv_bar=gg["reward_vars_bar"][s, b])
