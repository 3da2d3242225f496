"""Numpy restatement of the closed-loop moment-matched rollout of gpmpc_rollout_feedback (include/gpmpc.h), over the committed
oracles: oracle.gpmpc_oracle.moment_match_step (fp64, batched over candidates) and oracle.extended_precision.moment_match_step
(long double, one input at a time).  Costs are those of tests/feedback_rollout_ref.costs.  TEST CODE ONLY.

Policy u = ubar_t + K_t (x - mu_t), x ~ N(mu_t, Sigma_t).  Per step, with G = [I_D ; K_t ; 0] (E x D):
    model input mean [mu_t | ubar_t | time0 + t], model input covariance Sigma_in = G Sigma_t G^T (by blocks, time row zero)
    M, S, V = moment_match_step(mean, Sigma_in)
    C = Sigma_in[:D, :] V,   mu_{t+1} = mu_t + M,   Sigma_{t+1} = Sigma_t + S + C + C^T
which is oracle.gpmpc_oracle.predict_trajectory (gp_model.py:95-108) fed the policy's full input covariance.
"""
import numpy as np

from feedback_rollout_ref import broadcast_gains, costs  # noqa: F401  (costs: re-exported for the tests)
from oracle import extended_precision as xp
from oracle import gpmpc_oracle as orc

LD = np.longdouble


def input_covariance(Sig_t, K_t, E):
    """Sig_t (..., D, D), K_t (..., A, D) -> G Sig_t G^T (..., E, E), G = [I ; K_t ; 0]."""
    D, A = Sig_t.shape[-1], K_t.shape[-2]
    KS = K_t @ Sig_t
    s = np.zeros(Sig_t.shape[:-2] + (E, E), dtype=Sig_t.dtype)
    s[..., :D, :D] = Sig_t
    s[..., D:D + A, :D] = KS
    s[..., :D, D:D + A] = np.swapaxes(KS, -1, -2)
    s[..., D:D + A, D:D + A] = KS @ np.swapaxes(K_t, -1, -2)
    return s


def rollout(f, actions, gains, mu0, S0, include_time=False, time0=0.0):
    """fp64, batched: f an oracle.gpmpc_oracle.Factors; actions (B, H, A); gains (A, D) / (H, A, D) / (B, H, A, D)
    -> mu (B, H + 1, D), Sig (B, H + 1, D, D)."""
    actions = np.asarray(actions, dtype=np.float64)
    B, H, A = actions.shape
    D = f.lengthscales.shape[0]
    E = f.X.shape[1]
    K = broadcast_gains(gains, B, H, A, D)
    mu = np.empty((B, H + 1, D))
    Sig = np.empty((B, H + 1, D, D))
    mu[:, 0] = mu0
    Sig[:, 0] = S0
    for t in range(H):
        s = input_covariance(Sig[:, t], K[:, t], E)
        m = np.empty((B, E))
        m[:, :D] = mu[:, t]
        m[:, D:D + A] = actions[:, t]
        if include_time:
            m[:, -1] = time0 + t
        M, S, V = orc.moment_match_step(f, m, s)
        mu[:, t + 1] = mu[:, t] + M
        C = s[:, :D, :] @ V
        Sig[:, t + 1] = S + Sig[:, t] + C + C.transpose(0, 2, 1)
    return mu, Sig


def rollout_extended(fx, actions, gains, mu0, S0, include_time=False, time0=0.0):
    """Long double, one candidate at a time: fx an oracle.extended_precision.Factors; same arguments and shapes."""
    actions = np.asarray(actions, dtype=LD)
    B, H, A = actions.shape
    D = fx.lengthscales.shape[0]
    E = fx.X.shape[1]
    K = broadcast_gains(gains, B, H, A, D, LD)
    mu = np.empty((B, H + 1, D), dtype=LD)
    Sig = np.empty((B, H + 1, D, D), dtype=LD)
    mu[:, 0] = np.asarray(mu0, dtype=LD)
    Sig[:, 0] = np.asarray(S0, dtype=LD)
    for b in range(B):
        for t in range(H):
            s = input_covariance(Sig[b, t], K[b, t], E)
            m = np.empty(E, dtype=LD)
            m[:D] = mu[b, t]
            m[D:D + A] = actions[b, t]
            if include_time:
                m[-1] = LD(time0) + t
            M, S, V = xp.moment_match_step(fx, m, s)
            mu[b, t + 1] = mu[b, t] + M
            C = s[:D, :] @ V
            Sig[b, t + 1] = S + Sig[b, t] + C + C.T
    return mu, Sig


# The cases of tests/test_gpu_rollout_feedback.py, shared with the CPU checks of tests/test_feedback_mm_reference.py:
# (D, A, N, H, B, time).  One and three 64-row tiles of the pair pass with a ragged edge; B below, at and across the
# points-per-workgroup and chunk boundaries; A > 1 and a time input.
CASES = {
    "a_d3_a1_n50_h1_b65": (3, 1, 50, 1, 65, False),
    "b_d3_a2_n50_h5_b1_time": (3, 2, 50, 5, 1, True),
    "c_d3_a1_n50_h12_b130": (3, 1, 50, 12, 130, False),
    "d_d3_a2_n130_h5_b65_time": (3, 2, 130, 5, 65, True),
    "e_d5_a2_n130_h8_b1": (5, 2, 130, 8, 1, False),
}
MU_TOL, SIG_TOL = 1e-9, 1e-5          # GPU against long double, relative to max|mu| / max|Sig| (tests/test_gpu_moments.py)


def case_workload(case):
    """The workload recipe of tests/test_gpu_rollout_linear_feedback.py and per-candidate gains."""
    from oracle import synth
    D, A, N, H, B, time = CASES[case]
    w = synth.make_workload(N, D, A, H, B, include_time=time, seed=400 + N + H + A, time0=3.0, dynamics="contracting",
                            dense_s0=0.02)
    K = np.random.default_rng(401).standard_normal((B, H, A, D))
    return w, K


def selected(B):
    return np.unique(np.array([0, B // 2, B - 1]))


_extended = {}


def case_extended(case):
    """(sel, mu_ld, Sig_ld) of the case's candidates {0, B // 2, B - 1}: computed once per process, shared, left unchanged."""
    if case not in _extended:
        w, K = case_workload(case)
        sel = selected(w.dims[5])
        fx = xp.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        mu, Sig = rollout_extended(fx, w.actions[sel], K[sel], w.mu0, w.S0, w.include_time, w.time0)
        mu.setflags(write=False)
        Sig.setflags(write=False)
        _extended[case] = (sel, mu, Sig)
    return _extended[case]
