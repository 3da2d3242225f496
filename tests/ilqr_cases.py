"""Workloads of the iLQR tests (tests/test_ilqr_reference.py, tests/test_gpu_ilqr.py).  TEST CODE ONLY.

oracle/synth.py's dynamics barely feel the action (|V_u| ~ 0.02), so an optimiser over the actions has nothing to find there.  The
memory made here is ACTION-DRIVEN:
    Y_d = -0.2 (x_d - 0.5) + 0.15 (u_{d mod A} - 0.5) + 0.02 sin(3 x_d + u_last) + 1e-3 noise
with synth's length-scales, output scale 5e-2 and noise 1e-5; everything else (mu0, S0, actions, cost) is synth's.
"""
import numpy as np

from oracle import synth


def make_workload(N, D, A, H, B, include_time=False, seed=0, time0=3.0, dense_s0=0.02):
    w = synth.make_workload(N, D, A, H, B, include_time=include_time, seed=seed, time0=time0, dynamics="contracting",
                            dense_s0=dense_s0)
    rng = np.random.default_rng(seed + 77)
    X = w.X
    for d in range(D):
        w.Y[:, d] = (-0.2 * (X[:, d] - 0.5) + 0.15 * (X[:, D + d % A] - 0.5) + 0.02 * np.sin(3.0 * X[:, d] + X[:, D + A - 1])
                     + 1e-3 * rng.standard_normal(N))
    return w


def weights(D, A, seed):
    """A full, ASYMMETRIC stage weight with cross terms whose symmetric part is positive definite, and such a terminal weight
    (the construction of tests/test_gpu_lqr_gains._weights)."""
    rng = np.random.default_rng(seed)
    n = D + A
    G, S = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    W = G @ G.T / n + np.eye(n) + 0.25 * (S - S.T)
    G, S = rng.standard_normal((D, D)), rng.standard_normal((D, D))
    W_T = G @ G.T / D + np.eye(D) + 0.25 * (S - S.T)
    return W, W_T


def factors(w):
    """(X, ls, os, iK, beta) of the exact GP of the workload in fp64 numpy: what HipEngine.prepare + factors() give on the GPU."""
    X, ls, os_, nz = w.X, w.lengthscales, w.outputscales, w.noises
    N, D = X.shape[0], w.Y.shape[1]
    iK, beta = np.empty((D, N, N)), np.empty((D, N))
    for a in range(D):
        sc = (X[:, None, :] - X[None, :, :]) / ls[a]
        K = os_[a] * np.exp(-0.5 * np.sum(sc * sc, axis=-1)) + nz[a] * np.eye(N)
        iK[a] = np.linalg.inv(K)
        iK[a] = 0.5 * (iK[a] + iK[a].T)
        beta[a] = np.linalg.solve(K, w.Y[:, a])
    return (X, ls, os_, iK, beta)
