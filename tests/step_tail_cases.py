"""Workloads of tests/test_gpu_step_tail.py and of tools/gen_step_tail_golden.py (which pins their bits): a tiny GP memory
(N = 14), DENSE cost weights (the synthetic workloads' own are diagonal: a transposed or mis-strided weight index would not
show) and optional state constraints.  One function, so that the fixture and the test can never disagree about the inputs."""
import numpy as np

from oracle import synth

N_MEMORY = 14

# (D, A, H, B, clip, constraints, include_time): the shapes whose J / cost_mu / cost_var bits tests/golden/step_tail_costs.npz
# holds.  D <= 4 and A <= 2 take the register form of the cost kernel, (6, 3) the generic one; H + 1 = 65, 71: a second trip.
GOLDEN_CASES = [
    (3, 1, 25, 64, False, False, False),      # the config-2 shape of the cost kernel
    (1, 1, 5, 3, True, False, False),
    (2, 2, 70, 3, False, True, False),
    (4, 2, 64, 3, True, True, False),
    (4, 1, 63, 1, False, False, True),
    (3, 2, 1, 300, False, True, False),
    (6, 3, 5, 3, True, True, False),
]


def case_seed(D, A, H, B):
    return 1000 * D + 100 * A + H + 7 * B


def make_case(D, A, H, B, constraints=False, include_time=False):
    """(workload, state_min, state_max) -- state_min / state_max None without constraints."""
    seed = case_seed(D, A, H, B)
    w = synth.make_workload(N=N_MEMORY, D=D, A=A, H=H, B=B, include_time=include_time, seed=seed, time0=3.0,
                            dynamics="contracting", dense_s0=0.02)
    rng = np.random.default_rng(seed + 5)
    n = D + A
    G = rng.standard_normal((n, n))
    # dense, positive definite, slightly NON-symmetric (W[i, j] != W[j, i] tells a transposed index from the right one)
    w.W = w.W + 0.05 * (G @ G.T) / n + 0.002 * rng.standard_normal((n, n))
    GT = rng.standard_normal((D, D))
    w.W_T = w.W_T + 0.2 * (GT @ GT.T) / D + 0.01 * rng.standard_normal((D, D))
    w.kappa = 0.7
    smin = smax = None
    if constraints:
        # bounds INSIDE the range the trajectory visits, so that both erf terms are away from 0 and 1 somewhere
        smin = 0.3 + 0.1 * rng.uniform(size=D)
        smax = 0.6 + 0.1 * rng.uniform(size=D)
    return w, smin, smax


def run_case(engine, D, A, H, B, clip=False, constraints=False, include_time=False):
    """Prepare, set the cost and roll out on `engine`; returns (workload, state_min, state_max, out)."""
    w, smin, smax = make_case(D, A, H, B, constraints, include_time)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa, clip, smin, smax)
    out = engine.rollout(w.actions, w.mu0, w.S0, w.include_time, w.time0)
    return w, smin, smax, out
