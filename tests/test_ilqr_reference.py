"""Tier 1 (CPU): the numpy restatement of the clamped iLQR (tests/ilqr_ref.py, the definition the kernels of csrc/ilqr.hip are tested
against in tests/test_gpu_ilqr.py) tied to things it does not define:

  LQ exactness    on random affine dynamics with a positive definite cost, one iteration with alpha = 1, reg = 0 and no active bound
                  lands on the minimiser of the stacked normal equations (numpy.linalg.solve);
  K and P         are those of tests/lqr_gains_ref.sweep;
  dV              d c(alpha) / d alpha at alpha = 0 of the unclipped forward pass equals 2 dV (long-double central differences);
  behaviour       on the action-driven memory of tests/ilqr_cases.py the cost never increases and every start reaches one common
                  minimum; the box; the statuses.
"""
import numpy as np
import pytest

import ilqr_cases as cases
import ilqr_ref as ref
import lqr_gains_ref as lq

LD = np.longdouble


def _affine_problem(seed, D, A, H):
    """x' = A_t x + B_t u + c_t with a positive definite cost; returns the pieces and mean(x, u, t) = x' - x."""
    rng = np.random.default_rng(seed)
    At = np.eye(D) + 0.3 * rng.standard_normal((H, D, D))
    Bt = rng.standard_normal((H, D, A))
    ct = 0.1 * rng.standard_normal((H, D))
    W, W_T = cases.weights(D, A, seed + 1)
    target = rng.uniform(0.3, 0.7, D + A)
    mu0 = rng.uniform(0.3, 0.7, D)

    def mean(x, u, t):
        return x @ At[t].T + u @ Bt[t].T + ct[t] - x

    def rollout(actions):
        mu = np.empty((actions.shape[0], H + 1, D))
        mu[:, 0] = mu0
        for t in range(H):
            mu[:, t + 1] = mu[:, t] + mean(mu[:, t], actions[:, t], t)
        return mu
    return At, Bt, W, W_T, target, mu0, mean, rollout


@pytest.mark.parametrize("D,A,H", [(3, 1, 4), (4, 2, 6), (2, 3, 5)])
def test_one_iteration_solves_the_lq_problem(D, A, H):
    At, Bt, W, W_T, target, mu0, mean, rollout = _affine_problem(11 + D, D, A, H)
    n = H * A
    u0 = np.random.default_rng(12).uniform(0.2, 0.8, (1, H, A))
    # the minimiser from the stacked normal equations: z(u) = [e_0 .. e_{H-1} | e_H] is affine in u
    def z(u):
        mu = rollout(u.reshape(1, H, A))
        e, eH = ref.errors(mu, u.reshape(1, H, A), target)
        return np.concatenate([e[0].reshape(-1), eH[0]])
    z0 = z(np.zeros(n))
    G = np.stack([z(np.eye(n)[i]) - z0 for i in range(n)], axis=1)
    Wb = np.zeros((z0.size, z0.size))
    for t in range(H):
        s = slice(t * (D + A), (t + 1) * (D + A))
        Wb[s, s] = 0.5 * (W + W.T)
    Wb[H * (D + A):, H * (D + A):] = 0.5 * (W_T + W_T.T)
    u_star = np.linalg.solve(G.T @ Wb @ G, -G.T @ Wb @ z0)
    # one iLQR iteration from u0 (no clipping: the minimiser may lie outside the box)
    mu = rollout(u0)
    e, eH = ref.errors(mu, u0, target)
    s = ref.sweep(At[None], Bt[None], e, eH, W, W_T, 0.0)
    f = ref.forward(mean, u0, s["K"], s["k"], mu, mu0, [1.0], clip=False)
    got = f["trial_actions"][0, 0].reshape(-1)
    assert not s["flags"].any()
    assert np.max(np.abs(got - u_star)) <= 1e-10 * np.max(np.abs(u_star))
    # the model's predicted change is exact on an LQ problem: c(1) - c(0) = dV
    c0 = ref.cost(mu, u0, target, W, W_T)[0]
    c1 = ref.cost(f["trial_mu"][:, 0], f["trial_actions"][:, 0], target, W, W_T)[0]
    assert abs((c1 - c0) - s["dV"][0]) <= 1e-10 * abs(c0) and s["dV"][0] < 0
    # ... and K, P are those of the Riccati sweep of gpmpc_lqr_gains
    K, P, flags = lq.sweep(At[None], Bt[None], W, W_T, 0.0)
    assert np.array_equal(K, s["K"]) and np.array_equal(P, s["P"]) and not flags.any()


@pytest.mark.parametrize("D,A,N,H,time", [(3, 1, 50, 3, False), (4, 2, 50, 5, True), (3, 1, 60, 10, False)])
def test_k_and_p_and_the_directional_derivative_on_a_gp(D, A, N, H, time):
    w = cases.make_workload(N, D, A, H, 2, include_time=time, seed=21)
    W, W_T = cases.weights(D, A, 22)
    fa = cases.factors(w)
    b = ref.backward(fa, w.actions, w.mu0, w.target, W, W_T, w.include_time, w.time0, reg=1e-3, dtype=LD)
    K, P, _ = lq.gains(*fa, w.actions, w.mu0, W, W_T, w.include_time, w.time0, 1e-3, dtype=LD)
    assert np.array_equal(K, b["gains"]) and np.array_equal(P, b["P"])
    mean = ref.gp_mean(fa, w.include_time, w.time0, LD)

    def c(alpha):
        f = ref.forward(mean, w.actions, b["gains"], b["ff"], b["mu"], w.mu0, [alpha], dtype=LD, clip=False)
        return ref.cost(f["trial_mu"][:, 0], f["trial_actions"][:, 0], w.target, W, W_T, LD)
    # fourth-order central difference in long double: truncation h^4 c^(5) / 30 with h = 1e-3, rounding 1e-19 / h
    h = LD(1e-3)
    d = (8 * (c(h) - c(-h)) - (c(2 * h) - c(-2 * h))) / (12 * h)
    # reg enters Huu, so the quadratic model's slope is exact only up to reg |k|^2 / (H + 1): compare to the slope itself,
    # g_u^T k summed -- which is what dV is
    print("dc/dalpha", d, "2 dV", 2 * b["dV"])
    assert np.all(b["dV"] < 0)
    assert np.max(np.abs(d - 2 * b["dV"]) / np.abs(2 * b["dV"])) <= 1e-8


CASES = [(3, 1, 50, 3, False), (4, 2, 50, 5, True), (3, 1, 60, 10, False)]


@pytest.mark.parametrize("D,A,N,H,time", CASES)
def test_cost_never_increases_and_the_starts_meet(D, A, N, H, time):
    w = cases.make_workload(N, D, A, H, 4, include_time=time, seed=5)
    W, W_T = cases.weights(D, A, 6)
    fa = cases.factors(w)
    st = ref.init(w.actions, 8, 1e-3)
    mean, linearise = ref.gp_problem(fa, w.mu0, w.include_time, w.time0)
    costs = []
    for it in range(12):
        ref.step(st, mean, linearise, w.mu0, w.target, W, W_T, 1e-3, 10.0, 1e6, 1e-9)
        costs.append(st["cost"].copy())
        if it == 0:
            assert np.all(st["chosen"] >= 0)                               # every start improves in its first iteration
    costs = np.array(costs)
    first = ref.backward(fa, w.actions, w.mu0, w.target, W, W_T, w.include_time, w.time0, 1e-3)["cost"]
    assert np.all(costs[0] < first) and np.all(np.diff(costs, axis=0) <= 0)
    print(costs[-1], st["status"], st["accepts"])
    assert np.ptp(costs[-1]) <= 1e-9 * abs(costs[-1, 0])                   # one common minimum
    assert np.all((st["actions"] >= 0) & (st["actions"] <= 1))


def test_the_box():
    w = cases.make_workload(50, 3, 1, 3, 4, seed=760)
    target = w.target.copy()
    target[3:] = 1.5
    W = np.diag([1.0, 0.1, 0.1, 0.5])
    fa = cases.factors(w)
    st = ref.init(w.actions, 4, 1e-3)
    mean, linearise = ref.gp_problem(fa, w.mu0)
    ref.step(st, mean, linearise, w.mu0, target, W, w.W_T)
    assert np.array_equal(st["actions"], np.ones((4, 3, 1))) and not st["status"].any() and np.all(st["chosen"] == 0)
    ref.step(st, mean, linearise, w.mu0, target, W, w.W_T)
    assert np.array_equal(st["step"], np.zeros(4)) and np.array_equal(st["status"], np.ones(4)) and np.all(st["dV"] < 0)
    assert np.array_equal(st["actions"], np.ones((4, 3, 1)))
    before = {k: np.array(v, copy=True) for k, v in st.items() if isinstance(v, np.ndarray)}
    ref.step(st, mean, linearise, w.mu0, target, W, w.W_T)                 # a finished candidate's state no longer changes
    for k, v in before.items():
        assert np.array_equal(st[k], v), k


def test_statuses_two_and_three():
    D, A, H = 3, 1, 3
    w = cases.make_workload(50, D, A, H, 3, seed=31)
    W, W_T = cases.weights(D, A, 32)
    fa = cases.factors(w)
    mean, linearise = ref.gp_problem(fa, w.mu0)
    # status 2: a converged sequence rejects (no trial is strictly below it); with reg_max = reg0 the first reject ends the search
    st = ref.init(w.actions[:1], 8, 1e-3)
    for _ in range(12):
        ref.step(st, mean, linearise, w.mu0, w.target, W, W_T, 1e-3, 10.0, 1e6, 0.0)
    start = st["actions"].copy()
    for _ in range(40):                                                    # polish until an iteration rejects
        probe = ref.init(start, 8, 1e-3)
        ref.step(probe, mean, linearise, w.mu0, w.target, W, W_T, 1e-3, 10.0, 1e-3, 0.0)
        if probe["chosen"][0] == -1:
            break
        start = probe["actions"].copy()
    assert probe["chosen"][0] == -1 and probe["status"][0] == 2 and probe["reg"][0] == 1e-2 and probe["accepts"][0] == 0
    assert np.array_equal(probe["actions"], start)
    # status 3: a non-finite start
    x0 = w.actions.copy()
    x0[1, 0, 0] = np.nan
    st = ref.init(x0, 4, 1e-3)
    with np.errstate(all="ignore"):
        ref.step(st, mean, linearise, w.mu0, w.target, W, W_T)
    assert st["status"].tolist() == [0, 3, 0] and st["chosen"].tolist()[1] == -1 and st["accepts"].tolist() == [1, 0, 1]
