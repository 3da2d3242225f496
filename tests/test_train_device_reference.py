"""Tier 1 (no GPU): the numpy restatement of the device hyper-parameter search (tests/train_device_ref.py) against independent
yardsticks -- the box map's chain rule against longdouble central differences of the loss in x (step and tolerance as
tests/test_moments_backward_reference.py uses them with tests/moments_fd.py: h = 1e-6, |analytic - fd| <= 1e-6 |fd| + 1e-7 top),
the restated loop's monotonicity, and the winner rule on hand-made tables."""
import numpy as np
import pytest

import train_device_ref as tref
from oracle import synth

LD = np.longdouble
N, D, R, HISTORY = 24, 2, 4, 3


def setup():
    w = synth.make_workload(N, D, 1, 3, 2, seed=N)
    base = np.concatenate([w.lengthscales, w.outputscales[:, None], w.noises[:, None]], axis=1)
    return w, base / 8.0, base * 8.0


def test_the_package_has_the_device_search():
    from gp_mpc_amd import HipEngine, _lib
    assert _lib.ABI_VERSION >= 27
    for name in ("gpmpc_mll_batch", "gpmpc_train_search"):
        assert name in _lib.SIGNATURES
    for name in ("mll_batch", "train_search", "train_search_host"):
        assert callable(getattr(HipEngine, name))


@pytest.mark.parametrize("log_scale", [False, True])
def test_box_map_and_chain_rule_against_finite_differences(log_scale):
    w, lo, hi = setup()
    rng = np.random.default_rng(3)
    n = lo.shape[1]
    for a in range(D):
        # around the middle of the box, where K is well conditioned (the differences are of the loss, not of the map alone)
        x = rng.uniform(0.35, 0.65, size=n)
        theta = tref.box_map(x, lo[a], hi[a], log_scale)
        assert np.all((theta >= lo[a]) & (theta <= hi[a]))
        assert np.allclose(tref.box_unmap(theta, lo[a], hi[a], log_scale), x, rtol=0, atol=1e-12)
        theta_ld = tref.box_map(x, lo[a], hi[a], log_scale, dtype=LD)
        assert np.all(np.abs(theta.astype(LD) - theta_ld) <= 2 * np.spacing(theta))
        loss, g, _ = tref.loss_and_grad_x(w.X, w.Y[:, a], x, lo[a], hi[a], log_scale)
        assert abs(loss - float(tref.loss_longdouble_x(w.X, w.Y[:, a], x, lo[a], hi[a], log_scale))) <= 1e-10 * abs(loss)
        h = 1e-6
        fd = np.empty(n)
        for k in range(n):
            e = np.zeros(n, dtype=LD)
            e[k] = LD(h)
            lp = tref.loss_longdouble_x(w.X, w.Y[:, a], x.astype(LD) + e, lo[a], hi[a], log_scale)
            lm = tref.loss_longdouble_x(w.X, w.Y[:, a], x.astype(LD) - e, lo[a], hi[a], log_scale)
            fd[k] = float((lp - lm) / (2 * LD(h)))
        top = np.max(np.abs(fd))
        assert np.all(np.abs(g - fd) <= 1e-6 * np.abs(fd) + 1e-7 * top), (a, g, fd)
    # the ends of the box
    assert np.array_equal(tref.box_map(np.zeros(n), lo[0], hi[0], log_scale), lo[0])
    assert np.allclose(tref.box_map(np.ones(n), lo[0], hi[0], log_scale), hi[0], rtol=4e-16, atol=0)


@pytest.mark.parametrize("log_scale", [False, True])
def test_restated_loop_descends_and_the_winner_is_no_worse_than_the_first_start(log_scale):
    w, lo, hi = setup()
    n = lo.shape[1]
    x0 = np.random.default_rng(40 + N).uniform(0.05, 0.95, size=(R, D, n))
    J0, _ = tref.evaluate(w.X, w.Y, x0.reshape(R * D, n), lo, hi, log_scale)
    state, trace = tref.search(w.X, w.Y, x0, lo, hi, log_scale, 8, HISTORY)
    assert np.array_equal(trace[0], J0)                              # step 0 accepts the start
    for before, after in zip(trace, trace[1:]):
        assert np.all(after <= before)                               # J per restart never increases
    assert np.any(trace[-1] < trace[0])
    best = tref.winner(state["J"], state["status"], state["x"], lo, hi, log_scale, D)
    assert np.all(best[:, 0] <= J0.reshape(R, D)[0]) and np.all(best[:, 0] == state["J"].reshape(R, D).min(axis=0))
    # two calls of 3 and 5 iterations, the second continuing the state, are the one call of 8
    half, _ = tref.search(w.X, w.Y, x0, lo, hi, log_scale, 3, HISTORY)
    both, _ = tref.search(w.X, w.Y, None, lo, hi, log_scale, 5, HISTORY, first_iteration=3, state=half)
    for k in state:
        assert np.array_equal(both[k], state[k]), k


def test_winner_rule_on_hand_made_tables():
    n, Dg = 3, 2
    lo, hi = np.full((Dg, n), 0.5), np.full((Dg, n), 2.0)
    x = np.arange(4 * Dg * n, dtype=np.float64).reshape(4 * Dg, n) / (4 * Dg * n)

    def run(J, status):
        return tref.winner(np.asarray(J, dtype=np.float64).reshape(-1), np.asarray(status).reshape(-1), x, lo, hi, True, Dg)

    def theta(r, a):
        return tref.box_map(x[r * Dg + a], lo[a], hi[a], True)
    # rows: restarts; columns: GPs.  GP 0: a tie between restarts 1 and 3 goes to 1; GP 1: the lowest J has status 3 and is left out
    J = [[3.0, 5.0], [1.0, 4.0], [2.0, -9.0], [1.0, 6.0]]
    status = [[0, 1], [2, 0], [1, 3], [0, 2]]
    out = run(J, status)
    assert out[0, :3].tolist() == [1.0, 1.0, 2.0] and np.array_equal(out[0, 3:], theta(1, 0))
    assert out[1, :3].tolist() == [4.0, 1.0, 0.0] and np.array_equal(out[1, 3:], theta(1, 1))
    # every restart of GP 0 has status 3: [+inf | -1 | 3 | theta of restart 0's x]; GP 1 is untouched by it
    status = [[3, 1], [3, 0], [3, 3], [3, 2]]
    out = run(J, status)
    assert out[0, :3].tolist() == [np.inf, -1.0, 3.0] and np.array_equal(out[0, 3:], theta(0, 0))
    assert out[1, :3].tolist() == [4.0, 1.0, 0.0]
    # an infinite J of a restart that is not status 3 still beats "none"; a single restart
    out = tref.winner(np.array([np.inf, 2.0]), np.array([0, 3]), x[:2], lo, hi, False, Dg)
    assert out[0, :3].tolist() == [np.inf, 0.0, 0.0] and out[1, :3].tolist() == [np.inf, -1.0, 3.0]
    assert np.array_equal(out[1, 3:], tref.box_map(x[1], lo[1], hi[1], False))


def test_a_theta_that_is_not_positive_definite_is_an_infinite_loss():
    w, lo, hi = setup()
    E = w.X.shape[1]
    theta = np.concatenate([w.lengthscales[0], [0.5, -1.0]])
    loss, g = tref.loss_and_grad_theta(w.X, w.Y[:, 0], theta)
    assert loss == np.inf and np.all(g == 0.0) and g.shape == (E + 2,)
    theta[0] = np.nan
    assert tref.loss_and_grad_theta(w.X, w.Y[:, 0], theta)[0] == np.inf
