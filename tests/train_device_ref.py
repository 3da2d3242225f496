"""Numpy restatement of the device hyper-parameter search (csrc/mll_batch.hip: gpmpc_mll_batch, gpmpc_train_search): the box map
and its chain rule, the loop as the oracle's loss plus the restated L-BFGS step, and the per-GP winner rule.  TEST CODE ONLY.

A parameter row is [lengthscale (E) | outputscale | noise], n = E + 2; problem p = r D + a is restart r of GP a.  The box is a
pair (lo, hi) of (D, n) arrays; the optimiser works on x in [0, 1]^n.
"""
import numpy as np

import lbfgs_device_ref as lref
from oracle import extended_precision as xp
from oracle import gp_training

LD = np.longdouble


def box_map(x, lo, hi, log_scale, dtype=np.float64):
    """theta = lo + (hi - lo) x, or lo (hi / lo)^x."""
    x, lo, hi = (np.asarray(v, dtype=dtype) for v in (x, lo, hi))
    if log_scale:
        return lo * (hi / lo) ** x
    return lo + (hi - lo) * x


def box_chain(theta, lo, hi, log_scale, dtype=np.float64):
    """d theta / d x at theta = box_map(x): hi - lo, or theta ln(hi / lo)."""
    theta, lo, hi = (np.asarray(v, dtype=dtype) for v in (theta, lo, hi))
    if log_scale:
        return theta * np.log(hi / lo)
    return (hi - lo) + 0 * theta


def box_unmap(theta, lo, hi, log_scale):
    """x of a theta inside the box (float64; 0 where the box is a point)."""
    theta, lo, hi = (np.asarray(v, dtype=np.float64) for v in (theta, lo, hi))
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.log(theta / lo) / np.log(hi / lo) if log_scale else (theta - lo) / (hi - lo)
    return np.where(np.isfinite(x), x, 0.0)


def loss_and_grad_theta(X, y, theta):
    """oracle.gp_training.neg_mll_and_grad on a parameter row: (loss, gradient (n,)); (+inf, 0) where K + noise I is not positive
    definite or theta is not finite -- what gpmpc_mll_batch answers there."""
    E = X.shape[1]
    theta = np.asarray(theta, dtype=np.float64)
    try:
        if not np.all(np.isfinite(theta)):
            raise np.linalg.LinAlgError("theta is not finite")
        loss, g_ls, g_os, g_nz = gp_training.neg_mll_and_grad(X, y, theta[:E], theta[E], theta[E + 1])
    except np.linalg.LinAlgError:
        return np.inf, np.zeros(E + 2)
    return float(loss), np.concatenate([g_ls, [g_os, g_nz]])


def loss_and_grad_x(X, y, x, lo, hi, log_scale):
    """The loss at theta = box_map(x) and its gradient wrt x: (loss, gradient (n,), theta (n,))."""
    theta = box_map(x, lo, hi, log_scale)
    loss, g = loss_and_grad_theta(X, y, theta)
    return loss, g * box_chain(theta, lo, hi, log_scale), theta


def loss_longdouble(X, y, theta):
    """The same loss with every operation in longdouble (the yardstick of the finite differences)."""
    E = X.shape[1]
    theta = np.asarray(theta, dtype=LD)
    N = X.shape[0]
    K = xp.gram(X, theta[None, :E], theta[E:E + 1])[0] + theta[E + 1] * np.eye(N, dtype=LD)
    L = xp.cholesky_lower(K)
    z = xp.lower_inverse(L) @ np.asarray(y, dtype=LD)
    return (LD(0.5) * (z @ z) + np.sum(np.log(np.diag(L))) + LD(0.5) * N * np.log(2 * LD(np.pi))) / N


def loss_longdouble_x(X, y, x, lo, hi, log_scale):
    return loss_longdouble(X, y, box_map(x, lo, hi, log_scale, dtype=LD))


def evaluate(X, Y, actions, lo, hi, log_scale):
    """gpmpc_mll_batch of the state's `actions` (P, n) with the box: (J (P,), G (P, n))."""
    D = Y.shape[1]
    P, n = actions.shape
    J, G = np.empty(P), np.empty((P, n))
    for p in range(P):
        a = p % D
        J[p], G[p], _ = loss_and_grad_x(X, Y[:, a], actions[p], lo[a], hi[a], log_scale)
    return J, G


def search(X, Y, x0, lo, hi, log_scale, iterations, history, c1=1e-4, pgtol=1e-5, first_iteration=0, state=None):
    """gpmpc_train_search: init from x0 (R, D, n) (first_iteration == 0), then `iterations` x [evaluate the state's actions; the
    restated lbfgs step].  Returns (state, list of the J arrays after every step)."""
    R, D, n = np.asarray(x0).shape if state is None else (state["x"].shape[0] // Y.shape[1], Y.shape[1], state["x"].shape[1])
    if first_iteration == 0:
        state = lref.init(np.asarray(x0, dtype=np.float64).reshape(R * D, n), 1, n, history)
    trace = []
    for it in range(iterations):
        J, G = evaluate(X, Y, state["actions"], lo, hi, log_scale)
        state, _ = lref.step(state, J, G.reshape(R * D, 1, n), first_iteration + it, 1, n, history, c1, pgtol)
        trace.append(state["J"].copy())
    return state, trace


def winner(J, status, x, lo, hi, log_scale, D):
    """best_out (D, 3 + n) of gpmpc_train_search from the state's J (P,), status (P,), x (P, n): per GP the lowest J over the
    restarts whose status != 3, ties to the lowest restart; [+inf | -1 | 3 | theta of restart 0's x] where there is none."""
    J, status, x = np.asarray(J, dtype=np.float64), np.asarray(status), np.asarray(x, dtype=np.float64)
    P, n = x.shape
    R = P // D
    out = np.empty((D, 3 + n))
    for a in range(D):
        best, br = np.inf, -1
        for r in range(R):
            p = r * D + a
            if status[p] != 3 and (br < 0 and not np.isnan(J[p]) or J[p] < best):
                best, br = J[p], r
        src = max(br, 0) * D + a
        out[a, 0] = best if br >= 0 else np.inf
        out[a, 1] = br
        out[a, 2] = status[br * D + a] if br >= 0 else 3
        out[a, 3:] = box_map(x[src], lo[a], hi[a], log_scale)
    return out
