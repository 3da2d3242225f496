"""Tier 1 (CPU): the closed form gpmpc_predict computes, pinned to the reference's own code.

tests/golden/predict_batch*.npz hold predict_next_state_change (gp_model.py:112-180) at zero input
variance for 48 query points (memory points, points inside the input box, far points), made by
tools/gen_golden_predict.py.  At zero input variance the moment-matched S is diagonal with
S_aa = sigma2_a - k_a^T iK_a k_a and M_a = k_a^T beta_a: the GP posterior the GPU tests check against.
"""
import numpy as np
import pytest

from helpers import load, workload_of, rel_err

GOLDENS = ["predict_batch", "predict_batch_time"]


def closed_form(X, ls, os_, iK, beta, Xq):
    """(mean, var) (M, D) of the zero-mean RBF-ARD GPs at the query rows of Xq, numpy fp64."""
    D = beta.shape[0]
    mean = np.empty((Xq.shape[0], D))
    var = np.empty((Xq.shape[0], D))
    for a in range(D):
        d = (Xq[:, None, :] - X[None, :, :]) / ls[a]
        k = os_[a] * np.exp(-0.5 * np.sum(d * d, axis=-1))          # (M, N)
        mean[:, a] = k @ beta[a]
        var[:, a] = os_[a] - np.einsum("mi,ij,mj->m", k, iK[a], k)
    return mean, var


@pytest.mark.parametrize("name", GOLDENS)
def test_closed_form_reproduces_reference(name):
    g = load(name)
    w = workload_of(g)
    Xq, M, S = g["Xq"], g["M"], g["S"]
    D = w.Y.shape[1]
    assert Xq.shape == (48, w.X.shape[1]) and M.shape == (48, D) and S.shape == (48, D, D)
    mean, var = closed_form(w.X, w.lengthscales, w.outputscales, g["iK"], g["beta"], Xq)
    assert rel_err(mean, M) <= 1e-12          # scale-relative: k . beta is a small remainder of terms up to |beta| ~ 3e2
    assert np.max(np.abs(var - S[:, range(D), range(D)])) <= 1e-10
    # the off-diagonal of S is (beta_a . k_a)(beta_b . k_b) - M_a M_b, zero up to the rounding of the reference's pair sums:
    # measured <= 3e-12, the size of its diagonal's own rounding (4e-12 against the closed form above)
    off = S.copy()
    off[:, range(D), range(D)] = 0.0
    assert np.max(np.abs(off)) <= 1e-10
    assert np.all(off[g["kind"] == 2] == 0.0)


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_covers_the_three_regions(name):
    g = load(name)
    w = workload_of(g)
    D = w.Y.shape[1]
    var = g["S"][:, range(D), range(D)]
    kind = g["kind"]
    # memory points: the posterior variance is down at the noise level; far points: the prior (var = sigma2, mean = 0)
    assert np.all(var[kind == 0] < 20 * w.noises)
    assert np.all(var[kind == 1] < w.outputscales)
    assert np.all(var[kind == 2] == w.outputscales) and np.all(g["M"][kind == 2] == 0.0)


def test_step_zero_var_is_the_same_quantity():
    """The existing single-step golden at zero input variance is one more query point of the same closed form."""
    g = load("step_zero_var")
    w = workload_of(g)
    D = w.Y.shape[1]
    mean, var = closed_form(w.X, w.lengthscales, w.outputscales, g["iK"], g["beta"], g["in_mean"][None])
    assert np.max(np.abs(mean[0] - g["M"].ravel())) <= 1e-12 * np.max(np.abs(g["M"]))
    assert np.max(np.abs(var[0] - np.diag(g["S"])[:D])) <= 1e-10
