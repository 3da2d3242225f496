"""Tier 1 (CPU): gradients of the GP posterior at deterministic query inputs, pinned to the reference's own autograd.

tests/golden/predict_grad_batch*.npz hold torch autograd through the reference's predict_next_state_change (gp_model.py:112-180)
at zero input variance, at the 48 queries of predict_batch*.npz, for three upstream sets (tools/gen_golden_predict_grad.py): the
gradient of <mean_bar, M> + sum_a var_bar_a S_aa with respect to the query.  A torch-autograd fp64 restatement of the closed
form (mean = k^T beta, var = sigma2 - k^T iK k) must reproduce them, and both must give the longdouble central differences of
oracle.extended_precision.moment_match_step at Sigma = 0 (tests/moments_fd.py), which evaluates the same quantity.
"""
import numpy as np
import pytest
import torch

from helpers import load, rel_err
from moments_fd import xfactors, directional

GOLDENS = ["predict_batch", "predict_batch_time"]


def closed_form_grad(X, ls, os_, iK, beta, Xq, mean_bar, var_bar):
    """d/dXq of <mean_bar, mean> + <var_bar, var> for the zero-mean RBF-ARD GPs, by torch autograd in fp64."""
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float64)  # noqa: E731
    X, ls, os_, iK, beta, mb, vb = (t(v) for v in (X, ls, os_, iK, beta, mean_bar, var_bar))
    x = t(Xq).clone().requires_grad_(True)
    loss = 0.0
    for a in range(beta.shape[0]):
        d = (x[:, None, :] - X[None, :, :]) / ls[a]
        k = os_[a] * torch.exp(-0.5 * torch.sum(d * d, dim=-1))          # (M, N)
        mean = k @ beta[a]
        var = os_[a] - torch.einsum("mi,ij,mj->m", k, iK[a], k)
        loss = loss + (mb[:, a] * mean).sum() + (vb[:, a] * var).sum()
    loss.backward()
    return x.grad.numpy()


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_covers_kinds_and_upstream_sets(name):
    g, gg = load(name), load(name.replace("predict_", "predict_grad_"))
    assert np.array_equal(g["Xq"], gg["Xq"]) and np.array_equal(g["kind"], gg["kind"])
    Mq, E = gg["Xq"].shape
    D = g["M"].shape[1]
    assert gg["mean_bar"].shape == (3, Mq, D) and gg["var_bar"].shape == (3, Mq, D) and gg["Xq_bar"].shape == (3, Mq, E)
    # set 0: mean_bar and var_bar; set 1: mean_bar only; set 2: var_bar only
    assert np.all(gg["mean_bar"][:2] != 0) and np.all(gg["var_bar"][[0, 2]] != 0)
    assert np.all(gg["var_bar"][1] == 0) and np.all(gg["mean_bar"][2] == 0)
    # far points: the prior, whose gradient is exactly zero; elsewhere a gradient that is not
    assert np.all(gg["Xq_bar"][:, gg["kind"] == 2] == 0.0)
    assert np.all(np.abs(gg["Xq_bar"][:, gg["kind"] == 1]).max(axis=-1) > 0)


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("up", [0, 1, 2])
def test_closed_form_reproduces_reference_autograd(name, up):
    g, gg = load(name), load(name.replace("predict_", "predict_grad_"))
    got = closed_form_grad(g["X"], g["lengthscales"], g["outputscales"], g["iK"], g["beta"], gg["Xq"], gg["mean_bar"][up],
                           gg["var_bar"][up])
    # on the scale of the file's largest gradient: the reference's diagonal of S cancels (beta.k)^2 against M^2, terms of the
    # mean's size, so its variance-only gradients (set 2, ~100 times smaller) carry rounding of that size
    scale = float(np.abs(gg["Xq_bar"]).max())
    assert float(np.max(np.abs(got - gg["Xq_bar"][up]))) <= 1e-10 * scale
    if up != 2:
        assert rel_err(got, gg["Xq_bar"][up]) < 1e-10


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("up", [0, 1, 2])
def test_gradients_match_longdouble_differences(name, up):
    g, gg = load(name), load(name.replace("predict_", "predict_grad_"))
    f = xfactors(g["X"], g["lengthscales"], g["outputscales"], g["iK"], g["beta"])
    ls = g["lengthscales"].min(axis=0)
    Mq, E = gg["Xq"].shape
    D = g["M"].shape[1]
    ours = closed_form_grad(g["X"], g["lengthscales"], g["outputscales"], g["iK"], g["beta"], gg["Xq"], gg["mean_bar"][up],
                            gg["var_bar"][up])
    rng = np.random.default_rng(200 + up)
    zs, zv = np.zeros((E, E)), np.zeros((E, D))
    rows = []
    for p in range(Mq):
        dm = rng.standard_normal(E) * ls
        # Richardson from steps 1e-4 and 5e-5: at 1e-6 and below, the rounding of sigma2 - k^T iK k in longdouble divided by
        # the step is already ~1e-9
        fd_h = [directional(f, gg["Xq"][p], zs, gg["mean_bar"][up, p], np.diag(gg["var_bar"][up, p]), zv, dm, zs, h)
                for h in (1e-4, 5e-5)]
        fd = (4.0 * fd_h[1] - fd_h[0]) / 3.0
        sc = float(np.abs(gg["Xq_bar"][up, p]) @ np.abs(dm))
        rows.append((p, float(gg["Xq_bar"][up, p] @ dm), float(ours[p] @ dm), fd, sc))
    top = max(r[4] for r in rows)
    for p, an_ref, an_ours, fd, sc in rows:
        assert abs(an_ref - fd) <= 1e-6 * sc + 1e-7 * top, (p, gg["kind"][p], an_ref, fd)
        assert abs(an_ours - fd) <= 1e-6 * sc + 1e-7 * top, (p, gg["kind"][p], an_ours, fd)
