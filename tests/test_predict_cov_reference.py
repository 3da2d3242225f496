"""Tier 1 (CPU): the closed form gpmpc_predict_cov computes (tests/predict_cov_ref.py), pinned to the reference's own code.

tests/golden/predict_batch*.npz hold predict_next_state_change at zero input variance for 48 query points together with the
reference's iK: its S_aa is the diagonal of the joint posterior covariance (tests/test_predict_reference.py).  The
off-diagonal part has no golden of the reference's (its plot reads the diagonal only), so it is pinned by a second,
independent evaluation: the Schur complement of the joint prior covariance of (memory, queries), which never forms iK.
"""
import numpy as np
import pytest

from helpers import load, workload_of
from predict_cov_ref import closed_form_cov, schur_cov

GOLDENS = ["predict_batch", "predict_batch_time"]


def _diag(C):
    return np.diagonal(C, axis1=1, axis2=2)          # (D, M)


@pytest.mark.parametrize("name", GOLDENS)
def test_diagonal_reproduces_reference(name):
    g = load(name)
    w = workload_of(g)
    D = w.Y.shape[1]
    C = closed_form_cov(w.X, w.lengthscales, w.outputscales, g["iK"], g["Xq"])
    assert C.shape == (D, 48, 48)
    err = float(np.max(np.abs(_diag(C).T - g["S"][:, range(D), range(D)])))
    print(f"{name}: diagonal vs the reference's S_aa {err:.3e}")
    assert err <= 1e-10                              # the bound of test_predict_reference.py for the same quantity


@pytest.mark.parametrize("name", GOLDENS)
def test_schur_complement_agrees(name):
    """Both ways have their diagonal pinned to the golden; the off-diagonal may disagree by 3 x what the diagonals do.
    Measured (numpy fp64): predict_batch diagonal 1.40e-12, off-diagonal 1.29e-12 (allowed 4.21e-12);
    predict_batch_time diagonal 3.91e-13, off-diagonal 3.85e-13 (allowed 1.17e-12)."""
    g = load(name)
    w = workload_of(g)
    D = w.Y.shape[1]
    C = closed_form_cov(w.X, w.lengthscales, w.outputscales, g["iK"], g["Xq"])
    S = schur_cov(w.X, w.lengthscales, w.outputscales, w.noises, g["Xq"])
    assert np.max(np.abs(_diag(S).T - g["S"][:, range(D), range(D)])) <= 1e-10
    e_diag = float(np.max(np.abs(_diag(C) - _diag(S))))
    diff = np.abs(C - S)
    diff[:, range(48), range(48)] = 0.0
    e_off = float(np.max(diff))
    print(f"{name}: Schur complement vs iK form: diagonal {e_diag:.3e}, off-diagonal {e_off:.3e}")
    assert e_diag <= 2e-10                           # each within 1e-10 of the golden
    assert e_off <= 3 * e_diag


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_forms_are_consistent(name, dtype):
    g = load(name)
    w = workload_of(g)
    D = w.Y.shape[1]
    Xq = g["Xq"]
    args = (w.X, w.lengthscales, w.outputscales, g["iK"])
    J = closed_form_cov(*args, Xq, dtype=dtype)
    assert J.dtype == dtype
    assert np.array_equal(J, np.swapaxes(J, 1, 2))                      # exactly symmetric
    # cross form of two subsets = the block of the joint form of their union, up to the symmetrisation
    ia, ib = np.arange(0, 30), np.arange(17, 48)
    X_ = closed_form_cov(*args, Xq[ia], Xq[ib], dtype=dtype)
    assert X_.shape == (D, 30, 31)
    block = J[:, ia][:, :, ib]
    # iK of the golden is symmetric to rounding only: the two orders of a pair differ by the rounding of the sums
    assert np.max(np.abs(X_ - block)) <= 1e-12 * np.max(w.outputscales) * 48
    XT = closed_form_cov(*args, Xq[ib], Xq[ia], dtype=dtype)
    assert np.allclose(0.5 * (X_ + np.swapaxes(XT, 1, 2)), block, rtol=0, atol=1e-15)
    # noise: on the diagonal of the joint form only
    Jn = closed_form_cov(*args, Xq, noises=w.noises, dtype=dtype)
    d = Jn - J
    assert np.allclose(_diag(d), np.asarray(w.noises, dtype=dtype)[:, None], rtol=0, atol=1e-15)
    d[:, range(48), range(48)] = 0.0
    assert np.all(d == 0.0)
    with pytest.raises(ValueError):
        closed_form_cov(*args, Xq[ia], Xq[ib], noises=w.noises)


def test_far_points_keep_the_prior():
    g = load("predict_batch")
    w = workload_of(g)
    far = g["Xq"][g["kind"] == 2]
    assert len(far) >= 2
    C = closed_form_cov(w.X, w.lengthscales, w.outputscales, g["iK"], far)
    assert np.all(_diag(C) == w.outputscales[:, None])
