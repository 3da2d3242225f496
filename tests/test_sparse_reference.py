"""Tier 1 (CPU): the numpy restatement of the sparse (DTC) GP that the GPU tests of gpmpc_prepare_sparse are measured against
(tests/sparse_gp_ref.py).  Its float64 evaluation is compared with its longdouble one on the GPU tests' cases -- the errors are
printed and capped, which keeps the GPU tolerance 10 e64 + 64 eps scale meaningful -- and the formulas are tied to the exact GP:
with Z = X the DTC predictor IS the exact one, up to the jitter."""
import numpy as np
import pytest

import sparse_gp_ref as ref
from oracle import extended_precision as xp

MEAN_CAP = 1e-10              # absolute (the means are of size 1 to 2)
VAR_CAP_REL = 1e-8            # times the outputscale


@pytest.mark.parametrize("name", list(ref.CASES))
def test_float64_restatement_against_longdouble(name):
    c = ref.case(name)
    e_mean = np.max(np.abs(c.mean64 - c.mean_ld), axis=0)
    e_var = np.max(np.abs(c.var64 - c.var_ld), axis=0)
    print(f"{name}: float64 vs longdouble  mean {c.e64_mean:.3e} (max |mean| {np.max(np.abs(c.mean_ld)):.3f})  "
          f"var {c.e64_var:.3e} (var in [{float(c.var_ld.min()):.3e}, {float(c.var_ld.max()):.3e}])  "
          f"GPU tolerances: mean {c.tol_mean:.3e} var {c.tol_var:.3e}")
    assert np.all(e_mean <= MEAN_CAP)
    assert np.all(e_var <= VAR_CAP_REL * c.os)
    # the cached factor is exactly symmetric, and the DTC variance is >= 0 up to that tolerance
    assert np.array_equal(c.iK64, np.swapaxes(c.iK64, 1, 2))
    assert np.all(c.var64 >= -VAR_CAP_REL * c.os)
    assert np.all(c.var_ld > 0)


@pytest.mark.parametrize("name", ["n257_m70", "n1000_m130"])
def test_rejected_orders_of_operations_lose_digits(name):
    """Why the order is pinned: the textbook form and the Gram-first form lose the mean by orders of magnitude more."""
    c = ref.case(name)
    for label, fn in (("textbook", ref.textbook_factors), ("gram first", ref.gram_first_factors)):
        iK, beta = fn(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL)
        mean, var = ref.predict(c.Z, c.ls, c.os, iK, beta, c.Xq)
        e_mean, e_var = np.max(np.abs(mean - c.mean_ld)), np.max(np.abs(var - c.var_ld))
        print(f"{name}: {label}: mean {e_mean:.3e} var {e_var:.3e}   (pinned order: mean {c.e64_mean:.3e} var {c.e64_var:.3e})")
        assert e_mean > 100 * c.e64_mean


def test_inducing_inputs_equal_to_the_memory_give_the_exact_gp():
    """Z = X: Kuu^-1 - (Kuu + K K / n)^-1 = (K + n I)^-1, so DTC is the exact GP but for the jitter delta = jitter_rel sigma2 on
    Kuu.  First-order perturbation bounds with lam = lambda_min(K) (40 well-separated points: cond(K) < 1e3):
        |d var|  <= 2 delta |k|^2 / lam^2                      (d Kuu^-1 <= delta / lam^2, the second term moves by less)
        |d mean| <= 2 delta |k| |K y| / (n (lam + lam^2 / n)^2)
    plus 10 x the float64 restatement's own error against longdouble."""
    rng = np.random.default_rng(5)
    N, E, D, jitter = 40, 4, 3, 1e-10
    X = rng.uniform(0.0, 1.0, size=(N, E))
    ls = np.stack([np.full(E, 0.25) * (1.0 + 0.2 * a) for a in range(D)])
    os_, nz = np.array([1.0, 0.6, 1.5]), np.full(D, 1e-3)
    Y = np.stack([np.sin(3.0 * X[:, 0]), np.cos(2.0 * X[:, 1]), X[:, 0] - X[:, 2] ** 2], axis=1)
    Xq = rng.uniform(0.0, 1.0, size=(50, E))
    iK_x, beta_x = xp.factorize(X, Y, ls, os_, nz)
    mean_x, var_x = ref.predict(X, ls, os_, iK_x, beta_x, Xq, ref.LD)
    iK_ld, beta_ld = ref.sparse_factors(X, Y, X, ls, os_, nz, jitter, ref.LD)
    mean_ld, var_ld = ref.predict(X, ls, os_, iK_ld, beta_ld, Xq, ref.LD)
    iK, beta = ref.sparse_factors(X, Y, X, ls, os_, nz, jitter)
    mean, var = ref.predict(X, ls, os_, iK, beta, Xq)
    for a in range(D):
        K = ref.cross_gram(X, X, ls[a], os_[a], np.float64)
        lam = float(np.linalg.eigvalsh(K).min())
        assert np.linalg.cond(K) < 1e3
        kn = float(np.max(np.linalg.norm(ref.cross_gram(Xq, X, ls[a], os_[a], np.float64), axis=1)))
        delta = jitter * os_[a]
        e64_mean, e64_var = np.max(np.abs(mean[:, a] - mean_ld[:, a])), np.max(np.abs(var[:, a] - var_ld[:, a]))
        tol_var = 2 * delta * kn ** 2 / lam ** 2 + 10 * e64_var
        tol_mean = 2 * delta * kn * np.linalg.norm(K @ Y[:, a]) / (nz[a] * (lam + lam ** 2 / nz[a]) ** 2) + 10 * e64_mean
        d_mean, d_var = np.max(np.abs(mean[:, a] - mean_x[:, a])), np.max(np.abs(var[:, a] - var_x[:, a]))
        print(f"output {a}: sparse(Z = X) vs exact  mean {d_mean:.3e} (bound {tol_mean:.3e})  var {d_var:.3e} (bound {tol_var:.3e})  "
              f"float64 vs longdouble  mean {e64_mean:.3e} var {e64_var:.3e}")
        assert d_mean <= tol_mean and d_var <= tol_var


def test_strided_rows():
    assert list(ref.strided_rows(257, 70)[:3]) == [0, 4, 7] and ref.strided_rows(257, 70)[-1] == 256
    assert list(ref.strided_rows(5, 1)) == [0]
    assert list(ref.strided_rows(10, 10)) == list(range(10))
    for N, M in ((37, 16), (257, 70), (1000, 130), (257, 64), (5, 2)):
        r = ref.strided_rows(N, M)
        assert len(set(r.tolist())) == M and r[0] == 0 and r[-1] == N - 1 and np.all(np.diff(r) > 0)
