"""numpy restatement of the sparse (DTC / projected-process) GP of gpmpc_prepare_sparse (include/gpmpc.h), callable in float64
and in longdouble -- the formulas of Quinonero-Candela & Rasmussen 2005, section 5, in the order of operations the header pins:

    Kuu = k(Z, Z) + jitter_rel sigma2 I,  Lu = chol(Kuu),  Yu = Lu^-1
    V   = Yu k(Z, X),  B = I + V V^T / n,  w = V y,  LB = chol(B),  Yb = LB^-1
    beta_eff = Yu^T Yb^T Yb w / n,   iK_eff = Yu^T (I - Yb^T Yb) Yu     (the bracket first; i <= j computed, mirrored)

plus the two alternatives the design rejected (`textbook_factors`, `gram_first_factors`) so that their loss can be shown, the
strided choice of inducing inputs, the prediction from (Z, iK_eff, beta_eff) and the test cases shared by the CPU and GPU tests.
"""
import functools

import numpy as np

from oracle import extended_precision as xp

LD = np.longdouble
EPS = 2.0 ** -52


def cross_gram(A, B, ls_a, var_a, dtype):
    """k_a(A, B) = sigma2_a exp(-1/2 sum_e ((a_e - b_e) / l_ae)^2), differences formed per element."""
    A, B, ls_a = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype), np.asarray(ls_a, dtype=dtype)
    sq = np.zeros((A.shape[0], B.shape[0]), dtype=dtype)
    for e in range(A.shape[1]):
        d = (A[:, None, e] - B[None, :, e]) / ls_a[e]
        sq += d * d
    return dtype(var_a) * np.exp(-sq / 2)


def _chol(A, dtype):
    return xp.cholesky_lower(A) if dtype is LD else np.linalg.cholesky(A)


def _lower_inverse(L, dtype):
    if dtype is LD:
        return xp.lower_inverse(L)
    N = L.shape[0]
    Y = np.zeros((N, N), dtype=dtype)
    for i in range(N):                                   # forward substitution on the identity, as xp.lower_inverse
        r = -(L[i, :i] @ Y[:i, :i + 1]) if i else np.zeros(1, dtype=dtype)
        r[i] += 1
        Y[i, :i + 1] = r / L[i, i]
    return Y


def _mirror_upper(C):
    U = np.triu(C)
    return U + np.triu(C, 1).T


def sparse_factors(X, Y, Z, ls, os_, nz, jitter_rel, dtype=np.float64):
    """(iK_eff (D, M, M), beta_eff (D, M)) in `dtype`, by the pinned order of operations."""
    Yt = np.asarray(Y, dtype=dtype)
    D, M = Yt.shape[1], np.asarray(Z).shape[0]
    iK = np.empty((D, M, M), dtype=dtype)
    beta = np.empty((D, M), dtype=dtype)
    I = np.eye(M, dtype=dtype)
    for a in range(D):
        n = dtype(nz[a])
        Kuu = cross_gram(Z, Z, ls[a], os_[a], dtype) + dtype(jitter_rel) * dtype(os_[a]) * I
        Yu = _lower_inverse(_chol(Kuu, dtype), dtype)
        V = Yu @ cross_gram(Z, X, ls[a], os_[a], dtype)
        Yb = _lower_inverse(_chol(I + (V @ V.T) / n, dtype), dtype)
        w = V @ Yt[:, a]
        beta[a] = Yu.T @ (Yb.T @ (Yb @ w)) / n
        iK[a] = _mirror_upper(Yu.T @ ((I - Yb.T @ Yb) @ Yu))
    return iK, beta


def textbook_factors(X, Y, Z, ls, os_, nz, jitter_rel, dtype=np.float64):
    """iK_eff = Kuu^-1 - (Kuu + Kuf Kfu / n)^-1, beta_eff = (Kuu + Kuf Kfu / n)^-1 Kuf y / n: the form the design rejects."""
    Yt = np.asarray(Y, dtype=dtype)
    D, M = Yt.shape[1], np.asarray(Z).shape[0]
    iK = np.empty((D, M, M), dtype=dtype)
    beta = np.empty((D, M), dtype=dtype)
    for a in range(D):
        n = dtype(nz[a])
        Kuu = cross_gram(Z, Z, ls[a], os_[a], dtype) + dtype(jitter_rel) * dtype(os_[a]) * np.eye(M, dtype=dtype)
        Kuf = cross_gram(Z, X, ls[a], os_[a], dtype)
        Yu = _lower_inverse(_chol(Kuu, dtype), dtype)
        Ys = _lower_inverse(_chol(Kuu + (Kuf @ Kuf.T) / n, dtype), dtype)
        beta[a] = Ys.T @ (Ys @ (Kuf @ Yt[:, a])) / n
        iK[a] = _mirror_upper(Yu.T @ Yu - Ys.T @ Ys)
    return iK, beta


def gram_first_factors(X, Y, Z, ls, os_, nz, jitter_rel, dtype=np.float64):
    """C = Kuf Kfu formed first and whitened afterwards (Yu C Yu^T): the second form the design rejects."""
    Yt = np.asarray(Y, dtype=dtype)
    D, M = Yt.shape[1], np.asarray(Z).shape[0]
    iK = np.empty((D, M, M), dtype=dtype)
    beta = np.empty((D, M), dtype=dtype)
    I = np.eye(M, dtype=dtype)
    for a in range(D):
        n = dtype(nz[a])
        Kuu = cross_gram(Z, Z, ls[a], os_[a], dtype) + dtype(jitter_rel) * dtype(os_[a]) * I
        Kuf = cross_gram(Z, X, ls[a], os_[a], dtype)
        Yu = _lower_inverse(_chol(Kuu, dtype), dtype)
        Yb = _lower_inverse(_chol(I + (Yu @ (Kuf @ Kuf.T) @ Yu.T) / n, dtype), dtype)
        w = Yu @ (Kuf @ Yt[:, a])
        beta[a] = Yu.T @ (Yb.T @ (Yb @ w)) / n
        iK[a] = _mirror_upper(Yu.T @ ((I - Yb.T @ Yb) @ Yu))
    return iK, beta


def predict(Z, ls, os_, iK, beta, Xq, dtype=np.float64):
    """(mean, var) (Q, D) at the rows of Xq from the cached form: k(x, Z) beta_eff and sigma2 - k(x, Z) iK_eff k(Z, x)."""
    D = beta.shape[0]
    Q = np.asarray(Xq).shape[0]
    mean = np.empty((Q, D), dtype=dtype)
    var = np.empty((Q, D), dtype=dtype)
    for a in range(D):
        k = cross_gram(Xq, Z, ls[a], os_[a], dtype)
        mean[:, a] = k @ np.asarray(beta[a], dtype=dtype)
        var[:, a] = dtype(os_[a]) - np.sum((k @ np.asarray(iK[a], dtype=dtype)) * k, axis=1)
    return mean, var


def strided_rows(N, M):
    """Rows round(i (N - 1) / (M - 1)), i = 0..M-1, of an N-point memory (M = 1: row 0) -- ModelConfig.num_inducing_points."""
    if M == 1:
        return np.zeros(1, dtype=np.int64)
    return np.array([int(round(i * (N - 1) / (M - 1))) for i in range(M)], dtype=np.int64)


# -- the cases of the issue: D = 3, inputs uniform in [0, 1]^4 (+ a time input), Z the strided subset ---------------------------
CASES = {"n37_m16": (37, 16, 4), "n257_m70": (257, 70, 4), "n1000_m130": (1000, 130, 4), "n257_m64_time": (257, 64, 5)}
JITTER_REL = 1e-6
NOISE = 1e-3
N_QUERIES = 50


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs of a case and, computed once and shared, its longdouble and float64 restatements at the queries with the float64
    one's own errors e64 (never taken from the code under test)."""
    N, M, E = CASES[name]
    D = 3
    rng = np.random.default_rng(1000 + N + M + E)
    c = Case()
    c.name, c.N, c.M, c.D, c.E = name, N, M, D, E
    c.X = rng.uniform(0.0, 1.0, size=(N, E))
    Xq = rng.uniform(0.0, 1.0, size=(N_QUERIES, E))
    base = np.array([0.7, 0.9, 1.1, 1.3])
    c.ls = np.stack([base * (1.0 + 0.2 * a) for a in range(D)])
    if E == 5:                                            # a time input: the step index, a long lengthscale per output
        c.X[:, 4] = np.arange(N)
        Xq[:, 4] = rng.uniform(0.0, N - 1.0, size=N_QUERIES)
        c.ls = np.concatenate([c.ls, np.array([[150.0], [200.0], [250.0]])], axis=1)
    c.Xq = Xq
    c.os = np.array([1.0, 0.6, 1.5])
    c.nz = np.full(D, NOISE)
    f = np.stack([np.sin(3.0 * c.X[:, 0]) + c.X[:, 1] * c.X[:, 2], np.cos(2.0 * c.X[:, 1]) - 0.5 * c.X[:, 3],
                  c.X[:, 0] - c.X[:, 2] ** 2 + 0.3 * np.sin(5.0 * c.X[:, 3])], axis=1)
    c.Y = f + np.sqrt(NOISE) * rng.standard_normal((N, D))
    c.Z = c.X[strided_rows(N, M)].copy()
    iK_ld, beta_ld = sparse_factors(c.X, c.Y, c.Z, c.ls, c.os, c.nz, JITTER_REL, LD)
    c.mean_ld, c.var_ld = predict(c.Z, c.ls, c.os, iK_ld, beta_ld, c.Xq, LD)
    c.iK64, c.beta64 = sparse_factors(c.X, c.Y, c.Z, c.ls, c.os, c.nz, JITTER_REL, np.float64)
    c.mean64, c.var64 = predict(c.Z, c.ls, c.os, c.iK64, c.beta64, c.Xq, np.float64)
    c.e64_mean = float(np.max(np.abs(c.mean64 - c.mean_ld)))
    c.e64_var = float(np.max(np.abs(c.var64 - c.var_ld)))
    c.tol_mean = 10.0 * c.e64_mean + 64.0 * EPS * float(np.max(np.abs(c.mean_ld)))
    c.tol_var = 10.0 * c.e64_var + 64.0 * EPS * float(np.max(np.abs(c.var_ld)))
    return c
