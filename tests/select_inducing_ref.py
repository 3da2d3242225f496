"""numpy restatement of the greedy choice of inducing inputs of gpmpc_select_inducing (include/gpmpc.h), callable in float64 and
in longdouble: a pivoted partial Cholesky of the D kernel matrices K_a = k_a(X, X) run in lockstep over the outputs (greedy
variance selection: Burt et al. 2019; Fine & Scheinberg 2001).  State d_a(i) = sigma2_a, L_a (M x N) = 0; at step m

    s(i)  = sum_a max(d_a(i), 0) / sigma2_a                         (a ascending)
    p_m   = the unpicked point of largest s (lowest index on a tie; a score that is not finite ranks below every finite one)
    per a, if d_a(p) > jitter_rel sigma2_a:
        c(i) = (k_a(x_i, x_p) - sum_{j<m} L_a[j, i] L_a[j, p]) / sqrt(d_a(p)),   L_a[m, i] = c(i),   d_a(i) -= c(i)^2
    otherwise row m of L_a stays zero and d_a is unchanged (the pivot floor)
    trace[m] = sum_i s(i) after the update  =  sum_a tr(K_a - Q_a) / sigma2_a of the first m + 1 picks

plus the cases shared by the CPU and GPU tests.
"""
import functools

import numpy as np

import sparse_gp_ref as sgr
from oracle import extended_precision as xp

LD = np.longdouble
EPS = sgr.EPS
JITTER_REL = 1e-6


def scores(d, os_, dtype):
    s = np.zeros(d.shape[1], dtype=dtype)
    for a in range(d.shape[0]):
        s = s + np.where(d[a] < 0, dtype(0), d[a]) / dtype(os_[a])
    return s


def select(X, M, ls, os_, jitter_rel=JITTER_REL, dtype=np.float64):
    """dict(idx (M,) int64, trace (M,) dtype, gap (M,) float: (best - runner-up) / best over the distinct unpicked points at the
    step's choice (nan where there is no runner-up), floored (M, D) bool: the pivot floor acted)."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape[0], len(os_)
    assert 1 <= M <= N
    d = np.stack([np.full(N, dtype(os_[a]), dtype=dtype) for a in range(D)])
    L = np.zeros((D, M, N), dtype=dtype)
    picked = np.zeros(N, dtype=bool)
    idx = np.empty(M, dtype=np.int64)
    trace = np.empty(M, dtype=dtype)
    gap = np.full(M, np.nan)
    floored = np.zeros((M, D), dtype=bool)
    for m in range(M):
        s = scores(d, os_, dtype)
        key = np.where(np.isfinite(s), s, -np.inf)
        cand = np.flatnonzero(~picked)
        p = int(cand[np.argmax(key[cand])])                   # argmax: the first (= lowest) index of the largest
        rest = cand[cand != p]
        if len(rest):
            with np.errstate(invalid="ignore", divide="ignore"):
                gap[m] = float((key[p] - np.max(key[rest])) / key[p])
        idx[m] = p
        picked[p] = True
        for a in range(D):
            if not d[a, p] > dtype(jitter_rel) * dtype(os_[a]):
                floored[m, a] = True
                continue
            k = sgr.cross_gram(X, X[p:p + 1], ls[a], os_[a], dtype)[:, 0]
            c = (k - L[a, :m].T @ L[a, :m, p]) / np.sqrt(d[a, p])
            L[a, m] = c
            d[a] = d[a] - c * c
        trace[m] = np.sum(scores(d, os_, dtype))
    return {"idx": idx, "trace": trace, "gap": gap, "floored": floored}


def dense_trace(X, rows, ls, os_, dtype=LD):
    """sum_a (N sigma2_a - tr(Kfu Kuu^-1 Kuf)) / sigma2_a for the inducing inputs X[rows], by a dense Cholesky solve."""
    X = np.asarray(X, dtype=np.float64)
    t = dtype(0)
    for a in range(len(os_)):
        Kuu = sgr.cross_gram(X[rows], X[rows], ls[a], os_[a], dtype)
        Kuf = sgr.cross_gram(X[rows], X, ls[a], os_[a], dtype)
        V = xp.lower_inverse(xp.cholesky_lower(Kuu)) @ Kuf if dtype is LD else np.linalg.solve(np.linalg.cholesky(Kuu), Kuf)
        t = t + (dtype(X.shape[0]) * dtype(os_[a]) - np.sum(V * V)) / dtype(os_[a])
    return t


def exact_mean(X, Y, ls, os_, nz, Xq):
    """Posterior mean (Q, D) of the exact GP on the whole memory (float64)."""
    out = np.empty((len(Xq), len(os_)))
    for a in range(len(os_)):
        K = sgr.cross_gram(X, X, ls[a], os_[a], np.float64) + nz[a] * np.eye(len(X))
        out[:, a] = sgr.cross_gram(Xq, X, ls[a], os_[a], np.float64) @ np.linalg.solve(K, np.asarray(Y)[:, a])
    return out


def sparse_mean(X, Y, Z, ls, os_, nz, Xq, jitter_rel=JITTER_REL):
    iK, beta = sgr.sparse_factors(X, Y, Z, ls, os_, nz, jitter_rel)
    return sgr.predict(Z, ls, os_, iK, beta, Xq)[0]


# -- cases -------------------------------------------------------------------------------------------------------------------
CASE_NAMES = list(sgr.CASES) + ["n1_m1", "n65_m3", "n64_m64", "d1", "d16_e20", "floor_0.05", "floor_0.3", "dups",
                                "clustered_n600_m40"]
INDEX_CASES = [n for n in CASE_NAMES if n != "dups"]        # cases whose whole index sequence the GPU test compares


class Case:
    pass


def _functions(X):
    return np.stack([np.sin(3.0 * X[:, 0]) + X[:, 1] * X[:, 2], np.cos(2.0 * X[:, 1]) - 0.5 * X[:, 3],
                     X[:, 0] - X[:, 2] ** 2 + 0.3 * np.sin(5.0 * X[:, 3])], axis=1)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """X, M, lengthscales, outputscales and jitter_rel of a case (and Y, noises, queries where the case has them)."""
    c = Case()
    c.name, c.jitter_rel = name, JITTER_REL
    small = sgr.case("n37_m16")
    if name in sgr.CASES:
        b = sgr.case(name)
        c.X, c.M, c.ls, c.os = b.X, b.M, b.ls, b.os
    elif name in ("n1_m1", "n65_m3", "n64_m64"):
        N, M = {"n1_m1": (1, 1), "n65_m3": (65, 3), "n64_m64": (64, 64)}[name]
        c.X, c.M, c.ls, c.os = np.random.default_rng(2000 + N + M).uniform(0.0, 1.0, size=(N, 4)), M, small.ls, small.os
    elif name == "d1":
        b = sgr.case("n257_m70")
        c.X, c.M, c.ls, c.os = b.X, b.M, b.ls[:1], b.os[:1]
    elif name == "d16_e20":
        rng = np.random.default_rng(16)
        c.X, c.M = rng.uniform(0.0, 1.0, size=(130, 20)), 20
        c.ls, c.os = rng.uniform(1.5, 3.0, size=(16, 20)), rng.uniform(0.5, 1.5, size=16)
    elif name.startswith("floor_"):
        b = sgr.case("n257_m70")
        c.X, c.M, c.ls, c.os, c.jitter_rel = b.X, b.M, b.ls, b.os, float(name[len("floor_"):])
    elif name == "dups":
        c.X, c.M, c.ls, c.os = np.concatenate([small.X[:20], small.X[:20]]), 40, small.ls, small.os
    elif name == "clustered_n600_m40":
        rng = np.random.default_rng(5)
        c.X = np.concatenate([0.5 + 0.02 * rng.standard_normal((540, 4)), rng.uniform(0.0, 1.0, size=(60, 4))])
        c.M, c.ls, c.os, c.nz = 40, 0.4 * small.ls, np.array([1.0, 0.6, 1.5]), np.full(3, 1e-3)
        c.Y = _functions(c.X) + np.sqrt(1e-3) * rng.standard_normal((600, 3))
        c.Xq = rng.uniform(0.0, 1.0, size=(200, 4))
    else:
        raise KeyError(name)
    c.N, c.E, c.D = c.X.shape[0], c.X.shape[1], len(c.os)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case with, computed once and shared, its longdouble and float64 restatements and the float64 one's own
    trace error e64 (never taken from the code under test)."""
    c = inputs(name)
    c.ld = select(c.X, c.M, c.ls, c.os, c.jitter_rel, LD)
    c.f64 = select(c.X, c.M, c.ls, c.os, c.jitter_rel, np.float64)
    c.e64_trace = float(np.max(np.abs(c.f64["trace"] - c.ld["trace"])))
    c.tol_trace = 10.0 * c.e64_trace + 64.0 * EPS * float(np.max(np.abs(c.ld["trace"])))
    return c
