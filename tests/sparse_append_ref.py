"""numpy restatement of gpmpc_sparse_append (include/gpmpc.h), callable in float64 and in longdouble: the record
gpmpc_prepare_sparse keeps (Yu, Yb, w per output, by the order of operations of tests/sparse_gp_ref.py) and the rank-one recurrence
that lets one more memory point (x, y) join it,

    kz = k(Z, x),  v = Yu kz,  u = v / sqrt(n),  p = Yb u,  t_0 = 1, t_{i+1} = t_i + p_i^2,  tau = t_M
    g = Yu^T (Yb^T p)  (old Yb),   iK_eff += g g^T / tau
    d_i = sqrt(t_{i+1} / t_i),  c_i = p_i / sqrt(t_i t_{i+1})
    per column j:  acc = 0;  for i = j .. M-1:  Yb'[i,j] = (Yb[i,j] - p_i acc) / d_i;  acc += c_i Yb'[i,j]
    w' = w + v y,   beta_eff' = Yu^T Yb'^T Yb' w' / n

(`update`; with `forget` the same recurrence with the opposite sign and the pivot check, as tests/sparse_forget_ref.py states it),
plus the cases the CPU and GPU tests share: the memory splits of sparse_gp_ref's cases and a few small ones of other shapes, each
with its tolerance computed as sparse_gp_ref.case computes it (10 x the from-scratch float64 error + 64 eps scale, for the FULL
memory; never taken from the code under test).
"""
import functools

import numpy as np

import sparse_gp_ref as ref

LD = ref.LD
EPS = ref.EPS


class Record:
    """What gpmpc_prepare_sparse leaves for the append, per output: Yu, Yb (D, M, M), w (D, M), iK_eff (D, M, M)."""

    def beta(self):
        return np.stack([self.Yu[a].T @ (self.Yb[a].T @ (self.Yb[a] @ self.w[a])) / self.dtype(self.nz[a])
                         for a in range(len(self.nz))])


def build_record(X, Y, Z, ls, os_, nz, jitter_rel, dtype=np.float64):
    """The record of the memory (X, Y) from scratch, by sparse_gp_ref.sparse_factors' order of operations."""
    Yt = np.asarray(Y, dtype=dtype)
    D, M = Yt.shape[1], np.asarray(Z).shape[0]
    r = Record()
    r.dtype, r.Z, r.ls, r.os, r.nz = dtype, np.asarray(Z), np.asarray(ls), np.asarray(os_), np.asarray(nz)
    r.Yu = np.empty((D, M, M), dtype=dtype)
    r.Yb = np.empty((D, M, M), dtype=dtype)
    r.w = np.empty((D, M), dtype=dtype)
    r.iK = np.empty((D, M, M), dtype=dtype)
    I = np.eye(M, dtype=dtype)
    for a in range(D):
        n = dtype(nz[a])
        Kuu = ref.cross_gram(Z, Z, ls[a], os_[a], dtype) + dtype(jitter_rel) * dtype(os_[a]) * I
        Yu = ref._lower_inverse(ref._chol(Kuu, dtype), dtype)
        V = Yu @ ref.cross_gram(Z, X, ls[a], os_[a], dtype)
        Yb = ref._lower_inverse(ref._chol(I + (V @ V.T) / n, dtype), dtype)
        r.Yu[a], r.Yb[a], r.w[a] = Yu, Yb, V @ Yt[:, a]
        r.iK[a] = ref._mirror_upper(Yu.T @ ((I - Yb.T @ Yb) @ Yu))
    return r


class LostPivot(ArithmeticError):
    """The check of the forget's t chain failed: `point` (row of the call) and `output`."""

    def __init__(self, point, output, p2):
        super().__init__(f"sparse forget: point {point}, output {output}: the pivot is lost (p^T p = {float(p2):.3g})")
        self.point, self.output, self.p2 = point, output, float(p2)


def update(r, X_pts, Y_pts, forget=False):
    """The rows of (X_pts (k, E), Y_pts (k, D)) join the record in place -- or, with `forget`, leave it: the same recurrence with
    the opposite sign (tests/sparse_forget_ref.py), which raises LostPivot and records min tau in r.min_tau -- in ascending row
    order."""
    dtype = r.dtype
    X_pts, Y_pts = np.asarray(X_pts, dtype=dtype), np.asarray(Y_pts, dtype=dtype)
    D, M = r.w.shape
    one = dtype(1)
    s = -one if forget else one                              # a + s b is a + b or a - b bit for bit: the product with +-1 is exact
    for q in range(X_pts.shape[0]):
        for a in range(D):
            Yu, Yb = r.Yu[a], r.Yb[a]
            n = dtype(r.nz[a])
            kz = ref.cross_gram(r.Z, X_pts[q:q + 1], r.ls[a], r.os[a], dtype)[:, 0]
            v = Yu @ kz
            u = v / np.sqrt(n)
            p = Yb @ u
            t = np.empty(M + 1, dtype=dtype)
            t[0] = one
            lost = False
            for i in range(M):
                t[i + 1] = t[i] + s * (p[i] * p[i])
                lost = lost or not (t[i + 1] > 0)
            if forget:
                if lost or t[M] < one / (2 * (one + dtype(r.os[a]) / n)):
                    raise LostPivot(q, a, p @ p)
                r.min_tau = min(getattr(r, "min_tau", 1.0), float(t[M]))
            g = Yu.T @ (Yb.T @ p)
            r.iK[a] = r.iK[a] + s * ref._mirror_upper(np.outer(g, g) / t[M])
            d = np.sqrt(t[1:] / t[:-1])
            c = p / np.sqrt(t[:-1] * t[1:])
            acc = np.zeros(M, dtype=dtype)
            Yn = np.zeros((M, M), dtype=dtype)
            for i in range(M):                               # row i of every column j <= i at once: the columns are independent
                Yn[i, :i + 1] = (Yb[i, :i + 1] - s * (p[i] * acc[:i + 1])) / d[i]
                acc[:i + 1] += c[i] * Yn[i, :i + 1]
            r.Yb[a] = Yn
            r.w[a] = r.w[a] + s * (v * Y_pts[q, a])
    return r


def append(r, X_new, Y_new):
    """The rows of (X_new (k, E), Y_new (k, D)) join the record in place, in ascending row order."""
    return update(r, X_new, Y_new)


# -- cases --------------------------------------------------------------------------------------------------------------------------
# name -> (case of sparse_gp_ref or None, points the record is built on, points appended); the splits of the issue's table
SPLITS = {
    "n37_m16_29+8": ("n37_m16", 29, 8),
    "n257_m70_193+64": ("n257_m70", 193, 64),
    "n257_m70_57+200": ("n257_m70", 57, 200),
    "n257_m64_time_57+200": ("n257_m64_time", 57, 200),
    "n257_m64_time_248+9": ("n257_m64_time", 248, 9),
}
# small cases of other shapes: name -> (N, M, D, E, N0); Z strided over the N points unless said
SMALL = {
    "m1": (2, 1, 3, 4, 1),
    "n150_m130": (150, 130, 3, 4, 140),
    "n20_m37": (20, 37, 3, 4, 12),                           # fewer points than inducing inputs: Z = the 37 points of n37_m16
    "d1": (37, 16, 1, 4, 29),
    "d16_e20": (40, 20, 16, 20, 32),
}


class Case:
    pass


def _finish(c):
    """The longdouble and float64 from-scratch restatements of the FULL memory at the queries, and the tolerance from them."""
    iK_ld, beta_ld = ref.sparse_factors(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, LD)
    c.mean_ld, c.var_ld = ref.predict(c.Z, c.ls, c.os, iK_ld, beta_ld, c.Xq, LD)
    iK64, beta64 = ref.sparse_factors(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, np.float64)
    mean64, var64 = ref.predict(c.Z, c.ls, c.os, iK64, beta64, c.Xq, np.float64)
    c.e64_mean = float(np.max(np.abs(mean64 - c.mean_ld)))
    c.e64_var = float(np.max(np.abs(var64 - c.var_ld)))
    c.tol_mean = 10.0 * c.e64_mean + 64.0 * EPS * float(np.max(np.abs(c.mean_ld)))
    c.tol_var = 10.0 * c.e64_var + 64.0 * EPS * float(np.max(np.abs(c.var_ld)))
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """A case: the full memory (X, Y), Z, hyper-parameters, queries, N0 (the record is built on the first N0 rows, the others are
    appended), and the longdouble reference and tolerance of the full memory -- computed once and shared."""
    c = Case()
    c.name = name
    if name in SPLITS:
        base, c.N0, k = SPLITS[name]
        b = ref.case(base)
        assert c.N0 + k == b.N
        for f in ("N", "M", "D", "E", "X", "Y", "Z", "ls", "os", "nz", "Xq", "mean_ld", "var_ld", "e64_mean", "e64_var", "tol_mean",
                  "tol_var"):
            setattr(c, f, getattr(b, f))
        return c
    N, M, D, E, c.N0 = SMALL[name]
    c.N, c.M, c.D, c.E = N, M, D, E
    if name == "n20_m37":
        b = ref.case("n37_m16")
        c.X, c.Y, c.Z, c.ls, c.os, c.nz, c.Xq = b.X[:N], b.Y[:N], b.X.copy(), b.ls, b.os, b.nz, b.Xq
        return _finish(c)
    rng = np.random.default_rng(2000 + N + M + D + E)
    c.X = rng.uniform(0.0, 1.0, size=(N, E))
    c.Xq = rng.uniform(0.0, 1.0, size=(ref.N_QUERIES, E))
    base = np.sqrt(E / 4.0) * (0.7 + 0.6 * np.arange(E) / max(E - 1, 1))         # longer with E: the squared distance grows with it
    c.ls = np.stack([base * (1.0 + 0.2 * (a % 5)) for a in range(D)])
    c.os = 0.6 + 0.9 * ((np.arange(D) * 7) % 11) / 10.0
    c.nz = np.full(D, ref.NOISE)
    f = np.stack([np.sin(3.0 * c.X[:, a % E]) + c.X[:, (a + 1) % E] * c.X[:, (a + 2) % E] - 0.1 * a for a in range(D)], axis=1)
    c.Y = f + np.sqrt(ref.NOISE) * rng.standard_normal((N, D))
    c.Z = c.X[ref.strided_rows(N, M)].copy()
    return _finish(c)


def appended_record(c, dtype=np.float64):
    """The record built on the first N0 rows of the case with the other rows appended by the recurrence."""
    r = build_record(c.X[:c.N0], c.Y[:c.N0], c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, dtype)
    return append(r, c.X[c.N0:], c.Y[c.N0:])


def predict(c, r):
    return ref.predict(c.Z, c.ls, c.os, r.iK, r.beta(), c.Xq, r.dtype)
