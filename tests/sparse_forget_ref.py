"""numpy restatement of gpmpc_sparse_forget (include/gpmpc.h), callable in float64 and in longdouble: the rank-one recurrence that
lets a memory point (x, y) leave the record gpmpc_prepare_sparse keeps (tests/sparse_append_ref.py: build_record),

    kz = k(Z, x),  v = Yu kz,  u = v / sqrt(n),  p = Yb u,  t_0 = 1, t_{i+1} = t_i - p_i^2,  tau = t_M
    LOST PIVOT if some t_{i+1} is not > 0 (NaN included), or tau < 1 / (2 (1 + sigma2 / n))
    g = Yu^T (Yb^T p)  (old Yb),   iK_eff -= g g^T / tau
    d_i = sqrt(t_{i+1} / t_i),  c_i = p_i / sqrt(t_i t_{i+1})
    per column j:  acc = 0;  for i = j .. M-1:  Yb'[i,j] = (Yb[i,j] + p_i acc) / d_i;  acc += c_i Yb'[i,j]
    w' = w - v y,   beta_eff' = Yu^T Yb'^T Yb' w' / n

(one function with the append: sparse_append_ref.update), plus the cases the CPU and GPU tests share: a memory, the rows that leave it, and per case, from numpy alone,

    e_scratch = the float64 from-scratch build of the REDUCED memory against its longdouble build
    e_rec     = the float64 recurrence against the same longdouble build
    tol       = 10 max(e_scratch, e_rec) + 64 eps scale          for mean and variance separately

(10: the project's margin for the sparse kernels, whose sums are grouped differently from numpy's; never taken from the code under
test).
"""
import functools

import numpy as np

import sparse_append_ref as ar
import sparse_gp_ref as ref

LD = ref.LD
EPS = ref.EPS


LostPivot = ar.LostPivot


def forget(r, X_old, Y_old):
    """The rows of (X_old (k, E), Y_old (k, D)) leave the record in place, in ascending row order: sparse_append_ref.update with
    the opposite sign.  Records min tau in r.min_tau."""
    return ar.update(r, X_old, Y_old, forget=True)


# -- cases --------------------------------------------------------------------------------------------------------------------------
# name -> (case of sparse_gp_ref or of sparse_append_ref.SMALL, rows of its memory that leave)
SCATTERED = (0, 5, 6, 17, 18, 30, 35, 36)
CASES = {
    "n37_m16-8": ("n37_m16", tuple(range(8))),
    "n37_m16-scattered": ("n37_m16", SCATTERED),
    "n257_m70-64": ("n257_m70", tuple(range(64))),
    "n257_m70-every4th": ("n257_m70", tuple(range(3, 257, 4))),
    "n257_m70-200": ("n257_m70", tuple(range(200))),
    "n257_m64_time-9": ("n257_m64_time", tuple(range(9))),
    "n150_m130-10": ("n150_m130", tuple(range(10))),
    "n20_m37-8": ("n20_m37", tuple(range(8))),
    "d1-8": ("d1", tuple(range(8))),
    "d16_e20-8": ("d16_e20", tuple(range(8))),
    "m1-1": ("m1", (0,)),
    # the two rows whose loss belongs to the formulation: printed, never asserted
    "n257_m64_time-200": ("n257_m64_time", tuple(range(200))),
    "n37_m16-all_but_last": ("n37_m16", tuple(range(36))),
}
LOSS_ROWS = ("n257_m64_time-200", "n37_m16-all_but_last")


class Case:
    pass


def _base(name):
    return ref.case(name) if name in ref.CASES else ar.case(name)


def reference(c, keep):
    """(mean, var) at the case's queries of the longdouble and of the float64 from-scratch builds of the rows `keep`."""
    iK_ld, beta_ld = ref.sparse_factors(c.X[keep], c.Y[keep], c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, LD)
    mean_ld, var_ld = ref.predict(c.Z, c.ls, c.os, iK_ld, beta_ld, c.Xq, LD)
    iK64, beta64 = ref.sparse_factors(c.X[keep], c.Y[keep], c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, np.float64)
    mean64, var64 = ref.predict(c.Z, c.ls, c.os, iK64, beta64, c.Xq, np.float64)
    return mean_ld, var_ld, mean64, var64


def tolerance(c, mean_ld, var_ld, mean64, var64, mean_rec, var_rec):
    """e_scratch, e_rec and tol = 10 max(e_scratch, e_rec) + 64 eps scale, for mean and variance, set on the case."""
    c.mean_ld, c.var_ld = mean_ld, var_ld
    c.e64_mean = float(np.max(np.abs(mean64 - mean_ld)))
    c.e64_var = float(np.max(np.abs(var64 - var_ld)))
    c.erec_mean = float(np.max(np.abs(mean_rec - mean_ld)))
    c.erec_var = float(np.max(np.abs(var_rec - var_ld)))
    c.scale_mean = float(np.max(np.abs(mean_ld)))
    c.scale_var = float(np.max(np.abs(var_ld)))
    c.tol_mean = 10.0 * max(c.e64_mean, c.erec_mean) + 64.0 * EPS * c.scale_mean
    c.tol_var = 10.0 * max(c.e64_var, c.erec_var) + 64.0 * EPS * c.scale_var
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """A case: the memory (X, Y), Z, hyper-parameters, queries, the rows `gone` that leave and `keep` that stay, the float64
    record after the recurrence (`rec64`), the longdouble reference of the REDUCED memory and the tolerance -- computed once and
    shared, never modified."""
    base, gone = CASES[name]
    b = _base(base)
    c = Case()
    c.name = name
    for f in ("N", "M", "D", "E", "X", "Y", "Z", "ls", "os", "nz", "Xq"):
        setattr(c, f, getattr(b, f))
    c.gone = np.array(gone, dtype=np.int64)
    c.keep = np.setdiff1d(np.arange(c.N), c.gone)
    c.rec64 = forgotten_record(c, np.float64)
    mean_rec, var_rec = predict(c, c.rec64)
    return tolerance(c, *reference(c, c.keep), mean_rec, var_rec)


def forgotten_record(c, dtype=np.float64):
    """The record built on the whole memory of the case with the rows `gone` removed by the recurrence."""
    r = ar.build_record(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, dtype)
    return forget(r, c.X[c.gone], c.Y[c.gone])


def reduced_record(c, dtype=np.float64):
    """The record of the reduced memory from scratch."""
    return ar.build_record(c.X[c.keep], c.Y[c.keep], c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, dtype)


def predict(c, r):
    return ref.predict(c.Z, c.ls, c.os, r.iK, r.beta(), c.Xq, r.dtype)


@functools.lru_cache(maxsize=None)
def sliding_window():
    """Build on rows 0-28 of n37_m16; 8 steps of append row 29 + s, forget row s: the model of rows 8-36.  The case carries the
    reference of that window and the tolerance from the float64 recurrence (append then forget, step by step)."""
    b = ref.case("n37_m16")
    c = Case()
    c.name = "n37_m16-window"
    for f in ("N", "M", "D", "E", "X", "Y", "Z", "ls", "os", "nz", "Xq"):
        setattr(c, f, getattr(b, f))
    c.n0, c.steps = 29, 8
    c.keep = np.arange(c.steps, c.n0 + c.steps)
    r = ar.build_record(c.X[:c.n0], c.Y[:c.n0], c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, np.float64)
    for s in range(c.steps):
        ar.append(r, c.X[c.n0 + s:c.n0 + s + 1], c.Y[c.n0 + s:c.n0 + s + 1])
        forget(r, c.X[s:s + 1], c.Y[s:s + 1])
    c.rec64 = r
    mean_rec, var_rec = predict(c, r)
    return tolerance(c, *reference(c, c.keep), mean_rec, var_rec)


def lost_pivot_setup():
    """The `m1` case (N = 2, M = 1, Z = row 0): the model built on row 1 alone, from which Z[0] = row 0 -- never in it -- is to
    leave.  Returns (case of sparse_append_ref, rows the model is built on, the row to forget)."""
    return ar.case("m1"), np.array([1]), np.array([0])
