"""CPU tests of the recurrence of gpmpc_sparse_forget as restated in tests/sparse_forget_ref.py.  In longdouble the recurrence and
the from-scratch build of the reduced memory agree to 1e-15 relative: the algebra is right, what remains is rounding.  In float64
the recurrence stays within
    10 e_scratch + 64 eps scale        (e_scratch: the float64 from-scratch build's own error on the REDUCED memory)
of the longdouble build on every row of the table of DESIGN.md 4.4.5 but three: the two whose loss belongs to the formulation
(most of the data behind an inducing input leaves) and n20_m37 (11 x on the mean), which are printed.  iK_eff stays exactly
symmetric, a point that never was in the model loses the pivot, and append-then-forget returns to the start.  No GPU."""
import numpy as np
import pytest

import sparse_append_ref as ar
import sparse_forget_ref as fr
import sparse_gp_ref as ref

LONGDOUBLE_ROWS = ["n37_m16-8", "n257_m70-64", "n257_m64_time-9"]
PRINTED_ROWS = list(fr.LOSS_ROWS) + ["n20_m37-8"]
ASSERTED_ROWS = [n for n in fr.CASES if n not in PRINTED_ROWS]


def _report(c):
    print(f"{c.name}: recurrence mean {c.erec_mean:.2e} = {c.erec_mean / c.e64_mean:.1f} x e_scratch {c.e64_mean:.2e}   "
          f"var {c.erec_var:.2e} = {c.erec_var / c.e64_var:.1f} x e_scratch {c.e64_var:.2e}   min tau {c.rec64.min_tau:.1e}")


@pytest.mark.parametrize("name", LONGDOUBLE_ROWS)
def test_longdouble_recurrence_equals_the_longdouble_build_of_the_reduced_memory(name):
    c = fr.case(name)
    rld = fr.forgotten_record(c, fr.LD)
    full = fr.reduced_record(c, fr.LD)

    def rel(a, b):
        return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    figures = {"iK_eff": rel(rld.iK, full.iK), "Yb": rel(rld.Yb, full.Yb), "beta_eff": rel(rld.beta(), full.beta())}
    print(f"{name}: longdouble recurrence against longdouble build (relative): " + "  ".join(f"{k} {v:.1e}" for k, v in figures.items()))
    for k, v in figures.items():
        assert v <= 1e-15, k


@pytest.mark.parametrize("name", ASSERTED_ROWS)
def test_float64_recurrence_stays_inside_the_project_bound(name):
    c = fr.case(name)
    _report(c)
    assert c.erec_mean <= 10.0 * c.e64_mean + 64.0 * fr.EPS * c.scale_mean
    assert c.erec_var <= 10.0 * c.e64_var + 64.0 * fr.EPS * c.scale_var
    r = c.rec64
    assert np.array_equal(r.iK, np.swapaxes(r.iK, 1, 2))                           # exactly symmetric
    assert np.all(np.isfinite(r.iK)) and np.all(np.isfinite(r.Yb))
    for a in range(r.Yb.shape[0]):
        assert not np.any(np.triu(r.Yb[a], 1))                                     # Yb' stays lower triangular


@pytest.mark.parametrize("name", PRINTED_ROWS)
def test_rows_whose_loss_is_printed(name):
    """Not asserted against e_scratch: the two loss rows of the formulation, and n20_m37 (N < M).  The recurrence still runs
    through without losing a pivot, symmetric and finite."""
    c = fr.case(name)
    _report(c)
    r = c.rec64
    assert np.array_equal(r.iK, np.swapaxes(r.iK, 1, 2))
    assert np.all(np.isfinite(r.iK)) and np.all(np.isfinite(r.Yb))


def test_sliding_window_of_200_steps():
    """n257_m70, a window of 57 rows, 200 steps of append-newest + forget-oldest: against the window's longdouble build."""
    b = ref.case("n257_m70")
    n0, steps = 57, 200
    r = ar.build_record(b.X[:n0], b.Y[:n0], b.Z, b.ls, b.os, b.nz, ref.JITTER_REL, np.float64)
    for s in range(steps):
        ar.append(r, b.X[n0 + s:n0 + s + 1], b.Y[n0 + s:n0 + s + 1])
        fr.forget(r, b.X[s:s + 1], b.Y[s:s + 1])
    c = fr.Case()
    c.name = "n257_m70-window57x200"
    for f in ("Z", "ls", "os", "nz", "Xq", "X", "Y"):
        setattr(c, f, getattr(b, f))
    c.rec64 = r
    fr.tolerance(c, *fr.reference(c, np.arange(steps, steps + n0)), *fr.predict(c, r))
    _report(c)
    assert c.erec_mean <= 10.0 * c.e64_mean + 64.0 * fr.EPS * c.scale_mean
    assert c.erec_var <= 10.0 * c.e64_var + 64.0 * fr.EPS * c.scale_var
    assert np.array_equal(r.iK, np.swapaxes(r.iK, 1, 2))


def test_short_sliding_window_case_of_the_gpu_test():
    c = fr.sliding_window()
    _report(c)
    assert c.erec_mean <= 10.0 * c.e64_mean + 64.0 * fr.EPS * c.scale_mean
    assert c.erec_var <= 10.0 * c.e64_var + 64.0 * fr.EPS * c.scale_var


def test_a_point_that_never_was_in_the_model_loses_the_pivot():
    m1, built_on, gone = fr.lost_pivot_setup()
    for dtype in (np.float64, fr.LD):
        r = ar.build_record(m1.X[built_on], m1.Y[built_on], m1.Z, m1.ls, m1.os, m1.nz, ref.JITTER_REL, dtype)
        with pytest.raises(fr.LostPivot) as ei:
            fr.forget(r, m1.X[gone], m1.Y[gone])
        assert ei.value.point == 0 and ei.value.output == 0
    p2 = []
    for a in range(m1.D):                                            # every output on its own: p^T p = 3.2, 2.2, 1.8
        r = ar.build_record(m1.X[built_on], m1.Y[built_on][:, a:a + 1], m1.Z, m1.ls[a:a + 1], m1.os[a:a + 1], m1.nz[a:a + 1],
                            ref.JITTER_REL)
        with pytest.raises(fr.LostPivot) as ei:
            fr.forget(r, m1.X[gone], m1.Y[gone][:, a:a + 1])
        p2.append(ei.value.p2)
    print("m1, Z[0] forgotten from the model of row 1 alone: p^T p =", ", ".join(f"{v:.2f}" for v in p2))
    assert all(v > 1.0 for v in p2)


def test_append_then_forget_returns_to_the_start():
    c = ar.case("n37_m16_29+8")
    start = ar.build_record(c.X[:c.N0], c.Y[:c.N0], c.Z, c.ls, c.os, c.nz, ref.JITTER_REL)
    r = ar.appended_record(c)
    fr.forget(r, c.X[c.N0:], c.Y[c.N0:])
    w = fr.Case()
    for f in ("Z", "ls", "os", "nz", "Xq", "X", "Y"):
        setattr(w, f, getattr(c, f))
    fr.tolerance(w, *fr.reference(w, np.arange(c.N0)), *fr.predict(w, r))
    mean0, var0 = fr.predict(w, start)
    d_mean, d_var = float(np.max(np.abs(fr.predict(w, r)[0] - mean0))), float(np.max(np.abs(fr.predict(w, r)[1] - var0)))
    print(f"append 8 then forget 8: against the start mean {d_mean:.2e} (tol {w.tol_mean:.2e})  var {d_var:.2e} (tol {w.tol_var:.2e})")
    assert d_mean <= w.tol_mean and d_var <= w.tol_var
    assert w.erec_mean <= w.tol_mean and w.erec_var <= w.tol_var


def test_one_call_of_k_points_is_k_calls_of_one_point():
    c = fr.case("n37_m16-scattered")
    r = ar.build_record(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL)
    for q in c.gone:
        fr.forget(r, c.X[q:q + 1], c.Y[q:q + 1])
    assert np.array_equal(c.rec64.iK, r.iK) and np.array_equal(c.rec64.Yb, r.Yb) and np.array_equal(c.rec64.w, r.w)
