"""CPU tests of the recurrence of gpmpc_sparse_append as restated in tests/sparse_append_ref.py: appended to, a sparse model stays
as close to the longdouble from-scratch build of the whole memory as the project asks of gpmpc_prepare_sparse itself
    tolerance = 10 e64 + 64 eps scale        (e64: the from-scratch float64 restatement's own error on the FULL memory)
with iK_eff exactly symmetric and Yb lower triangular, Yb' is the inverse Cholesky factor of the rebuilt B, and in longdouble the
recurrence and the from-scratch build agree to 1e-15 relative: the algebra is right, what remains is rounding.  No GPU."""
import numpy as np
import pytest

import sparse_append_ref as ar
import sparse_gp_ref as ref

# every row of the table of DESIGN.md 4.4.4 but the 800-point one
ROWS = ["n37_m16_29+8", "n257_m70_193+64", "n257_m70_57+200", "n257_m64_time_57+200"]


@pytest.fixture(scope="module")
def appended():
    """name -> (float64 record, longdouble record) after the appends, computed once and shared, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            c = ar.case(name)
            cache[name] = (ar.appended_record(c, np.float64), ar.appended_record(c, ar.LD))
        return cache[name]
    return get


@pytest.mark.parametrize("name", ROWS)
def test_float64_recurrence_stays_inside_the_project_bound(appended, name):
    c = ar.case(name)
    r64, _ = appended(name)
    mean, var = ar.predict(c, r64)
    e_mean = float(np.max(np.abs(mean - c.mean_ld)))
    e_var = float(np.max(np.abs(var - c.var_ld)))
    print(f"{name}: append mean {e_mean:.2e} = {e_mean / c.e64_mean:.2f} x e64 (tol {c.tol_mean:.2e})   "
          f"var {e_var:.2e} = {e_var / c.e64_var:.2f} x e64 (tol {c.tol_var:.2e})")
    assert e_mean <= c.tol_mean
    assert e_var <= c.tol_var


@pytest.mark.parametrize("name", ROWS)
def test_factors_keep_their_structure(appended, name):
    r64, _ = appended(name)
    assert np.array_equal(r64.iK, np.swapaxes(r64.iK, 1, 2))                       # exactly symmetric
    assert np.all(np.isfinite(r64.iK)) and np.all(np.isfinite(r64.Yb))
    for a in range(r64.Yb.shape[0]):
        assert not np.any(np.triu(r64.Yb[a], 1))                                   # Yb' stays lower triangular
        assert np.all(np.diag(r64.Yb[a]) > 0)


@pytest.mark.parametrize("name", ROWS)
def test_yb_is_the_inverse_cholesky_factor_of_the_rebuilt_b(appended, name):
    """Against the longdouble from-scratch Yb of the full memory, by the rule of the predictions: 10 x the from-scratch float64
    factor's own error + 64 eps scale."""
    c = ar.case(name)
    r64, _ = appended(name)
    full_ld = ar.build_record(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, ar.LD)
    full64 = ar.build_record(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, np.float64)
    e64 = float(np.max(np.abs(full64.Yb - full_ld.Yb)))
    tol = 10.0 * e64 + 64.0 * ar.EPS * float(np.max(np.abs(full_ld.Yb)))
    err = float(np.max(np.abs(r64.Yb - full_ld.Yb)))
    e_w = float(np.max(np.abs(r64.w - full_ld.w)))
    tol_w = 10.0 * float(np.max(np.abs(full64.w - full_ld.w))) + 64.0 * ar.EPS * float(np.max(np.abs(full_ld.w)))
    print(f"{name}: Yb' {err:.2e} = {err / e64:.2f} x e64 (tol {tol:.2e})   w' {e_w:.2e} (tol {tol_w:.2e})")
    assert err <= tol
    assert e_w <= tol_w


@pytest.mark.parametrize("name", ROWS)
def test_longdouble_recurrence_equals_the_longdouble_build(appended, name):
    """"The build" is what the handle holds: iK_eff, beta_eff and the record Yb, w, each relative to its largest entry, and the
    predicted mean.  The predicted variance sigma2 - k iK_eff k is printed, not asserted: it is the difference of terms up to
    max|iK_eff| ~ 1e3..1e6 times its own size, so two longdouble builds that agree to 1e-19 in every factor differ by 1e-14 of
    it (n37_m16: 1.7e-14) -- conditioning of the query, not of the recurrence."""
    c = ar.case(name)
    _, rld = appended(name)
    full = ar.build_record(c.X, c.Y, c.Z, c.ls, c.os, c.nz, ref.JITTER_REL, ar.LD)

    def rel(a, b):
        return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    mean, var = ar.predict(c, rld)
    figures = {"iK_eff": rel(rld.iK, full.iK), "beta_eff": rel(rld.beta(), full.beta()), "Yb": rel(rld.Yb, full.Yb),
               "w": rel(rld.w, full.w), "mean": rel(mean, c.mean_ld)}
    print(f"{name}: longdouble recurrence against longdouble build (relative): "
          + "  ".join(f"{k} {v:.1e}" for k, v in figures.items()) + f"  [var {rel(var, c.var_ld):.1e}]")
    for k, v in figures.items():
        assert v <= 1e-15, k


def test_one_call_of_k_points_is_k_calls_of_one_point():
    c = ar.case("n37_m16_29+8")
    one = ar.appended_record(c)
    r = ar.build_record(c.X[:c.N0], c.Y[:c.N0], c.Z, c.ls, c.os, c.nz, ref.JITTER_REL)
    for q in range(c.N0, c.N):
        ar.append(r, c.X[q:q + 1], c.Y[q:q + 1])
    assert np.array_equal(one.iK, r.iK) and np.array_equal(one.Yb, r.Yb) and np.array_equal(one.w, r.w)


@pytest.mark.parametrize("name", list(ar.SMALL))
def test_small_cases_of_other_shapes(name):
    """The shapes the GPU test adds (M = 1, N0 < M, D = 1, D = 16 with E = 20, M = 130): the restatement itself meets their bound."""
    c = ar.case(name)
    r64 = ar.appended_record(c)
    mean, var = ar.predict(c, r64)
    e_mean, e_var = float(np.max(np.abs(mean - c.mean_ld))), float(np.max(np.abs(var - c.var_ld)))
    print(f"{name}: append mean {e_mean:.2e} (tol {c.tol_mean:.2e})  var {e_var:.2e} (tol {c.tol_var:.2e})")
    assert e_mean <= c.tol_mean and e_var <= c.tol_var
    assert np.array_equal(r64.iK, np.swapaxes(r64.iK, 1, 2))
