"""Tier 2 (GPU): the rank-one recurrence of a sparse model (csrc/sparse_update.hip: gpmpc_sparse_append and gpmpc_sparse_forget as
two instantiations of one pair of kernels) keeps its bits.

tests/golden/sparse_update_bits.npz holds beta_eff, predict's mean and variance and the SHA-256 of iK_eff of every run in
tests/sparse_update_cases.py::RUNS as the build computed them that still had the two calls as two copies of the kernels, plans and
driver (tools/gen_sparse_update_golden.py, on an MI355X).  Merging them moves vectors between buffers and chooses a sign at compile
time, never an element's arithmetic or the order of a sum, so the comparison is array_equal on the 64-bit patterns: M = 1 (16 row
groups of one row), one, two and three column tiles with a partial last one, D = 1 and D = 16 (every failure word in use) with
E = 20, 64 points in one call, appends and forgets alternating on one handle (a vector the other call left in the shared scratch
block would show), the lost pivot's code and text and the handle's recovery from it, M = 961 (one row group: the other branch of
the group rule) and M = 1700 (more than 64 KiB of LDS: the raised limit of both instantiations)."""
import numpy as np
import pytest

from helpers import load
import sparse_update_cases as cases

pytestmark = pytest.mark.gpu

LOST_PIVOT_TEXT = ("sparse_forget: point 0 of the call, output 0: the pivot is lost (the point is not in the model, or too little of the "
                   "model would remain)")


@pytest.fixture(scope="module")
def results():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    try:
        return cases.run_all(eng)            # computed once, shared by the tests below, never modified
    finally:
        eng.close()


@pytest.fixture(scope="module")
def golden():
    g = load("sparse_update_bits")
    assert [str(r) for r in g["runs"]] == cases.RUNS, "fixture and tests/sparse_update_cases.py disagree about the runs"
    for name in cases.LARGE:
        assert float(g[f"X_sum/{name}"]) == float(cases.large_case(name).X.sum()), (name, "another synthetic memory")
    return g


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("run", cases.RUNS)
def test_bits_pinned(results, golden, run):
    for name in ("beta", "mean", "var"):
        got, want = results[run][name], golden[f"{name}/{run}"]
        assert np.all(np.isfinite(got)), (run, name)
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (run, name, float(np.max(np.abs(got - want))))
    assert str(results[run]["iK_sha256"]) == str(golden[f"iK_sha256/{run}"]), run


def test_lost_pivot_code_text_and_recovery(results, golden):
    from gp_mpc_amd import _lib
    got = results["lost_pivot"]
    assert int(got["code"]) == int(golden["code/lost_pivot"]) == _lib.GPMPC_ERR_NOT_PD
    assert str(got["message"]) == str(golden["message/lost_pivot"])
    assert str(got["message"]).endswith(LOST_PIVOT_TEXT)
    for name in ("beta", "mean", "var"):                  # prepare_sparse + the forget of m1-1 on the handle that lost the pivot
        assert np.array_equal(_bits(got[name]), _bits(golden[f"{name}/forget/m1-1"])), name
    assert str(got["iK_sha256"]) == str(golden["iK_sha256/forget/m1-1"])
