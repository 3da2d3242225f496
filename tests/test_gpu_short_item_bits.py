"""Tier 2 (GPU): the short items of the fused-horizon kernel's pairwise work queue keep their bits.

tests/golden/short_item_bits.npz holds mu, Sig and J of every run in tests/short_item_cases.py::RUNS as the build BEFORE the
LDS-typed, scalar-argument separable items (sep3_item) and the one-pass mean sums computed them (tools/gen_short_item_golden.py; the fixture names that build).  How an item addresses its operands, in which
registers its arguments travel, where its scatter index comes from and when the wavefront claims its next entry change no
floating-point operation and no order of a sum, so the comparison is array_equal on the 64-bit patterns: N = 33, 64, 65 and 130
(a partial point trip, exactly one, one lane in a second, three), sep3_item<3 ... 6> (tests/test_short_item_cases.py shows which
run meets which), four and sixteen wavefronts, steps in 3 and 6 pair groups, X^T in LDS and in global memory, the time index as an
input, and one cooperative run."""
import numpy as np
import pytest

from helpers import load
import short_item_cases as cases

pytestmark = pytest.mark.gpu


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
    g = load("short_item_bits")
    assert [tuple(int(v) for v in r) for r in g["runs"]] == cases.RUNS, "fixture and tests/short_item_cases.py disagree about the runs"
    for case in cases.CASES:
        assert float(g["actions_sum_N%d_tm%d_s%d" % case]) == float(cases.make_case(*case).actions.sum()), (case, "another synthetic workload")
    return g


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("run", cases.RUNS, ids=cases.run_key)
def test_bits_pinned(results, golden, run):
    key = cases.run_key(run)
    for name in ("mu", "Sig", "J"):
        got, want = results[key][name], golden[f"{name}/{key}"]
        assert np.all(np.isfinite(got)), (key, name)
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (
            key, name, float(np.max(np.abs(got - want))))


def test_cooperative_form_equals_the_plain_kernel(results):
    """At equal chunk length the cooperative form's candidate is the plain kernel's first candidate, bit for bit."""
    plain = results[cases.run_key((130, cases.B, 1024, 16, 1, 0, 0, 1, 1))]
    coop = results[cases.run_key((130, 1, 0, 16, 2, 0, 0, 1, 1))]
    for name in ("mu", "Sig", "J"):
        assert np.array_equal(_bits(coop[name]), _bits(plain[name][:1])), name


def test_global_x_equals_lds_x(results):
    """Where X^T is read from changes no bit: all pairs in one group with the LDS copy and without it (90 KiB)."""
    lds = results[cases.run_key((130, cases.B, 256, 0, 1, 0, 0, 0, 1))]
    glb = results[cases.run_key((130, cases.B, 256, 0, 1, 90, 0, 0, 1))]
    for name in ("mu", "Sig", "J"):
        assert np.array_equal(_bits(glb[name]), _bits(lds[name])), name
