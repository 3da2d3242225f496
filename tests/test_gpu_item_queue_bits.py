"""Tier 2 (GPU): the work queue of the fused-horizon kernel's pairwise phase keeps its bits.

tests/golden/item_queue_bits.npz holds mu, Sig and J of every run in tests/item_queue_cases.py::RUNS as the build BEFORE the
per-entry descriptors and the claim-ahead pull computed them (tools/gen_item_queue_golden.py; the fixture names that build).  How
a wavefront learns which item is its next one changes which wavefront evaluates an item and when, never an item's arithmetic, the
slot its result is stored in or the order of a sum, so the comparison is array_equal on the 64-bit patterns: four wavefronts
against 9 to 48 entries (list lengths 0, 1 and 2 modulo 4), eight and sixteen against 48, steps whose pairs are walked in 2, 3 and
6 groups (the queue starts again per group), the three evaluation paths, the time index as an input, and one cooperative run."""
import numpy as np
import pytest

from helpers import load
import item_queue_cases as cases

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
    g = load("item_queue_bits")
    assert [tuple(int(v) for v in r) for r in g["runs"]] == cases.RUNS, "fixture and tests/item_queue_cases.py disagree about the runs"
    for (N, D, tm) in cases.CASES:
        assert float(g[f"actions_sum_N{N}_D{D}_tm{tm}"]) == float(cases.make_case(N, D, tm).actions.sum()), (N, D, tm, "another synthetic workload")
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
    plain = results[cases.run_key((130, 3, cases.B, 0, 1024, 16, 1, 0, 0, 1))]
    coop = results[cases.run_key((130, 3, 1, 0, 0, 16, 2, 0, 0, 1))]
    for name in ("mu", "Sig", "J"):
        assert np.array_equal(_bits(coop[name]), _bits(plain[name][:1])), name
