"""Tier 2 (GPU): the element loops of the fused-horizon kernel's pairwise items (item_taylor2 / item_exp2 of
csrc/rollout_kernel.h) keep their bits.

tests/golden/item_loop_bits.npz holds mu, Sig and J of every run in tests/item_loop_cases.py::RUNS as the build BEFORE the scalar
row addressing and the pinned T prefetch computed them (tools/gen_item_loop_golden.py).  Those changes move addresses and loads,
never an element's arithmetic or the order of a sum, so the comparison is array_equal on the 64-bit patterns: odd N (rows that
are not 16-byte aligned, the masked second column), one and two column units, 1- and 2-row last chunks, the prefetch running
into the zero rows behind the last output, two and four rows per trip, the Taylor loop's diagonal and off-diagonal branches,
the direct-exp loop, every workgroup width, short chunks and the cooperative form."""
import numpy as np
import pytest

from helpers import load
import item_loop_cases as cases

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
    g = load("item_loop_bits")
    assert [tuple(int(v) for v in r) for r in g["runs"]] == cases.RUNS, "fixture and tests/item_loop_cases.py disagree about the runs"
    for (N, D) in cases.SHAPES:
        assert float(g[f"actions_sum_N{N}_D{D}"]) == float(cases.make_case(N, D).actions.sum()), (N, D, "another synthetic workload")
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


@pytest.mark.parametrize("cs", [2, 9])
def test_cooperative_form_equals_the_plain_kernel(results, cs):
    """At equal chunk length the cooperative form's candidate is the plain kernel's first candidate, bit for bit (as
    tests/test_gpu_cluster.py asserts over its own shapes)."""
    plain = results[cases.run_key((130, 3, cases.B, 0, 0, 16, 1))]
    coop = results[cases.run_key((130, 3, 1, 0, 0, 16, cs))]
    for name in ("mu", "Sig", "J"):
        assert np.array_equal(_bits(coop[name]), _bits(plain[name][:1])), (cs, name)
