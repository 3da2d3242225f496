"""Tier 2 (GPU): the serial chain of a horizon step of the fused-horizon kernel (csrc/rollout_kernel.h: pair totals, M and V,
state update, trajectory store, the next step's small D x D algebra) keeps its bits.

tests/golden/step_chain_bits.npz holds mu, Sig and J of every run in tests/step_chain_cases.py::RUNS as the kernel computed
them BEFORE the state update and the next step's small algebra were merged onto one wavefront with no workgroup barrier between
them (tools/gen_step_chain_golden.py).  The merge moves work between wavefronts and barriers, never an operation or the order of
a sum, so the comparison is array_equal on the
64-bit patterns: horizons of 1, 2 and 5 steps (first algebra + last tail only, one merged trip, several), D = 1-4 and 6, fewer
points than a wavefront, every workgroup width, the time input, several pair groups per step, separable and element-wise totals,
the cooperative form and the per-candidate kernel of the batch-major path."""
import numpy as np
import pytest

from helpers import load
import step_chain_cases as cases

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
    g = load("step_chain_bits")
    assert [tuple(int(v) for v in r) for r in g["runs"]] == cases.RUNS, "fixture and tests/step_chain_cases.py disagree about the runs"
    for case in cases.CASES:
        assert float(g["actions_sum_N%d_D%d_H%d_tm%d" % case]) == float(cases.make_case(*case).actions.sum()), (case, "another synthetic workload")
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


@pytest.mark.parametrize("run", cases.MULTI_GROUP_RUNS, ids=cases.run_key)
def test_small_lds_limit_walks_several_pair_groups(results, run):
    """The runs meant to take the loop over pair groups did take it."""
    assert results[cases.run_key(run)]["groups"] > 1, (run, results[cases.run_key(run)]["groups"])


@pytest.mark.parametrize("coop,plain", cases.COOP_PAIRS, ids=lambda r: cases.run_key(r))
def test_cooperative_form_equals_the_plain_kernel(results, coop, plain):
    """At equal chunk length the cooperative form's candidate is the plain kernel's first candidate, bit for bit (as
    tests/test_gpu_cluster.py asserts over its own shapes), at one and two horizon steps."""
    c, p = results[cases.run_key(coop)], results[cases.run_key(plain)]
    for name in ("mu", "Sig", "J"):
        assert np.array_equal(_bits(c[name]), _bits(p[name][:1])), (coop, name)
