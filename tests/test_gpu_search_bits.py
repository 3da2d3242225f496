"""Tier 2 (GPU): the device-resident searches keep their bits.

tests/golden/search_bits.npz holds every result of tests/search_bits_cases.py::run_all as the build of commit d975212 computed it
(tools/gen_search_bits_golden.py) -- the last build with two copies of the bitonic sort, of the refit and of the action mapper.
Sharing that code (csrc/action_mapper.h, cem_sort / cem_load_keys / cem_refit of csrc/search.hip, finite_d / clip01 of
csrc/device_common.h, rollout_objective_only) moves text, never an element's arithmetic or the order of a sum, so the comparison
is array_equal on the 64-bit patterns:
  cem_search     B = 2 / 65 / 2049 x n_elite = 1 / 9 / B, both mappers, with and without a warm start: best | best J
  cem_shard      cem_local on two slices and an empty one + cem_merge, 3 iterations: every slice's records and mean | std |
                 best | best J after each -- the only place the refit's mean and std are observed directly
  lbfgs_search   n = 6 and n = 65, both mappers, both propagations, a wrapping pair ring: the state buffer and the winner
  train_search   2 restarts: the state buffer and the winner records
  ilqr_search    the state buffer and the winner"""
import numpy as np
import pytest

from helpers import load
import search_bits_cases as cases

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
    g = load("search_bits")
    assert [str(k) for k in g["keys"]] == cases.KEYS, "fixture and tests/search_bits_cases.py disagree about the runs"
    for (A, H) in cases.MODELS:
        assert float(g[f"actions_sum_A{A}_H{H}"]) == float(cases.make_case(A, H).actions.sum()), (A, H, "another synthetic workload")
    return g


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("key", cases.KEYS)
def test_bits_pinned(results, golden, key):
    names = sorted(results[key])
    assert names == sorted(k[len(key) + 1:] for k in golden if k.startswith(key + "/")), key
    for name in names:
        got, want = results[key][name], golden[f"{key}/{name}"]
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (
            key, name, int(np.count_nonzero(_bits(got) != _bits(want))), float(np.nanmax(np.abs(got - want))))
