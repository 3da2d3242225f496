"""Tier 1 (CPU): the numpy restatement of greedy variance selection (tests/select_inducing_ref.py) that the GPU tests of
gpmpc_select_inducing are measured against -- what it computes (the trace term of the Titsias bound of the chosen rows), and the
condition under which an index sequence can be compared at all: the float64 and the longdouble runs pick the same points and no
choice is closer than 1e-9 (relative) to its runner-up.  float64 scores carry errors near 1e-13, so 1e-9 leaves four orders of
margin; measured smallest gaps: 7.8e-6 (d1), 2.8e-5 (floor_0.05), >= 1e-4 for every other case."""
import numpy as np
import pytest

import select_inducing_ref as ref
import sparse_gp_ref as sgr

GAP_MIN = 1e-9


@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_trace_never_increases_and_indices_are_distinct(name):
    c = ref.case(name)
    for run in (c.ld, c.f64):
        assert run["idx"][0] == 0 and len(set(run["idx"].tolist())) == c.M
        assert np.all(np.isfinite(run["trace"].astype(np.float64)))
        assert np.all(np.diff(run["trace"]) <= 0)


@pytest.mark.parametrize("name", [n for n in ref.INDEX_CASES])
def test_trace_is_the_titsias_trace_term_of_the_chosen_rows(name):
    """trace[m] = sum_a (N sigma2_a - tr(Kfu Kuu^-1 Kuf)) / sigma2_a of the first m + 1 picks, by a dense solve, for as long as no
    pivot met the floor (afterwards the partial factors deliberately skip a pick)."""
    c = ref.case(name)
    clean = np.flatnonzero(~np.any(c.ld["floored"], axis=1))
    upto = c.M if len(clean) == c.M else int(np.flatnonzero(np.any(c.ld["floored"], axis=1))[0])
    checked = 0
    for m in sorted({0, upto // 2, upto - 1} & set(range(upto))):
        want = ref.dense_trace(c.X, c.ld["idx"][:m + 1], c.ls, c.os)
        scale = float(c.ld["trace"][0]) + 1.0
        # a dense longdouble solve on rows chosen for being independent: its own error is far below this
        assert abs(float(c.ld["trace"][m] - want)) <= 1e-9 * scale, (name, m)
        checked += 1
    assert checked >= 1 or upto == 0


def test_m_equal_n_returns_a_permutation():
    c = ref.case("n64_m64")
    assert sorted(c.ld["idx"].tolist()) == list(range(64)) and sorted(c.f64["idx"].tolist()) == list(range(64))
    one = ref.case("n1_m1")
    assert one.ld["idx"].tolist() == [0] and float(one.ld["trace"][0]) == 0.0


@pytest.mark.parametrize("name", ref.INDEX_CASES)
def test_the_condition_the_gpu_index_test_relies_on(name):
    """A cap, not a tolerance: no step is skipped (step 0 is a D-way tie by construction; at M = N the last step has no runner-up)."""
    c = ref.case(name)
    assert np.array_equal(c.ld["idx"], c.f64["idx"])
    last = c.M - 1 if c.M == c.N else c.M
    gaps = c.ld["gap"][1:last]
    print(f"{name}: smallest gap {np.min(gaps) if len(gaps) else float('nan'):.3e}, float64 trace error {c.e64_trace:.3e}")
    assert np.all(gaps >= GAP_MIN), (name, float(np.min(gaps)))
    assert np.array_equal(np.isnan(c.ld["gap"]), np.arange(c.M) >= (c.N - 1))      # a gap wherever there is a runner-up


def test_duplicated_rows_pick_the_distinct_rows_first():
    c = ref.case("dups")
    alone = ref.select(c.X[:20], 20, c.ls, c.os, c.jitter_rel, ref.LD)
    for run in (c.ld, c.f64):
        assert np.array_equal(run["idx"][:20], alone["idx"]) and len(set(run["idx"].tolist())) == 40
        assert np.all(np.abs(run["trace"][19:].astype(np.float64)) <= c.tol_trace)


def test_floor_cases_meet_the_floor():
    for name in ("floor_0.05", "floor_0.3"):
        c = ref.case(name)
        assert c.ld["floored"].any() and np.array_equal(c.ld["floored"], c.f64["floored"])
    assert not ref.case("n257_m70").ld["floored"].any()


def test_greedy_beats_strided_on_a_clustered_memory():
    """clustered_n600_m40: 540 rows in a tight cluster and 60 exploratory ones.  Measured: trace 5.16 against 23.1 for the strided
    rows, rms error of the sparse mean against the exact GP at 200 uniform queries 0.086 against 0.118."""
    c = ref.case("clustered_n600_m40")
    strided = sgr.strided_rows(c.N, c.M)
    t_greedy, t_strided = float(c.ld["trace"][-1]), float(ref.dense_trace(c.X, strided, c.ls, c.os))
    exact = ref.exact_mean(c.X, c.Y, c.ls, c.os, c.nz, c.Xq)
    rms = {k: float(np.sqrt(np.mean((ref.sparse_mean(c.X, c.Y, c.X[rows], c.ls, c.os, c.nz, c.Xq) - exact) ** 2)))
           for k, rows in (("greedy", c.f64["idx"]), ("strided", strided))}
    print(f"trace greedy {t_greedy:.3f} strided {t_strided:.3f}; rms greedy {rms['greedy']:.4f} strided {rms['strided']:.4f}")
    assert t_greedy < t_strided
    assert rms["greedy"] < rms["strided"]
