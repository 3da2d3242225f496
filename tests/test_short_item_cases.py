"""Tier 1 (CPU, no GPU): the runs of tests/short_item_cases.py reach the code they are there for.

Restating the kernel's degree selection on the numpy oracle's trajectory (tests/hetero_cases.taylor_degrees, as
tests/test_hetero_reference.py does): with force_separable every off-diagonal pair of degree 1 ... 6 is a separable pair evaluated
by sep3_item<max(3, degree)>.  Every instantiation 3, 4, 5 and 6 has to be met in some step of some run, every run has to hold
separable pairs in every step of some candidate, and the runs have to span the N, widths, groups and forms their docstring names."""
import os
import re

import numpy as np

import short_item_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "data-efficient-reinforcement-learning-with-probabilistic-model-predictive-control_amd"


def _taylor_max_arg():
    src = open(os.path.join(ROOT, PKG, "csrc", "rollout_kernel.h")).read()
    m = re.search(r"kTaylorMaxArg\[kMaxTaylor \+ 1\] = \{([^}]*)\}", src)
    return [float(x) for x in m.group(1).replace("\n", " ").split(",")]


def test_every_sep3_instantiation_is_met():
    tab = _taylor_max_arg()
    assert len(tab) == 15
    met = {3: [], 4: [], 5: [], 6: []}
    for case in cases.CASES:
        deg = cases.degrees_of(case, tab)                    # (B, H, 3 off-diagonal pairs)
        nB = max(r[1] for r in cases.RUNS if (r[0], r[6], r[7]) == case)
        nB_min = min(r[1] for r in cases.RUNS if (r[0], r[6], r[7]) == case)
        sep = (deg >= 1) & (deg <= 6)
        ks = np.where(sep, np.maximum(deg, 3), 0)
        print(case, "KS per (candidate, step, pair):", ks[:nB].tolist())
        # the first candidate (the only one of a one-candidate run) has a separable pair in every step
        assert np.all(sep[:nB_min].any(axis=2)), (case, deg[:nB_min].tolist())
        for k in met:
            if np.any(ks[:nB] == k):
                met[k].append(case)
    for k, v in met.items():
        print("sep3_item<%d>: %d cases, first %s" % (k, len(v), v[:1]))
        assert v, k
    # every N meets a low (3) and a high (>= 5) instantiation, so each point-trip corner runs short and long bands
    for N in (33, 64, 65, 130):
        lo = [c for c in met[3] if c[0] == N]
        hi = [c for c in met[5] + met[6] if c[0] == N]
        assert lo and hi, (N, lo, hi)


def test_runs_span_their_corners():
    runs = cases.RUNS
    assert len(set(runs)) == len(runs)
    assert {r[0] for r in runs} == {33, 64, 65, 130}
    for N in (33, 64, 65, 130):
        assert {r[2] for r in runs if r[0] == N} >= {256, 1024}, N
    assert {r[8] for r in runs} >= {1, 3, 6}                              # pair groups
    assert any(r[6] == 1 for r in runs)                                   # the time index
    assert any(r[4] == 2 and r[1] == 1 for r in runs)                     # the cooperative form, one candidate
    assert any(r[5] > 0 and r[8] == 1 for r in runs)                      # X^T in global memory with all pairs in one group
    assert all(r[1] <= 8 for r in runs) and cases.H == 3 and cases.D == 3
