"""engine.py against a recording stand-in for the library (no GPU): every call family hands the C ABI exactly what
tests/golden/engine_calls.json says -- function, integers and floats by value, pointers by role -- returns the same keys,
shapes and dtypes, and raises the same ValueErrors.  The cases and the recorder are tests/engine_call_cases.py; the fixture
was written by tools/gen_engine_calls_golden.py from the engine.py that had one wrapper body per entry point."""
import json
import os

import pytest

import engine_call_cases as cases

# the text of every ValueError path (the fixture holds the same; spelled out here so that a regenerated fixture cannot move them)
_GAINS = "feedback gains must have shape (A, D) = (1, 2), (H, A, D) = (3, 1, 2) or (B, H, A, D) = (2, 3, 1, 2), got (3, 2, 1)"
_UNPACK = "not enough values to unpack (expected 3, got 2)"
_OUT = "`out` does not match the batch shape"
_ROLLOUTS = ("rollout", "rollout_linear", "rollout_linear_feedback")
_BACKWARDS = ("rollout_backward", "rollout_linear_backward", "rollout_linear_feedback_backward")
RAISES = {
    "predict-rank": "expected query inputs of shape (M, E), got (3,)",
    "predict-bad_noises": "expected shape (2,), got (3,)",
    "predict_backward-rank": "expected query inputs of shape (M, E), got (3,)",
    "predict_backward-bad_mean_bar": "expected shape (3, 2), got (4, 2)",
    "predict_backward-bad_var_bar": "expected shape (3, 2), got (4, 2)",
    "predict_cov-rank": "expected query inputs of shape (Ma, E), got (3,)",
    "predict_cov-Xb_rank": "expected query inputs of shape (Mb, 3), got (3,)",
    "predict_cov-Xb_wrongE": "expected query inputs of shape (Mb, 3), got (2, 4)",
    "predict_cov-bad_noises": "expected shape (2,), got (3,)",
    "rollout_linear_feedback-bad_gains": _GAINS,
    "rollout_linear_feedback_backward-bad_gains": _GAINS,
}
for _m in ("moments", "moments_linear", "moments_backward", "moments_linear_backward"):
    RAISES[f"{_m}-rank"] = "expected input means of shape (P, E), got (3,)"
    RAISES[f"{_m}-bad_var"] = "expected shape (3, 3, 3), got (3, 3)"
for _m in ("moments_backward", "moments_linear_backward"):
    RAISES[f"{_m}-bad_M_bar"] = "expected shape (3, 2), got (4, 2)"
    RAISES[f"{_m}-bad_S_bar"] = "expected shape (3, 2, 2), got (3, 2)"
    RAISES[f"{_m}-bad_V_bar"] = "expected shape (3, 3, 2), got (3, 2, 3)"
for _m in _ROLLOUTS + _BACKWARDS:
    RAISES[f"{_m}-actions_rank"] = _UNPACK
    RAISES[f"{_m}-bad_mu0"] = "expected shape (2,), got (3,)"
    RAISES[f"{_m}-bad_S0"] = "expected shape (2, 2), got (2, 3)"
for _m in _ROLLOUTS:
    RAISES[f"{_m}-out_bad_J"] = _OUT
    RAISES[f"{_m}-out_bad_mu"] = _OUT
for _m in _BACKWARDS:
    RAISES[f"{_m}-bad_mu_bar"] = "expected shape (2, 4, 2), got (2, 3, 2)"
    RAISES[f"{_m}-bad_Sig_bar"] = "expected shape (2, 4, 2, 2), got (2, 4, 2)"
    RAISES[f"{_m}-bad_cost_mu_bar"] = "expected shape (2, 4), got (2, 3)"
    RAISES[f"{_m}-bad_cost_var_bar"] = "expected shape (2, 4), got (2, 3)"
    RAISES[f"{_m}-bad_J_bar"] = "expected shape (2,), got (3,)"


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "engine_calls.json")) as fh:
        return json.load(fh)


def test_fixture_covers_the_cases(golden):
    assert sorted(golden) == sorted(cases.IDS)
    assert {cid for cid, rec in golden.items() if "raises" in rec} == set(RAISES)
    for cid, text in RAISES.items():
        assert golden[cid]["raises"] == text, cid
        assert golden[cid]["calls"] == [], cid           # a rejected call never reaches the library
    # the three arities the families end in
    assert len(golden["rollout-E3"]["calls"][0]["args"]) + 1 == 15
    assert len(golden["rollout_linear_feedback_backward-E3"]["calls"][0]["args"]) + 1 == 21
    assert len(golden["moments_backward-E3"]["calls"][0]["args"]) + 1 == 12
    assert '"?"' not in json.dumps(golden)               # every pointer's role is named


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_engine_call(case, golden):
    rec = json.loads(json.dumps(cases.run_case(case)))   # (tuples -> lists, as the fixture went through)
    if case[0] in RAISES:
        assert rec.get("raises") == RAISES[case[0]]
    assert rec == golden[case[0]]
