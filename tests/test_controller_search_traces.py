"""GpMpcController's candidate searches against a recording stand-in engine (no GPU): every search makes exactly the engine
and model calls, takes exactly the draws from numpy's global generator, returns the action and leaves the attributes that
tests/golden/controller_search_traces.json says.  The cases and the recorder are tests/controller_search_cases.py; the fixture
was written by tools/gen_controller_search_golden.py from the controller that still held the seven searches inline.
The refused combinations and their messages are spelled out here, so that a regenerated fixture cannot move them."""
import json
import os
import re

import numpy as np
import pytest

import controller_search_cases as cases

_SUPPORTED = ("optimize=False (random shooting), candidate_optimizer='cem' or, in open loop, candidate_optimizer='lbfgs_device' "
              "or candidate_optimizer='ilqr_device'")
_NO_LINEARIZED = ("uncertainty_propagation='linearized' does not support {}: it has no gradient or device-search kernels; "
                  "supported optimisers: " + _SUPPORTED)
_GAIN = np.zeros((cases.A, cases.D))
# (optimizer, derivative mapper, propagation, feedback_gain) -> the ValueError's text
REFUSED = [
    (("ilqr_device", False, "moment_matching", None),
     "candidate_optimizer='ilqr_device' needs ModelConfig.uncertainty_propagation='linearized': the iLQR runs on the mean "
     "dynamics of the linearised propagation, moment matching has none"),
    (("ilqr_device", False, "linearized", _GAIN),
     "candidate_optimizer='ilqr_device' plans in open loop: it does not support ControllerConfig.feedback_gain"),
    (("ilqr_device", False, "linearized", "lqr"),
     "candidate_optimizer='ilqr_device' plans in open loop: it does not support ControllerConfig.feedback_gain"),
    (("ilqr_device", True, "linearized", None),
     "candidate_optimizer='ilqr_device' optimises the model actions themselves: it needs the normalisation action mapper, not "
     "the DerivativeActionMapper"),
    (("lbfgs_device", False, "linearized", _GAIN),
     "candidate_optimizer='lbfgs_device' searches the open-loop objective: it does not support ControllerConfig.feedback_gain"),
    ((False, False, "moment_matching", _GAIN),
     "ControllerConfig.feedback_gain needs ModelConfig.uncertainty_propagation='linearized': moment matching has no closed-loop "
     "rollout"),
    (("lbfgs_device", False, "moment_matching", _GAIN),
     "ControllerConfig.feedback_gain needs ModelConfig.uncertainty_propagation='linearized': moment matching has no closed-loop "
     "rollout"),
    ((None, False, "linearized", None), _NO_LINEARIZED.format("candidate_optimizer=None with optimize=True")),
    (("lbfgs", False, "linearized", None), _NO_LINEARIZED.format("candidate_optimizer='lbfgs' with optimize=True")),
    (("cem_device", True, "linearized", None), _NO_LINEARIZED.format("candidate_optimizer='cem_device' with optimize=True")),
    (("cem_device", False, "linearized", _GAIN), _NO_LINEARIZED.format("candidate_optimizer='cem_device' with optimize=True")),
]
ALLOWED = [(False, False, "linearized", None), (False, True, "linearized", _GAIN), ("cem", False, "linearized", "lqr"),
           ("lbfgs_device", True, "linearized", None), ("ilqr_device", False, "linearized", None)]
# the gradient-path entry points under the linearised propagation, whatever the search
GRADIENT_PATH = [("compute_mean_lcb_trajectory", _NO_LINEARIZED.format("compute_mean_lcb_trajectory (the gradient path)")),
                 ("objective_and_gradient_batch", _NO_LINEARIZED.format("objective_and_gradient_batch (the gradient path)"))]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "controller_search_traces.json")) as fh:
        return json.load(fh)


def test_fixture_covers_the_cases(golden):
    assert list(golden) == cases.IDS and len(cases.IDS) == 26
    for cid, rec in golden.items():
        assert sorted(rec) == ["action", "attributes", "calls", "next_draw"], cid
        assert rec["calls"][0]["call"] == "model.prepare_inference", cid
        assert set(cases.CACHES) < set(rec["attributes"]) and "actions_mpc_previous_iter" in rec["attributes"], cid


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_search_trace(case, golden):
    rec = json.loads(json.dumps(cases.run_case(case)))   # (tuples -> lists, as the fixture went through)
    want = golden[case[0]]
    assert [c["call"] for c in rec["calls"]] == [c["call"] for c in want["calls"]]
    cases.assert_same(rec, want)


def _rebuilt(opt, deriv, propagation, gain):
    """A controller constructed on the finished config: the support check of __init__ sees it."""
    c, w = cases.controller(opt, deriv, cases.ExactEngine(), feedback_gain=gain, propagation=propagation)
    z, o = np.zeros, np.ones
    return lambda: type(c)(z(cases.D), o(cases.D), z(cases.A), o(cases.A), c.config, engine=cases.ExactEngine()), c, w


@pytest.mark.parametrize("config,message", REFUSED, ids=[f"{c[0]}-{c[2]}-{i}" for i, (c, _) in enumerate(REFUSED)])
def test_refused_combinations(config, message):
    build, c, w = _rebuilt(*config)
    with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
        build()
    eng = c.transition_model.engine
    with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
        c._get_optimal_actions(w.mu0, w.S0)
    assert eng.calls == []                               # refused before the memory is prepared


@pytest.mark.parametrize("config", ALLOWED, ids=[f"{c[0]}-{i}" for i, c in enumerate(ALLOWED)])
def test_allowed_combinations_under_the_linearised_propagation(config):
    build, _, _ = _rebuilt(*config)
    build()._check_propagation_supported()


@pytest.mark.parametrize("opt", [False, "cem", "lbfgs_device", "ilqr_device"])
@pytest.mark.parametrize("method,message", GRADIENT_PATH)
def test_gradient_path_entry_points_are_refused_under_the_linearised_propagation(opt, method, message):
    c, w = cases.controller(opt, False, cases.ExactEngine(), propagation="linearized")
    x = np.full((1, cases.H * cases.A), 0.5)
    with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
        getattr(c, method)(x if method == "objective_and_gradient_batch" else x[0], w.mu0, w.S0)
    assert c.LINEARIZED_OPTIMIZERS == _SUPPORTED
