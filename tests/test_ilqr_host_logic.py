"""Tier 1 (CPU): the controller's host logic of candidate_optimizer = "ilqr_device" against a CPU stand-in engine
(tests/ilqr_stub_engine.py): the routing, the starts, the counters and caches, and the refusals."""
import os
import re

import numpy as np
import pytest

from helpers import make_controller
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_and_bound():
    from gp_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    for name in ("gpmpc_ilqr_backward", "gpmpc_ilqr_forward", "gpmpc_ilqr_init", "gpmpc_ilqr_step", "gpmpc_ilqr_search"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and name in _lib.SIGNATURES, name
    assert re.search(r"\blong long\s+gpmpc_ilqr_state_size\s*\(", header) and "gpmpc_ilqr_state_size" in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 26
    from gp_mpc_amd.config_classes import ControllerConfig
    cc = ControllerConfig(candidate_optimizer="ilqr_device")
    assert (cc.ilqr_candidates, cc.ilqr_iterations, cc.ilqr_reg, cc.ilqr_line_search_steps) == (None, 8, 1e-3, 8)


def test_state_size_needs_no_gpu():
    from gp_mpc_amd import _lib
    lib = _lib.lib()
    B, H, A, D, L = 5, 3, 2, 4, 8
    assert lib.gpmpc_ilqr_state_size(B, H, A, D, L) == B * (H * A * (2 + D + L) + 9 + L + (H + 1) * D)
    for bad in ((0, H, A, D, L), (4097, H, A, D, L), (B, 0, A, D, L), (B, H, 0, D, L), (B, H, 9, D, L), (B, H, A, 0, L),
                (B, H, A, 17, L), (B, H, A, D, 0), (B, H, A, D, 17)):
        assert lib.gpmpc_ilqr_state_size(*bad) < 0, bad


def _ilqr_controller(w, eng, deriv=False, propagation="linearized", starts=3, iterations=2):
    c = make_controller(w, limit_action_change=deriv, optimize=True, restarts=starts, engine=eng, shard=False)
    cc = c.config.controller
    cc.candidate_optimizer, cc.ilqr_iterations, cc.ilqr_line_search_steps, cc.ilqr_reg = "ilqr_device", iterations, 3, 1e-2
    c.transition_model.config.uncertainty_propagation = propagation
    return c


def test_ilqr_device_behind_get_action():
    from ilqr_stub_engine import IlqrOracleEngine
    from gp_mpc_amd.control_objects.actions_mappers.action_init_functions import (generate_mpc_action_init_random,
                                                                                   generate_mpc_action_init_frompreviousiter)
    w = synth.make_workload(16, 2, 1, 3, 1, seed=41)
    N, D, A, E, H, B = w.dims
    eng = IlqrOracleEngine()
    c = _ilqr_controller(w, eng)
    np.random.seed(7)
    a = c.get_action(w.mu0, w.S0)
    assert a.shape == (A,) and np.all(np.isfinite(a)) and np.all((a >= 0) & (a <= 1))
    call = eng.ilqr_calls[-1]
    assert call["iterations"] == 2 and call["line_search_steps"] == 3 and call["reg0"] == 1e-2 and call["x0"].shape == (3, H * A)
    assert call["include_time"] == w.include_time and call["time0"] == 0.0
    assert "rollout_linear" in eng.calls and "rollout" not in eng.calls
    # the starts are those "lbfgs_device" draws under the same seed
    np.random.seed(7)
    want = np.stack([generate_mpc_action_init_random(len_horizon=H, dim_action=A) for _ in range(3)]).reshape(3, H * A)
    assert np.array_equal(call["x0"], want) and np.array_equal(c.ilqr_device_starts, want)
    # counters and caches
    assert c.num_rollouts == 3 * 2 * (1 + 3) + 1 and c.ilqr_iterations_run == 2
    assert c.candidates_final_J.shape == (3,) and c.candidates_final_status.shape == (3,)
    assert c.best_candidate_J == np.min(c.candidates_final_J) and c.best_candidate_index == int(np.argmin(c.candidates_final_J))
    assert abs(c.cost_traj_mean_lcb.item() + c.best_candidate_J) <= 1e-9 * abs(c.best_candidate_J)
    assert c.states_mu_pred.shape == (H + 1, D)
    # the next step warm-starts: slot 0 is the shifted previous solution
    best = c.actions_mpc_previous_iter.copy()
    c.get_action(w.mu0, w.S0)
    shifted = np.asarray(generate_mpc_action_init_frompreviousiter(best, dim_action=A)).reshape(-1)
    assert np.array_equal(eng.ilqr_calls[-1]["x0"][0], shifted) and eng.ilqr_calls[-1]["time0"] == 1.0
    # ilqr_candidates overrides restarts_optim
    c.config.controller.ilqr_candidates = 5
    c.get_action(w.mu0, w.S0)
    assert eng.ilqr_calls[-1]["x0"].shape == (5, H * A)


def test_refusals():
    from ilqr_stub_engine import IlqrOracleEngine
    w = synth.make_workload(16, 2, 1, 3, 1, seed=41)
    # moment matching: the iLQR exists under the linearised propagation only
    eng = IlqrOracleEngine()
    c = _ilqr_controller(w, eng, propagation="moment_matching")
    with pytest.raises(ValueError, match="linearized"):
        c.get_action(w.mu0, w.S0)
    # closed-loop planning
    for gain in (np.zeros((1, 2)), "lqr"):
        c = _ilqr_controller(w, eng)
        c.config.controller.feedback_gain = gain
        with pytest.raises(ValueError, match="feedback_gain"):
            c.get_action(w.mu0, w.S0)
    # the derivative mapper
    c = _ilqr_controller(w, eng, deriv=True)
    with pytest.raises(ValueError, match="DerivativeActionMapper"):
        c.get_action(w.mu0, w.S0)
    # sharded starts: refused before the engine (or any collective) is touched
    c = _ilqr_controller(w, eng)
    c._ranks = lambda: (2, 1)
    with pytest.raises(ValueError, match="shard"):
        c.get_action(w.mu0, w.S0)
    assert not eng.ilqr_calls and eng.launches == 0
    # the other optimisers stay refused under the linearised propagation, and the message names what is supported
    c = make_controller(w, optimize=True, engine=IlqrOracleEngine(), shard=False)
    c.transition_model.config.uncertainty_propagation = "linearized"
    with pytest.raises(ValueError, match="ilqr_device"):
        c.get_action(w.mu0, w.S0)
    # optimize=False never reaches the iLQR and is not refused for naming it
    c = _ilqr_controller(w, IlqrOracleEngine(), propagation="moment_matching")
    c.config.controller.optimize = False
    assert np.all(np.isfinite(c.get_action(w.mu0, w.S0)))
