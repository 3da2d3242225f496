"""Tier 1 (CPU): the device-resident L-BFGS (gpmpc_lbfgs_init / _step / _search) without a GPU -- its numpy restatement
(tests/lbfgs_device_ref.py, the definition the kernels are tested against in tests/test_gpu_lbfgs_device.py) and the controller's
host logic of candidate_optimizer = "lbfgs_device" against a CPU stand-in engine (tests/lbfgs_stub_engine.py).

The convergence test runs on ONE seeded problem (quadratic(25, seed 3), 8 starts of seed 103): there every restart is within
1e-6 of the constrained minimum after 25 evaluations (worst 5e-8).  Other seeds of the same generator were measured too: worst
restarts between 5e-8 and 1e-5 after 25 evaluations -- the bound is a statement about this problem, not about the method.
"""
import os
import re

import numpy as np
import pytest

import lbfgs_device_ref as ref
from helpers import make_controller
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
C1, PGTOL = 1e-4, 1e-5


# -- 0. the interface exists ------------------------------------------------------------------------------------------------------
def test_header_and_bindings_declare_the_entries():
    from gp_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    for name in ("gpmpc_lbfgs_init", "gpmpc_lbfgs_step", "gpmpc_lbfgs_search"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"\blong long\s+gpmpc_lbfgs_state_size\s*\(", header) and "gpmpc_lbfgs_state_size" in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 25
    from gp_mpc_amd.config_classes import ControllerConfig
    cc = ControllerConfig(candidate_optimizer="lbfgs_device")
    assert cc.lbfgs_device_iterations == 30 and cc.lbfgs_device_history == 10 and cc.lbfgs_candidates is None


def test_state_size_needs_no_gpu():
    from gp_mpc_amd import _lib
    lib = _lib.lib()
    B, n, m = 65, 200, 10
    assert lib.gpmpc_lbfgs_state_size(B, n, m) == 5 * B * n + 4 * B + 2 * B * m * n + 2 * B * m
    st = ref.init(np.zeros((B, n)), n, 1, m)
    assert sum(v.size for v in st.values()) == lib.gpmpc_lbfgs_state_size(B, n, m)
    for bad in ((0, n, m), (4097, n, m), (B, 0, m), (B, 4097, m), (B, n, 0), (B, n, 33)):
        assert lib.gpmpc_lbfgs_state_size(*bad) < 0


# -- 1. the box-constrained quadratic ---------------------------------------------------------------------------------------------
def _quad_fun(Q, c):
    def fun(actions):
        B = actions.shape[0]
        vals = [ref.quad_value(Q, c, actions[b].reshape(-1)) for b in range(B)]
        return np.array([v[0] for v in vals]), np.stack([v[1] for v in vals]).reshape(actions.shape)
    return fun


def _constrained_minimum(Q, c):
    from scipy.optimize import minimize
    n = c.size
    runs = [minimize(lambda z: ref.quad_value(Q, c, z), x0=np.random.default_rng(s).uniform(size=n), jac=True, method="L-BFGS-B",
                     bounds=[(0, 1)] * n, options=dict(ftol=1e-16, gtol=1e-12, maxiter=1000, maxfun=10000)) for s in range(3)]
    return min(r.fun for r in runs)


def test_eight_restarts_reach_the_constrained_minimum_within_25_evaluations():
    n = 25
    Q, c = ref.quadratic(n, 3)
    assert np.sum((c < 0.0) | (c > 1.0)) >= 5                    # the unconstrained minimiser is partly outside the box
    J_star = _constrained_minimum(Q, c)
    x0 = np.random.default_rng(103).uniform(size=(8, n))
    trace = []
    st = ref.search(_quad_fun(Q, c), x0, n, 1, 25, 10, C1, 0.0, trace=trace)
    gap = st["J"] - J_star
    print("J* =", J_star, "gaps", gap)
    assert np.all(gap <= 1e-6) and np.all(gap >= -1e-12)
    # J never increases, and x is the point J belongs to
    Js = np.stack([s["J"] for _, s, _ in trace])
    assert np.all(np.diff(Js, axis=0) <= 0.0)
    for b in range(8):
        assert ref.quad_value(Q, c, st["x"][b])[0] == st["J"][b]
    assert np.all((st["x"] >= 0.0) & (st["x"] <= 1.0))
    # both faces of the box hold coordinates at the end
    last = trace[-1][2]
    assert all(i["fixed_lo"] > 0 and i["fixed_hi"] > 0 for i in last if i["branch"] == "accept")
    # the longdouble restatement gets there too
    stl = ref.search(_quad_fun(Q, c), x0, n, 1, 25, 10, C1, 0.0, dtype=LD)
    assert np.max(np.abs(np.asarray(stl["J"] - J_star, dtype=np.float64))) <= 1e-6


@pytest.mark.parametrize("m", [1, 3])
def test_ring_replaces_the_oldest_pair(m):
    n = 7
    Q, c = ref.quadratic(n, 11)
    x0 = np.random.default_rng(12).uniform(size=(1, n))
    trace = []
    ref.search(_quad_fun(Q, c), x0, n, 1, 12, m, C1, 0.0, trace=trace)
    pairs, dropped = [], 0
    prev = ref.init(x0, n, 1, m)
    for k, st, infos in trace:
        i = infos[0]
        if i["pushed"]:
            pairs.append((st["x"][0] - prev["x"][0], st["g"][0] - prev["g"][0]))
            dropped += i["dropped_oldest"]
        if i["reset"]:
            pairs = []
        held = pairs[-m:]
        assert int(st["pushes"][0]) == len(pairs) or i["branch"] == "frozen"
        for j, (s, y) in enumerate(reversed(held)):              # newest first
            slot = (len(pairs) - 1 - j) % m
            assert np.array_equal(st["S"][0, slot], s) and np.array_equal(st["Y"][0, slot], y)
            assert st["sy"][0, slot] == np.sum(s * y) and st["yy"][0, slot] == np.sum(y * y)
        prev = st
    assert dropped >= 2 and len(pairs) > m


# -- 2. every branch, by the hand-made sequences -----------------------------------------------------------------------------------
def _script_case(n, H, A, m, deriv, dtype=np.float64, seed=0):
    Q, c = ref.quadratic(n, 20 + seed)
    x0 = np.random.default_rng(30 + seed).uniform(0.05, 0.95, size=(len(ref.SCRIPTS), n))
    kw = dict(max_change=np.linspace(0.3, 0.9, A), action_prev=np.linspace(0.2, 0.8, A)) if deriv else {}
    return ref.run_scripts(ref.SCRIPTS, x0, Q, c, H, A, m, C1, PGTOL, dtype=dtype, **kw)


@pytest.mark.parametrize("deriv", [False, True])
@pytest.mark.parametrize("n,H,A,m", [(1, 1, 1, 1), (12, 4, 3, 3), (65, 13, 5, 10)])
def test_hand_made_sequences_reach_every_branch(n, H, A, m, deriv):
    trace = _script_case(n, H, A, m, deriv)
    idx = {name: b for b, name in enumerate(ref.SCRIPTS)}
    seen = {name: [t[2][b] for t in trace] for name, b in idx.items()}
    final = trace[-1][1]
    ev = seen["events"]
    assert [ev[k]["branch"] for k in ref.EVENT_REJECTS] == ["reject"] * len(ref.EVENT_REJECTS)
    for k in ref.EVENT_REJECTS[1:]:                              # exactly one non-finite value was fed at each of them
        Jk, Gk = trace[k][3][idx["events"]], trace[k][4][idx["events"]]
        assert int(not np.isfinite(Jk)) + int(np.sum(~np.isfinite(Gk))) == 1, k
    fed = {k: (trace[k][3][idx["events"]], trace[k][4][idx["events"]]) for k in ref.EVENT_REJECTS}
    assert np.isnan(fed[6][0]) and fed[8][0] == -np.inf and fed[9][0] == np.inf
    assert np.any(fed[7][1] == np.inf) and np.any(np.isnan(fed[10][1])) and np.any(fed[11][1] == -np.inf)
    assert ev[4]["branch"] == "accept" and ev[4]["skipped"] and not ev[4]["pushed"]            # the curvature skip
    assert any(i["pushed"] for i in ev) and final["status"][idx["events"]] == 1
    assert any(i["branch"] == "converged" for i in ev)
    ov = seen["overflow"]
    assert ov[0]["branch"] == "accept" and ov[0]["reset"]                                        # the non-descent reset
    assert [i["branch"] for i in ov[1:41]] == ["reject"] * 40 and ov[41]["branch"] == "underflow"
    assert final["status"][idx["overflow"]] == 2 and final["alpha"][idx["overflow"]] == 2.0 ** -41
    assert np.array_equal(final["xt"][idx["overflow"]], final["x"][idx["overflow"]])
    for name in ref.START_FAULTS:                                # J = NaN, +inf, -inf; one NaN, +inf, -inf entry of G -- each alone
        J0, G0 = trace[0][3][idx[name]], trace[0][4][idx[name]]
        assert int(not np.isfinite(J0)) + int(np.sum(~np.isfinite(G0))) == 1, name
        assert seen[name][0]["branch"] == "nonfinite_start" and final["status"][idx[name]] == 3
        assert all(i["branch"] == "frozen" for i in seen[name][1:])
    nat = seen["natural"]
    assert final["status"][idx["natural"]] == 1 and sum(i["pushed"] for i in nat) >= 2
    if n > 1:                                                    # both bound cases of the free set
        every = [i for name in ("natural", "events") for i in seen[name]]
        assert any(i["fixed_lo"] > 0 for i in every) and any(i["fixed_hi"] > 0 for i in every)
    if m < 4 and n > 1:
        assert any(i["dropped_oldest"] for i in nat + ev)
    # a finished restart's state no longer changes
    for (k0, s0, *_), (k1, s1, *_) in zip(trace[:-1], trace[1:]):
        for b in np.flatnonzero(s0["status"] != 0):
            for key in s0:
                assert np.array_equal(s0[key][b], s1[key][b], equal_nan=True), (k1, b, key)
    # every decision of the longdouble restatement is taken with room to spare: the GPU test's precondition
    trace_ld = _script_case(n, H, A, m, deriv, dtype=LD)
    margin = min(ref.min_margin(t[2]) for t in trace_ld)
    print("smallest relative margin", margin)
    assert margin >= 1e-6
    for t64, tld in zip(trace, trace_ld):
        assert [i["branch"] for i in t64[2]] == [i["branch"] for i in tld[2]]


@pytest.mark.parametrize("A,H,time", ref.CHAIN_SHAPES)
def test_chain_decisions_on_the_oracle_have_room_to_spare(A, H, time):
    """The precondition of the GPU test's chain on the model, checked here first with the oracle's J and G for its 65 starts: every
    Armijo, curvature and descent decision of the longdouble restatement has a relative margin >= 1e-6.  A failure means: change
    the seed of chain_starts (or of the workload)."""
    from lbfgs_stub_engine import LbfgsOracleEngine
    w = synth.make_workload(N=24, D=2, A=A, H=H, B=2, include_time=time, time0=3.0, seed=7)
    eng = LbfgsOracleEngine()
    eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    eng.set_cost(np.full(2 + A, 0.5), np.eye(2 + A), np.eye(2), w.kappa)
    for propagation in ("moment", "linearized"):
        grad_of = eng.rollout_grad if propagation == "moment" else eng.rollout_linear_grad
        for deriv in (False, True):
            kw = ref.chain_kw(A, deriv)

            def fun(actions):
                out = grad_of(actions, w.mu0, w.S0, w.include_time, w.time0)
                return out["J"].numpy(), out["grad"].numpy()
            trace = []
            st = ref.search(fun, ref.chain_starts(A, H), H, A, ref.T_CHAIN, ref.M_CHAIN, ref.C1_CHAIN, ref.PGTOL_CHAIN,
                            kw.get("max_change"), kw.get("action_prev"), dtype=LD, trace=trace)
            margin = min(ref.min_margin(infos) for _, _, infos in trace)
            print(propagation, deriv, "smallest relative margin", margin)
            assert margin >= 1e-6
            assert np.all(np.isfinite(np.asarray(st["J"], dtype=np.float64))) and np.all(st["status"] <= 1)
            assert any(i["pushed"] for _, _, infos in trace for i in infos)


# -- 3. the mappers are the controller's ------------------------------------------------------------------------------------------
def test_mapper_and_chain_rule_are_the_derivative_action_mappers():
    from gp_mpc_amd.config_classes import ActionsConfig
    from gp_mpc_amd.control_objects.actions_mappers.mappers import DerivativeActionMapper, NormalizationActionMapper
    H, A = 6, 3
    mc = [0.3, 0.7, 0.55]
    rng = np.random.default_rng(5)
    mapper = DerivativeActionMapper(np.zeros(A), np.ones(A), H, ActionsConfig(True, mc))
    prev = mapper.action_model_previous_iter.numpy()
    G = rng.standard_normal((4, H, A))
    for b in range(4):
        got = ref.chain(G[b], H, A, np.array(mc))
        assert np.array_equal(got.view(np.uint64), mapper.chain_grad_model_to_mpc(G[b]).view(np.uint64))
    X = rng.uniform(size=(4, H * A))
    acts = ref.to_model(X, H, A, np.array(mc), prev)
    assert np.any(acts == 0.0) or np.any(acts == 1.0)
    assert np.array_equal(acts, mapper.mpc_to_model_batch(X))
    ident = NormalizationActionMapper(np.zeros(A), np.ones(A), H, ActionsConfig(False, mc))
    assert np.array_equal(ref.chain(G[0], H, A), ident.chain_grad_model_to_mpc(G[0]))
    assert np.array_equal(ref.to_model(X, H, A), ident.mpc_to_model_batch(X))
    # unchain is the inverse the hand-made sequences rely on
    gt = rng.standard_normal(H * A)
    assert np.max(np.abs(ref.chain(ref.unchain(gt, H, A, np.array(mc)), H, A, np.array(mc)) - gt)) <= 1e-13


# -- 4. the controller's host logic -----------------------------------------------------------------------------------------------
def _lbfgs_controller(w, deriv, propagation, eng, starts=3, iterations=4):
    c = make_controller(w, limit_action_change=deriv, optimize=True, restarts=starts, engine=eng, shard=False)
    cc = c.config.controller
    cc.candidate_optimizer, cc.lbfgs_device_iterations, cc.lbfgs_device_history = "lbfgs_device", iterations, 3
    c.transition_model.config.uncertainty_propagation = propagation
    return c


@pytest.mark.parametrize("propagation", ["moment_matching", "linearized"])
@pytest.mark.parametrize("deriv", [False, True])
def test_lbfgs_device_behind_get_action(deriv, propagation):
    from lbfgs_stub_engine import LbfgsOracleEngine
    w = synth.make_workload(16, 2, 1, 3, 1, seed=41)
    N, D, A, E, H, B = w.dims
    eng = LbfgsOracleEngine()
    c = _lbfgs_controller(w, deriv, propagation, eng)
    np.random.seed(7)
    a = c.get_action(w.mu0, w.S0)
    assert a.shape == (A,) and np.all(np.isfinite(a))
    call = eng.lbfgs_calls[-1]
    assert call["propagation"] == ("linearized" if propagation == "linearized" else "moment")
    assert call["iterations"] == 4 and call["history"] == 3 and call["x0"].shape == (3, H * A)
    assert (call["max_change"] is not None) == deriv
    if deriv:
        assert np.array_equal(call["max_change"], [0.3] * A) and call["action_prev"].shape == (A,)
    assert ("rollout_linear" in eng.calls) == (propagation == "linearized")
    # the starts are those "lbfgs" draws under the same seed
    from gp_mpc_amd.control_objects.actions_mappers.action_init_functions import generate_mpc_action_init_random
    np.random.seed(7)
    want = np.stack([generate_mpc_action_init_random(len_horizon=H, dim_action=A) for _ in range(3)]).reshape(3, H * A)
    assert np.array_equal(call["x0"], want) and np.array_equal(c.lbfgs_device_starts, want)
    # counters and caches
    assert c.num_rollouts == 3 * 4 + 1 and c.lbfgs_evaluations == 4
    assert c.candidates_final_J.shape == (3,) and c.best_candidate_J == np.min(c.candidates_final_J)
    assert c.best_candidate_index == int(np.argmin(c.candidates_final_J))
    assert abs(c.cost_traj_mean_lcb.item() + c.best_candidate_J) <= 1e-9 * abs(c.best_candidate_J)
    assert c.states_mu_pred.shape == (H + 1, D)
    # the search went down from its starts
    acts0 = c.actions_mapper.mpc_to_model_batch(want) if not deriv else None
    if acts0 is not None:
        grad_of = eng.rollout_grad if propagation == "moment_matching" else eng.rollout_linear_grad
        J0 = grad_of(acts0, w.mu0, w.S0, w.include_time, float(w.time0))["J"].numpy()
        assert np.all(c.candidates_final_J <= J0) and c.best_candidate_J < np.min(J0)
    # the next step warm-starts: slot 0 is the shifted previous solution
    best = c.actions_mpc_previous_iter.copy()
    from gp_mpc_amd.control_objects.actions_mappers.action_init_functions import generate_mpc_action_init_frompreviousiter
    c.get_action(w.mu0, w.S0)
    shifted = np.asarray(generate_mpc_action_init_frompreviousiter(best, dim_action=A)).reshape(-1)
    assert np.array_equal(eng.lbfgs_calls[-1]["x0"][0], shifted)
    assert c.num_rollouts == 2 * (3 * 4 + 1)


def test_same_starts_as_the_lockstep_scipy_search():
    from lbfgs_stub_engine import LbfgsOracleEngine
    w = synth.make_workload(16, 2, 1, 3, 1, seed=41)
    eng = LbfgsOracleEngine()
    c = _lbfgs_controller(w, False, "moment_matching", eng, starts=4, iterations=1)
    np.random.seed(9)
    c.get_action(w.mu0, w.S0)
    bat = make_controller(w, optimize=True, restarts=4, engine=LbfgsOracleEngine(), shard=False,
                          optimizer_params={"maxfun": 1, "maxiter": 1})
    bat.config.controller.candidate_optimizer = "lbfgs"
    seen = []
    orig = bat.objective_and_gradient_batch
    bat.objective_and_gradient_batch = lambda X, *a: (seen.append(np.array(X)), orig(X, *a))[1]
    np.random.seed(9)
    bat.get_action(w.mu0, w.S0)
    assert np.array_equal(seen[0], eng.lbfgs_calls[0]["x0"])


def test_refusals():
    from lbfgs_stub_engine import LbfgsOracleEngine
    w = synth.make_workload(16, 2, 1, 3, 1, seed=41)
    # closed-loop planning
    c = _lbfgs_controller(w, False, "linearized", LbfgsOracleEngine())
    c.config.controller.feedback_gain = np.zeros((1, 2))
    with pytest.raises(ValueError, match="feedback_gain"):
        c.get_action(w.mu0, w.S0)
    c = _lbfgs_controller(w, False, "moment_matching", LbfgsOracleEngine())
    c.config.controller.feedback_gain = np.zeros((1, 2))
    with pytest.raises(ValueError, match="feedback_gain"):
        c.get_action(w.mu0, w.S0)
    # sharded restarts: refused before the engine (or any collective) is touched
    eng = LbfgsOracleEngine()
    c = _lbfgs_controller(w, False, "moment_matching", eng)
    c._ranks = lambda: (2, 1)
    with pytest.raises(ValueError, match="shard"):
        c.get_action(w.mu0, w.S0)
    assert not eng.lbfgs_calls and eng.launches == 0
    # the other optimisers stay refused under the linearised propagation, and the message names what is supported
    c = make_controller(w, optimize=True, engine=LbfgsOracleEngine(), shard=False)
    c.transition_model.config.uncertainty_propagation = "linearized"
    with pytest.raises(ValueError, match="lbfgs_device"):
        c.get_action(w.mu0, w.S0)
