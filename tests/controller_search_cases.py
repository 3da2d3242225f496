"""What one candidate search of GpMpcController does, recorded without a GPU: `_get_optimal_actions` runs against a
stand-in engine whose objective is an exact function of the actions, and every call it makes to the engine and to the model,
every draw it takes from numpy's global generator and everything it leaves on the controller is noted.
tests/test_controller_search_traces.py compares the record with tests/golden/controller_search_traces.json, written by
tools/gen_controller_search_golden.py.

The cases: every key of the search table (optimize=False, candidate_optimizer None, "cem", "cem_device", "lbfgs",
"lbfgs_device", "ilqr_device") x {first control step, second step with a previous solution} x {normalisation mapper,
DerivativeActionMapper where the search allows it}, on one rank.  Per case: the ordered calls (name, integers and floats by
value, arrays with shape and values), `np.random.random()` drawn right after the search (how many draws it consumed), the
returned action and the public attributes the search left behind."""
import math
import re

import numpy as np
import torch

from helpers import make_controller
from oracle import synth
from stub_engine import OracleEngine

N, D, A, H = 8, 2, 1, 3
RESTARTS, CEM_CANDIDATES, CEM_ITERATIONS = 3, 6, 2
CENTRE = 0.3                            # the objective: mean((x - CENTRE)^2) over the H*A actions of a sequence

# attributes a search may leave on the controller (the five logging caches are read through their properties)
ATTRIBUTES = re.compile(r"best_candidate_\w+|candidates_final_\w+|\w+_starts|lbfgs_evaluations|ilqr_iterations_run|num_rollouts|"
                        r"actions_mpc_previous_iter")
CACHES = ("states_mu_pred", "states_var_pred", "rewards_trajectory", "rewards_traj_var", "cost_traj_mean_lcb")
MODEL_METHODS = ("prepare_inference", "set_cost", "predict_trajectory_batch", "objective_and_gradient_batch",
                 "objective_and_gradient_host")


def encode(v):
    """JSON form of a recorded value: integers, floats, strings by value; arrays with dtype, shape and values."""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    if isinstance(v, np.ndarray):
        return {"dtype": str(v.dtype), "shape": list(v.shape), "values": v.reshape(-1).tolist()}
    if isinstance(v, (list, tuple)):
        return [encode(x) for x in v]
    if isinstance(v, dict):
        return {str(k): encode(x) for k, x in v.items()}
    return {"object": type(v).__name__}


class ExactEngine:
    """The method set of the stub engines (tests/stub_engine.py and its subclasses); the objective is computed with math.fsum
    over elementwise IEEE operations, so it is the same on every machine; trajectories and stage costs are zeros of the right
    shapes.  The three device searches return a fixed rule of their inputs: the first start, its J, J of all starts, status 0."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.calls = []

    def _note(self, name, *args, **kwargs):
        self.calls.append({"call": name, "args": encode(args), "kwargs": encode(kwargs)})

    @staticmethod
    def objective(X):
        X = np.asarray(X, dtype=np.float64)
        X = X.reshape(X.shape[0], -1)
        return np.array([math.fsum((float(x) - CENTRE) * (float(x) - CENTRE) for x in row) / X.shape[1] for row in X])

    def prepare(self, X, Y, lengthscales, outputscales, noises):
        self._note("prepare", X, Y, lengthscales, outputscales, noises)

    def set_cost(self, *args):
        self._note("set_cost", *args)

    def _rollout(self, name, actions, mu0, S0, include_time, time0, trajectories, stage_costs):
        self._note(name, actions, mu0, S0, include_time, time0, trajectories, stage_costs)
        actions = np.asarray(actions, dtype=np.float64)
        B = actions.shape[0]
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64)                          # noqa: E731
        out = {"J": torch.as_tensor(self.objective(actions)), "cost_mu": z(B, H + 1), "cost_var": z(B, H + 1)}
        if trajectories:
            out.update(mu=z(B, H + 1, D), Sig=z(B, H + 1, D, D))
        return out

    def rollout(self, actions, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True, out=None):
        return self._rollout("rollout", actions, mu0, S0, include_time, time0, trajectories, stage_costs)

    def rollout_linear(self, actions, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True, out=None):
        return self._rollout("rollout_linear", actions, mu0, S0, include_time, time0, trajectories, stage_costs)

    def argmin_async(self, J, first_global_index=0, actions=None, out=None):
        self._note("argmin_async", J, first_global_index=first_global_index, actions=actions)
        return OracleEngine.argmin_async(self, J, first_global_index, actions, out)

    def rollout_grad(self, actions, mu0, S0, include_time=False, time0=0.0, trajectories=False):
        self._note("rollout_grad", actions, mu0, S0, include_time, time0, trajectories)
        actions = np.asarray(actions, dtype=np.float64)
        out = {"J": torch.as_tensor(self.objective(actions)), "grad": torch.as_tensor(2.0 * (actions - CENTRE) / (H * A))}
        out["packed"] = torch.cat([out["J"], out["grad"].reshape(-1)])
        out["layout"] = [("J", tuple(out["J"].shape), 0, out["J"].numel()),
                         ("grad", tuple(out["grad"].shape), out["J"].numel(), out["grad"].numel())]
        return out

    host_views = staticmethod(OracleEngine.host_views)

    def objective_grad_host(self, actions, mu0, S0, include_time=False, time0=0.0):
        self._note("objective_grad_host", actions, mu0, S0, include_time, time0)
        actions = np.asarray(actions, dtype=np.float64)[None]
        return {"J": self.objective(actions), "grad": 2.0 * (actions - CENTRE) / (H * A), "mu": np.zeros((1, H + 1, D)),
                "Sig": np.zeros((1, H + 1, D, D)), "cost_mu": np.zeros((1, H + 1)), "cost_var": np.zeros((1, H + 1))}

    def cem_search(self, mu0, S0, B, H, A, iterations, n_elite, **kwargs):
        self._note("cem_search", mu0, S0, B, H, A, iterations, n_elite, **kwargs)
        first = kwargs.get("first_candidate")
        x = np.full(H * A, (kwargs["seed"] % 997) / 997.0) if first is None else np.array(first, dtype=np.float64).reshape(-1)
        return x, float(self.objective(x[None])[0])

    def _first_start(self, name, x0, *args, **kwargs):
        self._note(name, x0, *args, **kwargs)
        x0 = np.asarray(x0, dtype=np.float64)
        J = self.objective(x0)
        return x0[0].copy(), float(J[0]), J, np.zeros(x0.shape[0], dtype=np.int64)

    def lbfgs_search_host(self, x0, mu0, S0, H, A, iterations, **kwargs):
        return self._first_start("lbfgs_search_host", x0, mu0, S0, H, A, iterations, **kwargs)

    def ilqr_search_host(self, x0, mu0, S0, H, A, iterations, **kwargs):
        return self._first_start("ilqr_search_host", x0, mu0, S0, H, A, iterations, **kwargs)


OPTIMIZERS = (False, None, "cem", "cem_device", "lbfgs", "lbfgs_device", "ilqr_device")
CASES = [(f"{'shooting' if opt is False else opt or 'scipy'}-{'deriv' if deriv else 'norm'}-step{step}", opt, deriv, step)
         for opt in OPTIMIZERS for deriv in (False, True) for step in (1, 2) if not (deriv and opt == "ilqr_device")]
IDS = [c[0] for c in CASES]


def controller(opt, deriv, engine, feedback_gain=None, propagation=None):
    w = synth.make_workload(N, D, A, H, 1, seed=5)
    c = make_controller(w, limit_action_change=deriv, optimize=opt is not False, restarts=RESTARTS, engine=engine, shard=False)
    if deriv:                           # the mapper draws its first previous action from torch's generator: a fixed one here
        c.actions_mapper.action_model_previous_iter = torch.full((A,), 0.4, dtype=torch.float64)
    cc = c.config.controller
    cc.candidate_optimizer = opt or None
    cc.cem_candidates, cc.cem_iterations, cc.cem_elite_fraction = CEM_CANDIDATES, CEM_ITERATIONS, 0.34
    cc.lbfgs_device_iterations, cc.lbfgs_device_history = 4, 3
    cc.ilqr_iterations, cc.ilqr_line_search_steps, cc.ilqr_reg = 2, 3, 1e-2
    cc.feedback_gain = feedback_gain
    if propagation is None:
        propagation = "linearized" if opt == "ilqr_device" else "moment_matching"
    c.transition_model.config.uncertainty_propagation = propagation
    return c, w


def run_case(case):
    cid, opt, deriv, step = case
    eng = ExactEngine()
    c, w = controller(opt, deriv, eng)
    mu0, S0 = torch.as_tensor(w.mu0), torch.as_tensor(w.S0)
    k = IDS.index(cid)
    if step == 2:                       # a whole control step first: a previous solution, the mapper's previous action, time 1
        np.random.seed(1000 + k)
        c.get_action(w.mu0, w.S0)
        eng.calls.clear()
    tm = c.transition_model
    for name in MODEL_METHODS:          # the model's methods note themselves in the same list, ahead of the engine call they make
        def noted(*args, _name=name, _fn=getattr(tm, name), **kwargs):
            eng._note("model." + _name, *args, **kwargs)
            return _fn(*args, **kwargs)
        setattr(tm, name, noted)
    np.random.seed(k)
    action = c._get_optimal_actions(mu0, S0)
    rec = {"calls": eng.calls, "next_draw": float(np.random.random()), "action": encode(action)}
    left = {name: encode(v) for name, v in vars(c).items() if ATTRIBUTES.fullmatch(name)}
    for name in CACHES:
        left[name] = encode(getattr(c, name))
    rec["attributes"] = left
    return rec


def run_all():
    return {case[0]: run_case(case) for case in CASES}


def assert_same(got, want, where=""):
    """Names, order, integers, shapes and the sets of keys exactly; floats to rtol = 1e-9, atol = 0."""
    assert type(got) is type(want), (where, type(got), type(want))
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), (where, sorted(got), sorted(want))
        for key in want:
            assert_same(got[key], want[key], f"{where}/{key}")
    elif isinstance(want, list):
        assert len(got) == len(want), (where, len(got), len(want))
        for i, (a, b) in enumerate(zip(got, want)):
            assert_same(a, b, f"{where}[{i}]")
    elif isinstance(want, float):
        assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= 1e-9 * abs(want), (where, got, want)
    else:
        assert got == want, (where, got, want)
