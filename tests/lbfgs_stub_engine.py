"""tests/stub_engine.OracleEngine (through tests/linear_stub_engine.LinearOracleEngine, for the linearised rollout) plus
HipEngine.lbfgs_search_host, computed by the numpy restatement of tests/lbfgs_device_ref.py on the oracle's objective and
gradient (oracle/adjoint.py; the closed forms of tests/linear_moments_torch_ref.py for the linearised propagation).  TEST CODE
ONLY: the CPU tests of the controller plumbing of candidate_optimizer = "lbfgs_device" run against it."""
import numpy as np
import torch

import lbfgs_device_ref as ref
import linear_moments_torch_ref as lin_t
from linear_stub_engine import LinearOracleEngine


class LbfgsOracleEngine(LinearOracleEngine):
    def __init__(self):
        super().__init__()
        self.lbfgs_calls = []

    def rollout_linear_grad(self, actions, mu0, S0, include_time=False, time0=0.0):
        actions = np.asarray(actions, dtype=np.float64)
        J = self.rollout_linear(actions, mu0, S0, include_time, time0, trajectories=False)["J"].numpy()
        target, W, W_T, kappa, clip, smin, smax = self._cost
        cost = dict(target=target, W=W, W_T=W_T, kappa=kappa, constraints=None if smin is None else (smin, smax))
        grad, _, _ = lin_t.rollout_backward_closed(self._factors(), cost, actions, np.asarray(mu0), np.asarray(S0), include_time,
                                                   time0, J_bar=np.ones(actions.shape[0]))
        return {"J": torch.as_tensor(J), "grad": torch.as_tensor(grad)}

    def lbfgs_search_host(self, x0, mu0, S0, H, A, iterations, history=10, c1=1e-4, pgtol=1e-5, propagation="moment",
                          include_time=False, time0=0.0, max_change=None, action_prev=None):
        x0 = np.asarray(x0, dtype=np.float64)
        self.lbfgs_calls.append(dict(x0=x0.copy(), iterations=iterations, history=history, propagation=propagation,
                                     max_change=None if max_change is None else np.array(max_change),
                                     action_prev=None if action_prev is None else np.array(action_prev), time0=time0))
        grad_of = self.rollout_grad if propagation == "moment" else self.rollout_linear_grad

        def fun(actions):
            out = grad_of(actions, mu0, S0, include_time, time0)
            return out["J"].numpy(), out["grad"].numpy()
        return ref.search_host(fun, x0, H, A, iterations, history, c1, pgtol, max_change, action_prev)
