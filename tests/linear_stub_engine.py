"""tests/stub_engine.OracleEngine plus the two linearised entries of HipEngine (`moments_linear`, `rollout_linear`), computed
by the numpy restatement of tests/linear_moments_ref.py.  TEST CODE ONLY: the CPU tests of the model / controller plumbing of
ModelConfig.uncertainty_propagation = "linearized" run against it."""
import numpy as np
import torch

import linear_moments_ref as lin
from oracle import gpmpc_oracle as orc
from stub_engine import OracleEngine


class LinearOracleEngine(OracleEngine):
    def __init__(self):
        super().__init__()
        self.calls = []

    def _factors(self):
        f = self.f
        return f.X, f.lengthscales, f.variances, f.iK, f.beta

    def moments(self, mu, var=None, S=True, V=True):
        self.calls.append("moments")
        mu = np.asarray(mu, dtype=np.float64)
        s = np.zeros((mu.shape[0], mu.shape[1], mu.shape[1])) if var is None else np.asarray(var, dtype=np.float64)
        M, Sm, Vm = orc.moment_match_step(self.f, mu, s)
        return {"M": torch.as_tensor(M), "S": torch.as_tensor(Sm), "V": torch.as_tensor(Vm)}

    def moments_linear(self, mu, var=None, S=True, V=True):
        self.calls.append("moments_linear")
        M, Sm, Vm, _ = lin.step(*self._factors(), np.asarray(mu, dtype=np.float64),
                                None if var is None else np.asarray(var, dtype=np.float64))
        out = {"M": torch.as_tensor(M)}
        if S:
            out["S"] = torch.as_tensor(Sm)
        if V:
            out["V"] = torch.as_tensor(Vm)
        return out

    def rollout(self, *args, **kwargs):
        self.calls.append("rollout")
        return super().rollout(*args, **kwargs)

    def rollout_linear(self, actions, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True, out=None):
        self.calls.append("rollout_linear")
        actions = np.asarray(actions, dtype=np.float64)
        self.launches += 1
        mu, Sig = lin.rollout(*self._factors(), actions, np.asarray(mu0), np.asarray(S0), include_time, time0)
        t = torch.as_tensor
        res = {}
        if trajectories:
            res.update(mu=t(mu), Sig=t(Sig))
        if stage_costs:
            target, W, W_T, kappa, clip, smin, smax = self._cost
            cm, cv = orc.stage_costs(mu, Sig, actions, target, W, W_T, smin, smax)
            res.update(J=t(orc.lcb_objective(cm, cv, kappa, clip)), cost_mu=t(cm), cost_var=t(cv))
        return res
