"""tests/linear_stub_engine.LinearOracleEngine plus HipEngine's closed-loop entry `rollout_linear_feedback`, computed by the
numpy restatement of tests/feedback_rollout_ref.py; it records its calls and the gains it was given.  TEST CODE ONLY: the CPU
tests of the `feedback_gains` / `ControllerConfig.feedback_gain` plumbing run against it."""
import numpy as np
import torch

import feedback_rollout_ref as fb
from linear_stub_engine import LinearOracleEngine


class FeedbackOracleEngine(LinearOracleEngine):
    def __init__(self):
        super().__init__()
        self.gains_seen = []

    def _reward_config(self):
        from types import SimpleNamespace
        target, W, W_T, kappa, clip, smin, smax = self._cost
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))       # noqa: E731
        D = np.asarray(W_T).shape[0]
        return SimpleNamespace(target_state_action_norm=t(target), target_state_norm=t(target)[:D], weight_matrix_cost=t(W),
                               weight_matrix_cost_terminal=t(W_T), exploration_factor=kappa, clip_lower_bound_cost_to_0=clip,
                               use_constraints=smin is not None, state_min=None if smin is None else t(smin),
                               state_max=None if smax is None else t(smax))

    def rollout_linear_feedback(self, actions, gains, mu0, S0, include_time=False, time0=0.0, trajectories=True,
                                stage_costs=True, out=None):
        if gains is None:
            return self.rollout_linear(actions, mu0, S0, include_time, time0, trajectories, stage_costs, out)
        self.calls.append("rollout_linear_feedback")
        actions = np.asarray(actions, dtype=np.float64)
        gains = np.asarray(gains, dtype=np.float64)
        self.gains_seen.append(gains.copy())
        self.launches += 1
        mu, Sig = fb.rollout(*self._factors(), actions, gains, np.asarray(mu0), np.asarray(S0), include_time, time0)
        t = torch.as_tensor
        res = {}
        if trajectories:
            res.update(mu=t(mu), Sig=t(Sig))
        if stage_costs:
            cm, cv, J = fb.costs(self._reward_config(), mu, Sig, actions, gains)
            res.update(J=t(J), cost_mu=t(cm), cost_var=t(cv))
        return res
