"""tests/feedback_mm_stub_engine.FeedbackMmOracleEngine plus HipEngine's two gradient entries of the closed-loop moment-matched
rollout (`rollout_feedback_backward`, `rollout_feedback_grad`), computed by torch autograd of the restatement of
tests/feedback_mm_torch_ref.py; it records its calls and the gains it was given.  TEST CODE ONLY: the CPU tests of
GpStateTransitionModel.feedback_objective_and_gradient_batch run against it."""
import numpy as np
import torch

import feedback_mm_torch_ref as fmt
from feedback_mm_stub_engine import FeedbackMmOracleEngine
from gp_mpc_amd.engine import feedback_gains_layout


class FeedbackMmGradOracleEngine(FeedbackMmOracleEngine):
    def rollout_feedback_backward(self, actions, gains, mu0, S0, include_time=False, time0=0.0, mu_bar=None, Sig_bar=None,
                                  cost_mu_bar=None, cost_var_bar=None, J_bar=None, want_initial=True, want_gains=True):
        self.calls.append("rollout_feedback_backward")
        actions = np.asarray(actions, dtype=np.float64)
        B, H, A = actions.shape
        D = self.f.lengthscales.shape[0]
        K = np.zeros((H, A, D)) if gains is None else np.asarray(gains, dtype=np.float64)
        feedback_gains_layout(K.shape, B, H, A, D)               # the engine's ValueError for a bad shape
        self.gains_seen.append(K.copy())
        self.launches += 1
        cost_on = cost_mu_bar is not None or cost_var_bar is not None or J_bar is not None
        n = lambda a: None if a is None else np.asarray(a, dtype=np.float64)      # noqa: E731
        ga, gK, gm, gS = fmt.rollout_vjp(self._factors(), self._reward_config() if cost_on else None, actions, K, np.asarray(mu0),
                                         np.asarray(S0), include_time, time0, n(mu_bar), n(Sig_bar), n(cost_mu_bar),
                                         n(cost_var_bar), n(J_bar))
        t = torch.as_tensor
        out = {"actions_bar": t(ga)}
        if want_gains and gains is not None:
            out["gains_bar"] = t(gK)
        if want_initial:
            out.update(mu0_bar=t(gm), S0_bar=t(gS))
        return out

    def rollout_feedback_grad(self, actions, gains, mu0, S0, include_time=False, time0=0.0):
        self.calls.append("rollout_feedback_grad")
        actions = np.asarray(actions, dtype=np.float64)
        if gains is not None:
            feedback_gains_layout(np.shape(gains), *actions.shape, self.f.lengthscales.shape[0])
        J = self.rollout_feedback(actions, gains, mu0, S0, include_time, time0, trajectories=False)["J"]
        back = self.rollout_feedback_backward(actions, gains, mu0, S0, include_time, time0, J_bar=np.ones(actions.shape[0]),
                                              want_initial=False)
        return {"J": J, "grad": back["actions_bar"], "gains_grad": back.get("gains_bar")}
