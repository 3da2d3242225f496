"""tests/lqr_stub_engine.LqrOracleEngine plus HipEngine's two closed-loop moment-matched entries (`rollout_feedback`,
`rollout_feedback_lqr`), computed by the numpy restatement of tests/feedback_mm_ref.py; it records its calls and the gains it was
given.  TEST CODE ONLY: the CPU tests of GpStateTransitionModel.predict_trajectory_feedback(_batch) run against it."""
import numpy as np
import torch

import feedback_mm_ref as fm
from lqr_stub_engine import LqrOracleEngine


class FeedbackMmOracleEngine(LqrOracleEngine):
    def rollout_feedback(self, actions, gains, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True,
                         out=None):
        self.calls.append("rollout_feedback")
        actions = np.asarray(actions, dtype=np.float64)
        B, H, A = actions.shape
        gains = np.zeros((H, A, self.f.lengthscales.shape[0])) if gains is None else np.asarray(gains, dtype=np.float64)
        self.gains_seen.append(gains.copy())
        self.launches += 1
        mu, Sig = fm.rollout(self.f, actions, gains, np.asarray(mu0), np.asarray(S0), include_time, time0)
        t = torch.as_tensor
        res = {}
        if trajectories:
            res.update(mu=t(mu), Sig=t(Sig))
        if stage_costs:
            cm, cv, J = fm.costs(self._reward_config(), mu, Sig, actions, gains)
            res.update(J=t(J), cost_mu=t(cm), cost_var=t(cv))
        return res

    def rollout_feedback_lqr(self, actions, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True, out=None,
                             reg=0.0):
        gains = self.lqr_gains(actions, mu0, include_time, time0, reg)["gains"]
        res = self.rollout_feedback(actions, gains, mu0, S0, include_time, time0, trajectories, stage_costs, out)
        res["gains"] = gains
        return res
