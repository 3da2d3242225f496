"""tests/feedback_stub_engine.FeedbackOracleEngine plus HipEngine's two LQR entries (`lqr_gains`, `rollout_linear_lqr`), computed
by the numpy restatement of tests/lqr_gains_ref.py; it records its calls and the `reg` it was given.  TEST CODE ONLY: the CPU tests
of the `feedback_gains="lqr"` / `ControllerConfig(feedback_gain="lqr")` plumbing run against it."""
import numpy as np
import torch

import lqr_gains_ref as lq
from feedback_stub_engine import FeedbackOracleEngine


class LqrOracleEngine(FeedbackOracleEngine):
    def __init__(self):
        super().__init__()
        self.regs_seen = []

    def lqr_gains(self, actions, mu0, include_time=False, time0=0.0, reg=0.0, want_cost_to_go=False, want_flags=False):
        self.calls.append("lqr_gains")
        self.regs_seen.append(float(reg))
        target, W, W_T = self._cost[:3]
        K, P, flags = lq.gains(*self._factors(), np.asarray(actions, dtype=np.float64), np.asarray(mu0), W, W_T, include_time,
                               time0, reg)
        out = {"gains": torch.as_tensor(K)}
        if want_cost_to_go:
            out["P"] = torch.as_tensor(P)
        if want_flags:
            out["flags"] = torch.as_tensor(flags)
        return out

    def rollout_linear_lqr(self, actions, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True, out=None,
                           reg=0.0):
        gains = self.lqr_gains(actions, mu0, include_time, time0, reg)["gains"]
        res = self.rollout_linear_feedback(actions, gains, mu0, S0, include_time, time0, trajectories, stage_costs, out)
        res["gains"] = gains
        return res
