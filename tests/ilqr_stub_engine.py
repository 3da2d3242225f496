"""tests/linear_stub_engine.LinearOracleEngine plus HipEngine.ilqr_search_host, computed by the numpy restatement of
tests/ilqr_ref.py (the iterations) and tests/linear_moments_ref.py (the final LCB objective); it records its calls.  TEST CODE
ONLY: the CPU tests of the controller plumbing of candidate_optimizer = "ilqr_device" run against it."""
import numpy as np

import ilqr_ref as ref
from linear_stub_engine import LinearOracleEngine


class IlqrOracleEngine(LinearOracleEngine):
    def __init__(self):
        super().__init__()
        self.ilqr_calls = []

    def ilqr_search_host(self, x0, mu0, S0, H, A, iterations, line_search_steps=8, reg0=1e-3, reg_factor=10.0, reg_max=1e6, tol=1e-9,
                         include_time=False, time0=0.0):
        x0 = np.asarray(x0, dtype=np.float64)
        self.ilqr_calls.append(dict(x0=x0.copy(), iterations=iterations, line_search_steps=line_search_steps, reg0=reg0,
                                    include_time=include_time, time0=time0))
        B = x0.shape[0]
        target, W, W_T = self._cost[:3]
        fa = self._factors()
        mu0 = np.asarray(mu0, dtype=np.float64)
        st = ref.init(x0.reshape(B, H, A), line_search_steps, reg0)
        mean, linearise = ref.gp_problem(fa, mu0, include_time, time0)
        for _ in range(iterations):
            ref.step(st, mean, linearise, mu0, target, W, W_T, reg0, reg_factor, reg_max, tol)
        J = self.rollout_linear(st["actions"], mu0, S0, include_time, time0, trajectories=False)["J"].numpy()
        sel = np.where(np.isnan(J), np.inf, J)
        best = int(np.argmin(sel))                                # the first strict minimum: gpmpc_argmin's rule
        return st["actions"][best].reshape(-1).copy(), float(J[best]), J, st["status"].astype(np.int64)
