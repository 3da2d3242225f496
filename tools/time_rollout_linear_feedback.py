#!/usr/bin/env python3
"""Time gpmpc_rollout_linear_feedback (HipEngine.rollout_linear_feedback, per-candidate gains) beside gpmpc_rollout_linear for the
same candidates, on the same build and the same device, by the method of tools/time_rollout_linear.py: device events around
`reps` back-to-back calls after `warmup` calls, median of `trials` such windows.  Both calls return the objective J only.  One
JSON line per shape:
  ms_linear       per gpmpc_rollout_linear call
  ms_feedback     per gpmpc_rollout_linear_feedback call with (B, H, A, D) gains (the same tile launches; the step kernel forms
                  C = V_s + K^T V_u, the cost kernel the closed-loop stage costs)
  ms_shared       the same with one (H, A, D) gain sequence shared by the candidates
  ratio           ms_feedback / ms_linear
Default shapes: config 2 (N = 200, D = 3, H = 25, B = 256), config 4 (N = 1000, D = 4, H = 30, B = 2048), and two with D > 4, where
the cost kernel keeps its per-lane arrays in scratch: N = 500, D = 6, H = 20, B = 512 and the config-5 class (N = 4096, D = 16,
H = 50, B = 64).  Needs a GPU.
  python tools/time_rollout_linear_feedback.py [--shape N,D,A,H,B ...] [--reps 3] [--trials 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_mpc_amd  # noqa: E402
from oracle import synth  # noqa: E402
from time_predict import time_calls  # noqa: E402

DEFAULT = ["200,3,1,25,256", "1000,4,2,30,2048", "500,6,2,20,512", "4096,16,4,50,64"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A,H,B")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trials", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_rollout_linear_feedback.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        N, D, A, H, B = (int(v) for v in spec.split(","))
        w = synth.make_workload(N, D, A, H, B, seed=5, dynamics="contracting")
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        acts = torch.as_tensor(w.actions, device=eng.device)
        gains = torch.as_tensor(0.1 * np.random.default_rng(6).standard_normal((B, H, A, D)), device=eng.device)
        shared = gains[0].contiguous()
        outs = [{"J": torch.empty(B, dtype=torch.float64, device=eng.device)} for _ in range(3)]
        w_, r_, t_ = args.warmup, args.reps, args.trials
        ms_l, spread_l = time_calls(lambda: eng.rollout_linear(acts, w.mu0, w.S0, out=outs[0]), w_, r_, t_)
        ms_f, spread_f = time_calls(lambda: eng.rollout_linear_feedback(acts, gains, w.mu0, w.S0, out=outs[1]), w_, r_, t_)
        ms_s, spread_s = time_calls(lambda: eng.rollout_linear_feedback(acts, shared, w.mu0, w.S0, out=outs[2]), w_, r_, t_)
        print(json.dumps({"N": N, "D": D, "A": A, "H": H, "B": B, "ms_linear": round(ms_l, 4),
                          "ms_linear_trials": [round(v, 4) for v in spread_l], "ms_feedback": round(ms_f, 4),
                          "ms_feedback_trials": [round(v, 4) for v in spread_f], "ms_shared": round(ms_s, 4),
                          "ms_shared_trials": [round(v, 4) for v in spread_s], "ratio": round(ms_f / ms_l, 3),
                          "J_finite": bool(torch.isfinite(outs[1]["J"]).all()), "build_id": eng.build_id}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
