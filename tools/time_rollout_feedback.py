#!/usr/bin/env python3
"""Time gpmpc_rollout_feedback (HipEngine.rollout_feedback, per-candidate gains) beside gpmpc_rollout_linear_feedback with the same
gains and gpmpc_rollout for the same candidates, on the same build and the same device in one run, by the method of
tools/time_rollout_linear_feedback.py: device events around `reps` back-to-back calls after `warmup` calls, median of `trials`
such windows.  Every call returns the objective J only.  One JSON line per shape:
  ms_feedback          per gpmpc_rollout_feedback call with (B, H, A, D) gains (per horizon step: the four launches of gpmpc_moments
                       over the candidates and one step launch)
  ms_linear_feedback   per gpmpc_rollout_linear_feedback call with the same gains
  ms_rollout           per gpmpc_rollout call (the fused-horizon kernel at these shapes)
  ratio_rollout / ratio_linear_feedback   ms_feedback over the other two
Default shapes: config 2 (N = 200, D = 3, A = 1, H = 25) with B = 16 and B = 256.  Needs a GPU.
  python tools/time_rollout_feedback.py [--shape N,D,A,H,B ...] [--reps 3] [--trials 3] [--out FILE]
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

DEFAULT = ["200,3,1,25,16", "200,3,1,25,256"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A,H,B")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_rollout_feedback.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        N, D, A, H, B = (int(v) for v in spec.split(","))
        w = synth.make_workload(N, D, A, H, B, seed=5, dynamics="contracting")
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        acts = torch.as_tensor(w.actions, device=eng.device)
        gains = torch.as_tensor(0.1 * np.random.default_rng(6).standard_normal((B, H, A, D)), device=eng.device)
        outs = [{"J": torch.empty(B, dtype=torch.float64, device=eng.device)} for _ in range(3)]
        w_, r_, t_ = args.warmup, args.reps, args.trials
        ms_f, spread_f = time_calls(lambda: eng.rollout_feedback(acts, gains, w.mu0, w.S0, out=outs[0]), w_, r_, t_)
        ms_l, spread_l = time_calls(lambda: eng.rollout_linear_feedback(acts, gains, w.mu0, w.S0, out=outs[1]), w_, r_, t_)
        ms_r, spread_r = time_calls(lambda: eng.rollout(acts, w.mu0, w.S0, out=outs[2]), w_, r_, t_)
        line = json.dumps({"N": N, "D": D, "A": A, "H": H, "B": B, "ms_feedback": round(ms_f, 4),
                           "ms_feedback_trials": [round(v, 4) for v in spread_f], "ms_linear_feedback": round(ms_l, 4),
                           "ms_linear_feedback_trials": [round(v, 4) for v in spread_l], "ms_rollout": round(ms_r, 4),
                           "ms_rollout_trials": [round(v, 4) for v in spread_r], "ratio_rollout": round(ms_f / ms_r, 2),
                           "ratio_linear_feedback": round(ms_f / ms_l, 2), "launches_per_step": 5,
                           "J_finite": bool(torch.isfinite(outs[0]["J"]).all()), "build_id": eng.build_id})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
