#!/usr/bin/env python3
"""Time gpmpc_lqr_gains (HipEngine.lqr_gains) beside gpmpc_rollout_linear_feedback with given per-candidate gains and beside the two
in sequence (HipEngine.rollout_linear_lqr), for the same candidates, on the same build and the same device, by the method of
tools/time_rollout_linear.py: device events around `reps` back-to-back calls after `warmup` calls, median of `trials` such windows.
The rollouts return the objective J only.  One JSON line per shape:
  ms_gains        per gpmpc_lqr_gains call (gains only: no cost-to-go, no flags)
  ms_feedback     per gpmpc_rollout_linear_feedback call with (B, H, A, D) gains already on the device
  ms_lqr_rollout  per rollout_linear_lqr call (the gain design, then the closed-loop rollout under those gains)
  ratio           ms_gains / ms_feedback
Default shapes: config 2 (N = 200, D = 3, A = 1, H = 25, B = 256) and config 4 (N = 1000, D = 4, A = 2, H = 30, B = 2048).  Needs a
GPU.
  python tools/time_lqr_gains.py [--shape N,D,A,H,B ...] [--reps 3] [--trials 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_mpc_amd  # noqa: E402
from oracle import synth  # noqa: E402
from time_predict import time_calls  # noqa: E402

DEFAULT = ["200,3,1,25,256", "1000,4,2,30,2048"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A,H,B")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--reg", type=float, default=1e-3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_lqr_gains.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        N, D, A, H, B = (int(v) for v in spec.split(","))
        w = synth.make_workload(N, D, A, H, B, seed=5, dynamics="contracting")
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        acts = torch.as_tensor(w.actions, device=eng.device)
        designed = eng.lqr_gains(acts, w.mu0, reg=args.reg, want_flags=True)
        gains = designed["gains"].clone()
        outs = [{"J": torch.empty(B, dtype=torch.float64, device=eng.device)} for _ in range(2)]
        w_, r_, t_ = args.warmup, args.reps, args.trials
        ms_g, spread_g = time_calls(lambda: eng.lqr_gains(acts, w.mu0, reg=args.reg), w_, r_, t_)
        ms_f, spread_f = time_calls(lambda: eng.rollout_linear_feedback(acts, gains, w.mu0, w.S0, out=outs[0]), w_, r_, t_)
        ms_b, spread_b = time_calls(lambda: eng.rollout_linear_lqr(acts, w.mu0, w.S0, out=outs[1], reg=args.reg), w_, r_, t_)
        print(json.dumps({"N": N, "D": D, "A": A, "H": H, "B": B, "ms_gains": round(ms_g, 4),
                          "ms_gains_trials": [round(v, 4) for v in spread_g], "ms_feedback": round(ms_f, 4),
                          "ms_feedback_trials": [round(v, 4) for v in spread_f], "ms_lqr_rollout": round(ms_b, 4),
                          "ms_lqr_rollout_trials": [round(v, 4) for v in spread_b], "ratio": round(ms_g / ms_f, 3),
                          "lost_pivots": int(designed["flags"].sum()), "J_equal": bool(torch.equal(outs[0]["J"], outs[1]["J"])),
                          "build_id": eng.build_id}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
