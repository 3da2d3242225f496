#!/usr/bin/env python3
"""Time gpmpc_rollout_backward (HipEngine.rollout_backward) against gpmpc_rollout_grad (HipEngine.rollout_grad) the way
tools/time_moments_backward.py times its entry: device events around `reps` back-to-back calls after `warmup` calls, median of
`trials` windows.  One JSON line per shape:
  ms_rollout_grad       objective + LCB gradient per call
  ms_backward_J         gpmpc_rollout_backward with the objective's seed alone (the same launches, the seeded sweep)
  ms_backward_all       with every cotangent given (trajectory, stage costs, objective) and the initial-state outputs
  ratio                 ms_backward_all / ms_rollout_grad (target: <= 1.05)
Shapes (N, D, A, H, B): config 2 at B = 1 and B = 256, config 4 at B = 256, and a D = 16 class shape.  Needs a GPU.
  python tools/time_rollout_backward.py [--shape N,D,A,H,B ...] [--reps 20] [--trials 5]
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
from time_moments import time_calls  # noqa: E402

DEFAULT = ["200,3,1,25,1", "200,3,1,25,256", "1000,4,2,30,256", "1024,16,4,10,16"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A,H,B")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_rollout_backward.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        N, D, A, H, B = (int(v) for v in spec.split(","))
        w = synth.make_workload(N, D, A, H, B, seed=5)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        rng = np.random.default_rng(8)
        act = eng._dev(w.actions)
        seeds = dict(mu_bar=eng._dev(rng.standard_normal((B, H + 1, D))), Sig_bar=eng._dev(rng.standard_normal((B, H + 1, D, D))),
                     cost_mu_bar=eng._dev(rng.standard_normal((B, H + 1))), cost_var_bar=eng._dev(rng.standard_normal((B, H + 1))),
                     J_bar=eng._dev(rng.standard_normal(B)))
        ones = eng._dev(np.ones(B))
        ms_g, spread_g = time_calls(lambda: eng.rollout_grad(act, w.mu0, w.S0), args.warmup, args.reps, args.trials)
        path = eng.last_grad_path
        ms_j, _ = time_calls(lambda: eng.rollout_backward(act, w.mu0, w.S0, J_bar=ones, want_initial=False), args.warmup,
                             args.reps, args.trials)
        ms_a, spread_a = time_calls(lambda: eng.rollout_backward(act, w.mu0, w.S0, **seeds), args.warmup, args.reps, args.trials)
        print(json.dumps({"N": N, "D": D, "A": A, "H": H, "B": B, "grad_path": path, "ms_rollout_grad": round(ms_g, 4),
                          "ms_rollout_grad_trials": [round(v, 4) for v in spread_g], "ms_backward_J": round(ms_j, 4),
                          "ms_backward_all": round(ms_a, 4), "ms_backward_all_trials": [round(v, 4) for v in spread_a],
                          "ratio": round(ms_a / ms_g, 3), "build_id": eng.build_id}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
