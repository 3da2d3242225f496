#!/usr/bin/env python3
"""Time gpmpc_rollout_linear (HipEngine.rollout_linear) beside gpmpc_rollout for the same candidates, on the same build and the
same device: device events around `reps` back-to-back calls after `warmup` calls, median of `trials` such windows
(tools/time_predict.py).  Both calls return the objective J only (the shape of call of the candidate searches).  One JSON line per
shape:
  ms_linear       per gpmpc_rollout_linear call (H tile launches + H step launches + the cost launch per chunk of candidates)
  ms_rollout      per gpmpc_rollout call (moment matching), with the kernel form it took (path)
  ratio           ms_rollout / ms_linear (> 1: the linearised rollout is faster)
  tflops          useful fp64 rate of the linearised rollout, 2 D B H N^2 flop per call (the K* iK products alone), and its share
                  of the 78.6 TFLOP/s fp64 matrix peak
Default shapes: config 2 (N = 200, D = 3, H = 25, B = 256), config 4 (N = 1000, D = 4, H = 30, B = 2048) and a config-5-class
shape (N = 4096, D = 16, H = 50, B = 64).  Needs a GPU.
  python tools/time_rollout_linear.py [--shape N,D,A,H,B ...] [--reps 3] [--trials 3]
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

DEFAULT = ["200,3,1,25,256", "1000,4,2,30,2048", "4096,16,4,50,64"]
PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A,H,B")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trials", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_rollout_linear.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        N, D, A, H, B = (int(v) for v in spec.split(","))
        w = synth.make_workload(N, D, A, H, B, seed=5, dynamics="contracting")
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        acts = torch.as_tensor(w.actions, device=eng.device)
        out_l = {"J": torch.empty(B, dtype=torch.float64, device=eng.device)}
        out_m = {"J": torch.empty(B, dtype=torch.float64, device=eng.device)}
        w_, r_, t_ = args.warmup, args.reps, args.trials
        ms_l, spread_l = time_calls(lambda: eng.rollout_linear(acts, w.mu0, w.S0, out=out_l), w_, r_, t_)
        ms_m, spread_m = time_calls(lambda: eng.rollout(acts, w.mu0, w.S0, out=out_m), w_, r_, t_)
        tf = 2.0 * D * B * H * float(N) * N / ms_l * 1e-9
        print(json.dumps({"N": N, "D": D, "A": A, "H": H, "B": B, "ms_linear": round(ms_l, 4),
                          "ms_linear_trials": [round(v, 4) for v in spread_l], "ms_rollout": round(ms_m, 4),
                          "ms_rollout_trials": [round(v, 4) for v in spread_m], "rollout_path": eng.last_rollout_path,
                          "ratio": round(ms_m / ms_l, 3), "tflops": round(tf, 2), "of_peak": round(tf / PEAK_TFLOPS, 3),
                          "J_finite": bool(torch.isfinite(out_l["J"]).all()), "build_id": eng.build_id}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
