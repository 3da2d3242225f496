#!/usr/bin/env python3
"""Time gpmpc_rollout_linear_feedback_backward (HipEngine.rollout_linear_feedback_backward, per-candidate gains, J_bar = 1, every
output) beside gpmpc_rollout_linear_backward for the same candidates, on the same build and the same device, by the method of
tools/time_rollout_linear.py: device events around `reps` back-to-back calls after `warmup` calls, median of `trials` such
windows.  One JSON line per shape:
  ms_open_loop    per gpmpc_rollout_linear_backward call (J_bar = 1, actions_bar | mu0_bar | S0_bar)
  ms_feedback     per gpmpc_rollout_linear_feedback_backward call with (B, H, A, D) gains and gains_bar (the same tile launches;
                  the per-candidate kernels do the extra A x D work, the cost variances come from the closed-loop cost kernel)
  ms_shared       the same with one (H, A, D) gain sequence shared by the candidates
  ratio           ms_feedback / ms_open_loop
Default shapes: config 2 (N = 200, D = 3, H = 25, B = 256) and config 4 (N = 1000, D = 4, H = 30, B = 2048).  Needs a GPU.
  python tools/time_rollout_linear_feedback_backward.py [--shape N,D,A,H,B ...] [--reps 3] [--trials 3] [--open-loop-only]
(--open-loop-only: the first figure alone -- what a build without the closed-loop entry can be asked for.)
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

DEFAULT = ["200,3,1,25,256", "1000,4,2,30,2048"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A,H,B")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--open-loop-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_rollout_linear_feedback_backward.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        N, D, A, H, B = (int(v) for v in spec.split(","))
        w = synth.make_workload(N, D, A, H, B, seed=5, dynamics="contracting")
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        acts = torch.as_tensor(w.actions, device=eng.device)
        ones = torch.ones(B, dtype=torch.float64, device=eng.device)
        w_, r_, t_ = args.warmup, args.reps, args.trials
        res = {"N": N, "D": D, "A": A, "H": H, "B": B}
        ms_o, spread_o = time_calls(lambda: eng.rollout_linear_backward(acts, w.mu0, w.S0, J_bar=ones), w_, r_, t_)
        res.update(ms_open_loop=round(ms_o, 4), ms_open_loop_trials=[round(v, 4) for v in spread_o])
        if not args.open_loop_only:
            K = torch.as_tensor(0.3 * np.random.default_rng(6).standard_normal((B, H, A, D)), device=eng.device)
            Ks = K[0].contiguous()
            ms_f, spread_f = time_calls(lambda: eng.rollout_linear_feedback_backward(acts, K, w.mu0, w.S0, J_bar=ones), w_, r_, t_)
            ms_s, spread_s = time_calls(lambda: eng.rollout_linear_feedback_backward(acts, Ks, w.mu0, w.S0, J_bar=ones), w_, r_, t_)
            out = eng.rollout_linear_feedback_backward(acts, K, w.mu0, w.S0, J_bar=ones)
            res.update(ms_feedback=round(ms_f, 4), ms_feedback_trials=[round(v, 4) for v in spread_f], ms_shared=round(ms_s, 4),
                       ms_shared_trials=[round(v, 4) for v in spread_s], ratio=round(ms_f / ms_o, 3),
                       finite=bool(all(torch.isfinite(v).all() for v in out.values())))
        res["build_id"] = eng.build_id
        print(json.dumps(res), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
