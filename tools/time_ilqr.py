#!/usr/bin/env python3
"""Time gpmpc_ilqr_search (HipEngine.ilqr_search: 16 starts, 8 iterations, L = 8 step sizes) beside gpmpc_lbfgs_search with the
linearised propagation and 30 iterations on the same starts, on the same build and the same device, by the method of
tools/time_lqr_gains.py: device events around `reps` back-to-back calls after `warmup` calls, median of `trials` such windows.  The
memory is the action-driven one of tests/ilqr_cases.py (synth's dynamics barely feel the action).  One JSON line per shape:
  ms_ilqr / ms_lbfgs   per search call
  J_ilqr / J_lbfgs     the winners' LCB objective (gpmpc_rollout_linear's J)
  ms_per_iteration     ms_ilqr / iterations
  status               how many iLQR starts ended with status 0 / 1 / 2 / 3, and the accepted steps per start
Default shapes: config 2 (N = 200, D = 3, A = 1, H = 25) and config 4 (N = 1000, D = 4, A = 2, H = 30).  Needs a GPU.
  python tools/time_ilqr.py [--shape N,D,A,H ...] [--starts 16] [--iterations 8] [--steps 8] [--lbfgs-iterations 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_mpc_amd  # noqa: E402
import ilqr_cases as cases  # noqa: E402
from time_predict import time_calls  # noqa: E402

DEFAULT = ["200,3,1,25", "1000,4,2,30"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A,H")
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--lbfgs-iterations", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--reg", type=float, default=1e-3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ilqr.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        N, D, A, H = (int(v) for v in spec.split(","))
        B = args.starts
        w = cases.make_workload(N, D, A, H, B, seed=5, dense_s0=0.0)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        x0 = torch.as_tensor(w.actions, device=eng.device)
        st = eng.ilqr_state(B, H, A, args.steps)
        best_i = torch.empty(2 + H * A, dtype=torch.float64, device=eng.device)
        ilqr = lambda: eng.ilqr_search(st, w.mu0, w.S0, args.iterations, x0, reg0=args.reg, best_out=best_i)       # noqa: E731
        lst = eng.lbfgs_state(B, H * A, 10)
        best_l = torch.empty(2 + H * A, dtype=torch.float64, device=eng.device)
        x0f = x0.reshape(B, H * A)
        lbfgs = lambda: eng.lbfgs_search(lst, w.mu0, w.S0, H, A, args.lbfgs_iterations, x0=x0f,       # noqa: E731
                                         propagation="linearized", best_out=best_l)
        w_, r_, t_ = args.warmup, args.reps, args.trials
        ms_i, spread_i = time_calls(ilqr, w_, r_, t_)
        ms_l, spread_l = time_calls(lbfgs, w_, r_, t_)
        J0 = eng.rollout_linear(x0, w.mu0, w.S0, trajectories=False, stage_costs=False)["J"]
        status = st["status"].cpu().numpy().astype(int)
        print(json.dumps({"N": N, "D": D, "A": A, "H": H, "starts": B, "iterations": args.iterations, "L": args.steps,
                          "ms_ilqr": round(ms_i, 4), "ms_ilqr_trials": [round(v, 4) for v in spread_i],
                          "ms_per_iteration": round(ms_i / args.iterations, 4), "lbfgs_iterations": args.lbfgs_iterations,
                          "ms_lbfgs": round(ms_l, 4), "ms_lbfgs_trials": [round(v, 4) for v in spread_l],
                          "J_ilqr": float(best_i[0]), "J_lbfgs": float(best_l[0]), "J_best_start": float(J0.min()),
                          "status": np.bincount(status, minlength=4).tolist(),
                          "accepts": st["accepts"].cpu().numpy().astype(int).tolist(), "build_id": eng.build_id}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
