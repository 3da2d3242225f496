#!/usr/bin/env python3
"""Time gpmpc_predict_cov (HipEngine.predict_cov) beside gpmpc_predict with variance for the same queries: device events around
`reps` back-to-back calls after `warmup` calls, median of `trials` such windows (tools/time_predict.py).  One JSON line per shape:
  ms_joint        per call of the joint form (D, M, M), symmetrisation included
  ms_cross        per call of the cross form of the M points with themselves (no symmetrisation pass)
  ms_predict      per gpmpc_predict call (mean + variance): the M N^2 half of the work
  ratio           ms_joint / ms_predict, beside ratio_expected = 1 + M / N from the operation count
  tflops          useful fp64 rate of the joint form, 2 D (M N^2 + M^2 N) flop per call
Default shapes: the model plot's 75 x 75 grid on a config-2 memory (M = 5625, N = 200, D = 3, E = 4), M = 4096 on a config-4
memory (N = 1000, D = 4, E = 6) and M = 1024 on a config-5 memory (N = 4096, D = 16, E = 20).  Needs a GPU.
  python tools/time_predict_cov.py [--shape M,N,D,E ...] [--reps 10] [--trials 5]
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

DEFAULT = ["5625,200,3,4", "4096,1000,4,6", "1024,4096,16,20"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="M,N,D,E")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trials", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_predict_cov.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        M, N, D, E = (int(v) for v in spec.split(","))
        w = synth.make_workload(N, D, E - D, 2, 1, seed=5)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        rng = np.random.default_rng(6)
        Xq = torch.as_tensor(rng.uniform(0.0, 1.0, size=(M, E)), device=eng.device)
        Xb = Xq.clone()
        w_, r_, t_ = args.warmup, args.reps, args.trials
        ms_j, spread = time_calls(lambda: eng.predict_cov(Xq, noises=w.noises), w_, r_, t_)
        ms_x, _ = time_calls(lambda: eng.predict_cov(Xq, Xb), w_, r_, t_)
        ms_p, _ = time_calls(lambda: eng.predict(Xq, noises=w.noises), w_, r_, t_)
        flop = 2.0 * D * (float(M) * N * N + float(M) * M * N)
        print(json.dumps({"M": M, "N": N, "D": D, "E": E, "ms_joint": round(ms_j, 4),
                          "ms_joint_trials": [round(v, 4) for v in spread], "ms_cross": round(ms_x, 4),
                          "ms_predict": round(ms_p, 4), "ratio": round(ms_j / ms_p, 3), "ratio_expected": round(1 + M / N, 3),
                          "tflops": round(flop / ms_j * 1e-9, 2), "build_id": eng.build_id}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
