#!/usr/bin/env python3
"""Time gpmpc_predict (HipEngine.predict): device events around `reps` back-to-back calls after `warmup` calls, median of
`trials` such windows.  One JSON line per shape:
  ms                   per call (mean + variance)
  ms_mean_only         per call without the variance (no matrix product)
  gflops               useful fp64 work per second: 2 M N^2 D (the variance's products) + M N D (3 E + 4) (building K*
                       and the mean's dot products) over the measured time
  frac_fp64_matrix_peak  gflops over the 78.6 TF fp64 matrix peak DESIGN.md uses
Default shapes: the model plot (M = 5625 = 75 x 75, N = 1500, D = 3, E = 4), a config-5 class shape (M = 1024, N = 4096,
D = 16, E = 20) and one query at N = 200 (latency).  Needs a GPU.
  python tools/time_predict.py [--shape M,N,D,E ...] [--reps 20] [--trials 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_mpc_amd  # noqa: E402
from oracle import synth  # noqa: E402

PEAK_FP64_MATRIX = 78.6e12
DEFAULT = ["5625,1500,3,4", "1024,4096,16,20", "1,200,3,4"]


def time_calls(fn, warmup, reps, trials):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(trials):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        per_call.append(t0.elapsed_time(t1) / reps)
    return statistics.median(per_call), per_call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="M,N,D,E")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_predict.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        M, N, D, E = (int(v) for v in spec.split(","))
        w = synth.make_workload(N, D, E - D, 2, 1, seed=5)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        Xq = torch.as_tensor(np.random.default_rng(6).uniform(0.0, 1.0, size=(M, E)), device=eng.device)
        ms, spread = time_calls(lambda: eng.predict(Xq, noises=w.noises), args.warmup, args.reps, args.trials)
        ms_mean, _ = time_calls(lambda: eng.predict(Xq, var=False), args.warmup, args.reps, args.trials)
        flop = 2.0 * M * N * N * D + M * N * D * (3.0 * E + 4.0)
        gflops = flop / (ms * 1e-3) / 1e9
        print(json.dumps({"M": M, "N": N, "D": D, "E": E, "ms": round(ms, 4), "ms_trials": [round(v, 4) for v in spread],
                          "ms_mean_only": round(ms_mean, 4), "gflops": round(gflops, 1),
                          "frac_fp64_matrix_peak": round(gflops * 1e9 / PEAK_FP64_MATRIX, 3),
                          "build_id": eng.build_id}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
