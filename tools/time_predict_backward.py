#!/usr/bin/env python3
"""Time gpmpc_predict_backward (HipEngine.predict_backward) beside the forward gpmpc_predict: device events around `reps`
back-to-back calls after `warmup` calls, median of `trials` such windows.  One JSON line per shape:
  ms_backward            per backward call with both upstreams (mean_bar and var_bar)
  ms_backward_mean_only  per backward call with mean_bar alone (no matrix product)
  ms_forward             per forward call (mean + variance), measured in the same window of calls
  ms_forward_mean_only   per forward call without the variance
  ratio, ratio_mean_only backward over forward
  ms_moments_backward    the workaround this entry replaces: gpmpc_moments_backward at zero input variance with
                         M_bar = mean_bar and a diagonal S_bar = diag(var_bar), for all M points; it is timed on the first
                         `--moments-points` of them (moments_points) and scaled by M / moments_points (its cost is per point)
Default shapes: the model plot (M = 5625 = 75 x 75, N = 1500, D = 3, E = 4), a config-5 class shape (M = 1024, N = 4096,
D = 16, E = 20) and one query at N = 200 (latency), as tools/time_predict.py.  Needs a GPU.
  python tools/time_predict_backward.py [--shape M,N,D,E ...] [--reps 20] [--trials 5]
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
from time_predict import DEFAULT, time_calls  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="M,N,D,E")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--moments-points", type=int, default=64, help="points the (slow) moments_backward workaround is timed on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_predict_backward.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        M, N, D, E = (int(v) for v in spec.split(","))
        w = synth.make_workload(N, D, E - D, 2, 1, seed=5)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        rng = np.random.default_rng(6)
        Xq = torch.as_tensor(rng.uniform(0.0, 1.0, size=(M, E)), device=eng.device)
        mb = torch.as_tensor(rng.standard_normal((M, D)), device=eng.device)
        vb = torch.as_tensor(rng.standard_normal((M, D)), device=eng.device)
        Sb = torch.diag_embed(vb)
        w_, r_, t_ = args.warmup, args.reps, args.trials
        ms_b, spread = time_calls(lambda: eng.predict_backward(Xq, mb, vb), w_, r_, t_)
        ms_f, _ = time_calls(lambda: eng.predict(Xq, noises=w.noises), w_, r_, t_)
        ms_bm, _ = time_calls(lambda: eng.predict_backward(Xq, mb, None), w_, r_, t_)
        ms_fm, _ = time_calls(lambda: eng.predict(Xq, var=False), w_, r_, t_)
        P = min(M, args.moments_points)
        ms_mb, _ = time_calls(lambda: eng.moments_backward(Xq[:P], None, M_bar=mb[:P], S_bar=Sb[:P], var_bar=False), 1, 2, 3)
        ms_mb *= M / P
        print(json.dumps({"M": M, "N": N, "D": D, "E": E, "ms_backward": round(ms_b, 4),
                          "ms_backward_trials": [round(v, 4) for v in spread], "ms_backward_mean_only": round(ms_bm, 4),
                          "ms_forward": round(ms_f, 4), "ms_forward_mean_only": round(ms_fm, 4),
                          "ratio": round(ms_b / ms_f, 3), "ratio_mean_only": round(ms_bm / ms_fm, 3),
                          "ms_moments_backward": round(ms_mb, 4), "moments_points": P, "build_id": eng.build_id}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
