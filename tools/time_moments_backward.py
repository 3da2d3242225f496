#!/usr/bin/env python3
"""Time gpmpc_moments_backward (HipEngine.moments_backward) the way tools/time_moments.py times the forward: device events around
`reps` back-to-back calls after `warmup` calls, median of `trials` windows.  One JSON line per shape:
  ms                    per call with all of M_bar, S_bar, V_bar (both outputs)
  ms_without_S          per call with M_bar and V_bar only (no pairwise pass)
  ms_forward            gpmpc_moments with S and V at the same inputs, for the ratio
  gflops                useful fp64 work per second of the full call: per point, the pair pass's elements (as the forward
                        counts them) at 4 E + 16 flops each (the E-long dot product, the exponent's sums, one exp counted as
                        12, the weighting, the row / column sums and the E-long Y_i accumulation), plus the per-point pass's
                        D N (E^2 + 3 E (E + 1) + 4 E + 16) (C^-1 u, the two weighted second moments, the sums)
  frac_fp64_peak        gflops over the 78.6 TF fp64 peak DESIGN.md uses
Shapes: those of time_moments.py.  Needs a GPU.
  python tools/time_moments_backward.py [--shape P,N,D,E,kind ...] [--reps 20] [--trials 5]
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
from time_moments import DEFAULT, PEAK_FP64, inputs, time_calls  # noqa: E402


def flops(P, N, D, E):
    pairs = D * (N * N + N) / 2 + D * (D - 1) / 2 * N * N
    return P * (pairs * (4 * E + 16) + D * N * (E * E + 3 * E * (E + 1) + 4 * E + 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="P,N,D,E,kind")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_moments_backward.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        P, N, D, E, kind = spec.split(",")
        P, N, D, E = int(P), int(N), int(D), int(E)
        w = synth.make_workload(N, D, E - D, 2, 1, seed=5)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        mu, var = inputs(w, P, kind, seed=6)
        rng = np.random.default_rng(8)
        mu_d, var_d = eng._dev(mu), eng._dev(var)
        Mb, Sb, Vb = (eng._dev(rng.standard_normal(s)) for s in ((P, D), (P, D, D), (P, E, D)))
        reps = args.reps if P * N * N * D * D < 1e11 else max(2, args.reps // 10)
        ms, spread = time_calls(lambda: eng.moments_backward(mu_d, var_d, Mb, Sb, Vb), args.warmup, reps, args.trials)
        ms_mv, _ = time_calls(lambda: eng.moments_backward(mu_d, var_d, Mb, None, Vb), args.warmup, reps, args.trials)
        ms_f, _ = time_calls(lambda: eng.moments(mu_d, var_d), args.warmup, reps, args.trials)
        gflops = flops(P, N, D, E) / (ms * 1e-3) / 1e9
        print(json.dumps({"P": P, "N": N, "D": D, "E": E, "sigma": kind, "ms": round(ms, 4),
                          "ms_trials": [round(v, 4) for v in spread], "ms_without_S": round(ms_mv, 4),
                          "ms_forward": round(ms_f, 4), "ratio_to_forward": round(ms / ms_f, 2),
                          "gflops": round(gflops, 1), "frac_fp64_peak": round(gflops * 1e9 / PEAK_FP64, 3),
                          "build_id": eng.build_id}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
