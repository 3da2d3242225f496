#!/usr/bin/env python3
"""Time gpmpc_moments (HipEngine.moments): device events around `reps` back-to-back calls after `warmup` calls, median of
`trials` such windows.  One JSON line per shape:
  ms                    per call (M, S and V)
  points_per_s          P / ms
  gflops                useful fp64 work per second over the measured time: per point, the pair pass's elements
                        (D (N^2 + N) / 2 diagonal + D (D - 1) / 2 N^2 off-diagonal) at 2 E + 16 flops each (the E-long dot
                        product, the exponent's sums, one exp counted as 12, the weighted accumulation), plus the per-point
                        pass's D N (E^2 + 4 E + 16)
  frac_fp64_peak        gflops over the 78.6 TF fp64 peak DESIGN.md uses
Shapes ("P,N,D,E,kind", kind full = dense Sigma over all E inputs, state = Sigma in the state block only): P = 4096, N = 200,
D = 3, E = 4 in both kinds (printed beside the config-2 rollout's candidate-steps per second from the same run), P = 1024,
N = 1000, D = 4, E = 6, P = 64, N = 4096, D = 16, E = 20 and P = 1 at N = 200 (latency).  Needs a GPU.
  python tools/time_moments.py [--shape P,N,D,E,kind ...] [--reps 20] [--trials 5]
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

PEAK_FP64 = 78.6e12
DEFAULT = ["4096,200,3,4,full", "4096,200,3,4,state", "1024,1000,4,6,full", "64,4096,16,20,full", "1,200,3,4,full"]


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


def inputs(w, P, kind, seed):
    rng = np.random.default_rng(seed)
    N, E = w.X.shape
    D = w.Y.shape[1]
    lo, hi = w.X.min(axis=0), w.X.max(axis=0)
    mu = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(P, E))
    ls = w.lengthscales.min(axis=0)
    n = E if kind == "full" else D
    G = rng.standard_normal((P, n, n)) * (0.3 * ls[:n])[None, :, None]
    var = np.zeros((P, E, E))
    var[:, :n, :n] = G @ G.transpose(0, 2, 1) + 1e-6 * np.diag(ls[:n] ** 2)[None]
    return mu, var


def flops(P, N, D, E):
    pairs = D * (N * N + N) / 2 + D * (D - 1) / 2 * N * N
    return P * (pairs * (2 * E + 16) + D * N * (E * E + 4 * E + 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="P,N,D,E,kind")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_moments.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    rollout_rate = None
    for spec in args.shape:
        P, N, D, E, kind = spec.split(",")
        P, N, D, E = int(P), int(N), int(D), int(E)
        w = synth.make_workload(N, D, E - D, 2, 1, seed=5)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        mu, var = inputs(w, P, kind, seed=6)
        mu_d, var_d = eng._dev(mu), eng._dev(var)
        reps = args.reps if P * N * N * D * D < 1e11 else max(2, args.reps // 10)
        ms, spread = time_calls(lambda: eng.moments(mu_d, var_d), args.warmup, reps, args.trials)
        ms_mv, _ = time_calls(lambda: eng.moments(mu_d, var_d, S=False), args.warmup, reps, args.trials)
        gflops = flops(P, N, D, E) / (ms * 1e-3) / 1e9
        rec = {"P": P, "N": N, "D": D, "E": E, "sigma": kind, "ms": round(ms, 4), "ms_trials": [round(v, 4) for v in spread],
               "ms_without_S": round(ms_mv, 4), "points_per_s": round(P / (ms * 1e-3), 1), "gflops": round(gflops, 1),
               "frac_fp64_peak": round(gflops * 1e9 / PEAK_FP64, 3), "build_id": eng.build_id}
        if (N, D, E) == (200, 3, 4) and P > 1:
            if rollout_rate is None:     # config 2 of bench.py: B = 256 candidates, H = 25 steps
                c = synth.make_workload(200, 3, 1, 25, 256, seed=7)
                eng.prepare(c.X, c.Y, c.lengthscales, c.outputscales, c.noises)
                eng.set_cost(c.target, c.W, c.W_T, c.kappa)
                acts = eng._dev(c.actions)
                ms_r, _ = time_calls(lambda: eng.rollout(acts, c.mu0, c.S0, trajectories=False, stage_costs=False),
                                     args.warmup, 10, args.trials)
                rollout_rate = 256 * 25 / (ms_r * 1e-3)
            rec["rollout_candidate_steps_per_s"] = round(rollout_rate, 1)
        print(json.dumps(rec), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
