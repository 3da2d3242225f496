#!/usr/bin/env python3
"""Times gpmpc_select_inducing (HipEngine.select_inducing) beside gpmpc_prepare_sparse on the same inputs, and compares what the
chosen inducing inputs buy: max |J_sparse - J_exact| / max |J_exact| of gpmpc_rollout over B candidates with the greedy rows against
the strided rows ModelConfig.num_inducing_points picks by default (the strided figure is the one of 4.4.2).
Wall clock around synchronised calls: median [min, max] of 5 after 2 warm-ups.  Each shape runs in a child process under its own
time limit, and nothing more is started after a child that failed.  One JSON line per shape.  Needs a GPU.

    python tools/time_select_inducing.py [--shape N,D,A,H,B,M ...] [--reps 5] [--limit 240]

Default shapes: config 5 (N = 4096, D = 16, A = 4: E = 20, H = 50, B = 1024) with M = 256 and config 4 (N = 1000, D = 4, A = 2:
E = 6, H = 30, B = 1024) with M = 130.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = ["4096,16,4,50,1024,256", "1000,4,2,30,1024,130"]


def one(spec, reps, warm=2):
    import torch
    import gp_mpc_amd
    from gp_mpc_amd.control_objects.models.gp_model import inducing_rows
    from oracle import synth
    N, D, A, H, B, M = (int(v) for v in spec.split(","))
    w = synth.make_workload(N, D, A, H, B, seed=0)
    eng = gp_mpc_amd.HipEngine(0)
    eng.set_option("incremental", 0)
    X, Y, ls, osc, nz = (torch.as_tensor(v, dtype=torch.float64, device=eng.device)
                         for v in (w.X, w.Y, w.lengthscales, w.outputscales, w.noises))

    def clock(fn):
        for _ in range(warm):
            fn()
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(np.min(t)), 4),
                "max_ms": round(float(np.max(t)), 4), "reps": len(t)}

    out = {"shape": {"N": N, "D": D, "E": D + A, "H": H, "B": B, "M": M}, "build_id": eng.build_id,
           "device": torch.cuda.get_device_name(0)}
    sel = eng.select_inducing(X, M, ls, osc)
    Z_greedy = sel["Z"].clone()
    trace = sel["trace"].cpu().numpy()
    out["trace_first"], out["trace_last"] = float(trace[0]), float(trace[-1])
    Z_strided = X[inducing_rows(N, M)].contiguous()
    out["select_inducing"] = clock(lambda: eng.select_inducing(X, M, ls, osc))
    out["prepare_sparse"] = clock(lambda: eng.prepare_sparse(X, Y, Z_greedy, ls, osc, nz))
    out["ratio"] = round(out["select_inducing"]["median_ms"] / out["prepare_sparse"]["median_ms"], 2)
    # what the choice buys: the objective of B candidates on the sparse models against the exact one
    eng.set_cost(w.target, w.W, w.W_T, w.kappa)
    eng.prepare(X, Y, ls, osc, nz)
    J_exact = eng.rollout(w.actions, w.mu0, w.S0, trajectories=False)["J"].cpu().numpy()
    for name, Z in (("strided", Z_strided), ("greedy", Z_greedy)):
        eng.prepare_sparse(X, Y, Z, ls, osc, nz)
        J = eng.rollout(w.actions, w.mu0, w.S0, trajectories=False)["J"].cpu().numpy()
        out[f"J_{name}_vs_exact_max_rel"] = float(np.max(np.abs(J - J_exact)) / np.max(np.abs(J_exact)))
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A,H,B,M")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.reps)
    for spec in args.shape:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", spec, "--reps", str(args.reps)],
                            timeout=args.limit).returncode
        if rc != 0:
            sys.exit(f"time_select_inducing.py: shape {spec} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
