#!/usr/bin/env python3
"""Times gpmpc_sparse_forget (HipEngine.sparse_forget) beside the rebuild it replaces in a sliding window:
  (a) a forget of 1 point (the call synchronises);
  (b) a sliding step: forget the oldest point + append a new one + synchronise;
  (c) gpmpc_prepare_sparse of the window of N points from scratch -- the call the step replaces (code this feature does not touch).
Every repetition of (a) and (b) removes a different row that really is in the model (rows 0, 1, 2, ... of the memory) and (b) appends
a different new row.  Wall clock around synchronised calls: median [min, max] of 5 after 2 warm-ups.  Every shape runs in a child
process under its own time limit, and nothing more is started after a child that failed.  One JSON line per shape.  Needs a GPU.

    python tools/time_sparse_forget.py [--shape N,D,A,M ...] [--reps 5] [--limit 240]

Default shapes (those of DESIGN.md 4.4.2): N = 4096, D = 16, A = 4 (E = 20), M = 256 and N = 1000, D = 4, A = 2 (E = 6), M = 130.
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

DEFAULT = ["4096,16,4,256", "1000,4,2,130"]
WARM = 2


def _clock(fn, reps, warm=WARM):
    """fn(i) for i = 0 .. warm + reps - 1; the first `warm` calls are not timed."""
    import torch
    t = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        if i >= warm:
            t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(np.min(t)), 4), "max_ms": round(float(np.max(t)), 4),
            "reps": len(t)}


def one(spec, reps):
    import torch
    import gp_mpc_amd
    from oracle import synth
    N, D, A, M = (int(v) for v in spec.split(","))
    n_calls = WARM + reps
    w = synth.make_workload(N + n_calls, D, A, 2, 1, seed=0)     # the last rows are the ones a sliding step appends
    rows = [0] if M == 1 else [int(round(i * (N - 1) / (M - 1))) for i in range(M)]
    eng = gp_mpc_amd.HipEngine(0)
    X, Y, ls, osc, nz = (torch.as_tensor(v, dtype=torch.float64, device=eng.device)
                         for v in (w.X, w.Y, w.lengthscales, w.outputscales, w.noises))
    Z = X[rows].contiguous()
    XN, YN = X[:N].contiguous(), Y[:N].contiguous()
    row = [(X[i:i + 1].contiguous(), Y[i:i + 1].contiguous()) for i in list(range(n_calls)) + list(range(N, N + n_calls))]
    out = {"shape": {"N": N, "D": D, "E": D + A, "M": M}, "build_id": eng.build_id, "device": torch.cuda.get_device_name(0)}
    out["prepare_sparse_window"] = _clock(lambda i: eng.prepare_sparse(XN, YN, Z, ls, osc, nz), reps)
    out["forget_1"] = _clock(lambda i: eng.sparse_forget(*row[i]), reps)
    assert eng.last_prepare_mode == 6
    eng.prepare_sparse(XN, YN, Z, ls, osc, nz)

    def step(i):
        eng.sparse_forget(*row[i])
        eng.sparse_append(*row[n_calls + i])
    out["sliding_step"] = _clock(step, reps)
    assert eng.last_prepare_mode == 5
    out["prepare_over_step"] = round(out["prepare_sparse_window"]["median_ms"] / out["sliding_step"]["median_ms"], 2)
    out["ranges_apart"] = out["sliding_step"]["max_ms"] < out["prepare_sparse_window"]["min_ms"]
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A,M")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.reps)
    for spec in args.shape:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--one", spec],
                            timeout=args.limit).returncode
        if rc != 0:
            sys.exit(f"time_sparse_forget.py: --one {spec} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
