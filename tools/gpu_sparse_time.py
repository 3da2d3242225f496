"""Times gpmpc_prepare_sparse against gpmpc_prepare on the same memory, and gpmpc_rollout on the sparse model against the exact
one, on one GPU.  Defaults are config 5's shape: N = 4096, D = 16, A = 4 (E = 20), H = 50, B = 1024 per GPU, with
M = 256 inducing inputs (the strided rows ModelConfig.num_inducing_points picks).  Both calls synchronise their stream, so wall
clock around them is the call's time; the rollouts are timed by gpmpc_rollout_timed (HIP events).  One JSON line on stdout.

    python tools/gpu_sparse_time.py [--N 4096 --D 16 --A 4 --H 50 --B 1024 --M 256 --exact-B 1024 --reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("N", 4096), ("D", 16), ("A", 4), ("H", 50), ("B", 1024), ("M", 256), ("reps", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--exact-B", type=int, default=1024, help="candidates of the exact model's rollout (0: skip it)")
    args = ap.parse_args()
    import torch
    import gp_mpc_amd
    from gp_mpc_amd.control_objects.models.gp_model import inducing_rows
    from oracle import synth
    w = synth.make_workload(args.N, args.D, args.A, args.H, args.B, seed=0)
    eng = gp_mpc_amd.HipEngine(0)
    eng.set_option("incremental", 0)                       # every gpmpc_prepare below is a full factorisation
    dev = [torch.as_tensor(v, dtype=torch.float64, device=eng.device) for v in (w.X, w.Y, w.lengthscales, w.outputscales, w.noises)]
    X, Y, ls, osc, nz = dev
    Z = X[inducing_rows(args.N, args.M)].contiguous()

    def clock(fn, warm=2):
        for _ in range(warm):
            fn()
        t = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t)), "reps": len(t)}

    out = {"shape": {k: getattr(args, k) for k in ("N", "D", "A", "H", "B", "M")}, "build_id": eng.build_id,
           "device": torch.cuda.get_device_name(0)}
    out["prepare_exact"] = clock(lambda: eng.prepare(X, Y, ls, osc, nz))
    assert eng.last_prepare_mode == 0
    eng.set_cost(w.target, w.W, w.W_T, w.kappa)
    if args.exact_B > 0:
        eng.rollout_timed(w.actions[:2], w.mu0, w.S0, 1)
        ms, J_exact = eng.rollout_timed(w.actions[:args.exact_B], w.mu0, w.S0, 1)
        out["rollout_exact"] = {"ms": ms, "B": args.exact_B, "reps": 1}
    out["prepare_sparse"] = clock(lambda: eng.prepare_sparse(X, Y, Z, ls, osc, nz))
    assert eng.last_prepare_mode == 4
    eng.rollout_timed(w.actions, w.mu0, w.S0, 1)
    ms, J_sparse = eng.rollout_timed(w.actions, w.mu0, w.S0, args.reps)
    out["rollout_sparse"] = {"ms": ms, "B": args.B, "reps": args.reps}
    if args.exact_B > 0:
        n = min(args.exact_B, args.B)
        a, b = J_exact[:n].cpu().numpy(), J_sparse[:n].cpu().numpy()
        out["J_sparse_vs_exact_max_rel"] = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
