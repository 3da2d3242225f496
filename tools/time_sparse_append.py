#!/usr/bin/env python3
"""Times gpmpc_sparse_append (HipEngine.sparse_append) beside gpmpc_prepare_sparse of the grown memory:
  (a) an append of 1 point;  (b) an append of 8 points in one call;  (c) gpmpc_prepare_sparse of the N + 1 points from scratch;
  (d) with --parent-lib: gpmpc_prepare_sparse of the N points by a library built from the parent commit and by this one, in child
      processes started alternately (parent, this, parent, this, ...), which shows what keeping the append's record costs.
Wall clock around synchronised calls: median [min, max] of 5 after 2 warm-ups.  Every measurement runs in a child process under its
own time limit, and nothing more is started after a child that failed.  One JSON line per measurement.  Needs a GPU.

    python tools/time_sparse_append.py [--shape N,D,A,M ...] [--reps 5] [--limit 240] [--parent-lib PATH] [--rounds 3]

Default shapes (those of DESIGN.md 4.4.2): N = 4096, D = 16, A = 4 (E = 20), M = 256 and N = 1000, D = 4, A = 2 (E = 6), M = 130.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = ["4096,16,4,256", "1000,4,2,130"]


def _clock(fn, reps, warm=2):
    import torch
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(np.min(t)), 4), "max_ms": round(float(np.max(t)), 4),
            "reps": len(t)}


def _workload(spec):
    from oracle import synth
    N, D, A, M = (int(v) for v in spec.split(","))
    w = synth.make_workload(N + 8, D, A, 2, 1, seed=0)           # the last 8 rows are the ones appended
    rows = [0] if M == 1 else [int(round(i * (N - 1) / (M - 1))) for i in range(M)]
    return N, D, A, M, w, rows


def one(spec, reps):
    """(a), (b), (c) on this build."""
    import torch
    import gp_mpc_amd
    N, D, A, M, w, rows = _workload(spec)
    eng = gp_mpc_amd.HipEngine(0)
    X, Y, ls, osc, nz = (torch.as_tensor(v, dtype=torch.float64, device=eng.device)
                         for v in (w.X, w.Y, w.lengthscales, w.outputscales, w.noises))
    Z = X[rows].contiguous()
    out = {"shape": {"N": N, "D": D, "E": D + A, "M": M}, "build_id": eng.build_id, "device": torch.cuda.get_device_name(0)}
    X1, Y1 = X[:N + 1].contiguous(), Y[:N + 1].contiguous()
    out["prepare_sparse_n_plus_1"] = _clock(lambda: eng.prepare_sparse(X1, Y1, Z, ls, osc, nz), reps)
    eng.prepare_sparse(X[:N], Y[:N], Z, ls, osc, nz)
    x1, y1, x8, y8 = X[N:N + 1].contiguous(), Y[N:N + 1].contiguous(), X[N:N + 8].contiguous(), Y[N:N + 8].contiguous()
    out["append_1"] = _clock(lambda: eng.sparse_append(x1, y1), reps)
    eng.prepare_sparse(X[:N], Y[:N], Z, ls, osc, nz)
    out["append_8"] = _clock(lambda: eng.sparse_append(x8, y8), reps)
    assert eng.last_prepare_mode == 5
    out["prepare_over_append_1"] = round(out["prepare_sparse_n_plus_1"]["median_ms"] / out["append_1"]["median_ms"], 2)
    eng.close()
    print(json.dumps(out), flush=True)


def prepare_only(spec, reps, lib_path, label):
    """(d): gpmpc_prepare_sparse of the N points through the library at lib_path, by the C ABI alone (the signatures of
    include/gpmpc.h that both builds share), so the same code measures both."""
    import torch
    N, D, A, M, w, rows = _workload(spec)
    lib = C.CDLL(lib_path)
    P, I, F = C.c_void_p, C.c_int, C.c_double
    lib.gpmpc_create.argtypes, lib.gpmpc_create.restype = [C.POINTER(P), I], I
    lib.gpmpc_destroy.argtypes, lib.gpmpc_destroy.restype = [P], I
    lib.gpmpc_build_id.argtypes, lib.gpmpc_build_id.restype = [], C.c_char_p
    lib.gpmpc_prepare_sparse.argtypes, lib.gpmpc_prepare_sparse.restype = [P, P, P, I, P, I, P, P, P, F, I, I, P], I
    dev = torch.device("cuda", 0)
    X, Y, ls, osc, nz = (torch.as_tensor(v, dtype=torch.float64, device=dev).contiguous()
                         for v in (w.X[:N], w.Y[:N], w.lengthscales, w.outputscales, w.noises))
    Z = X[rows].contiguous()
    h = P()
    assert lib.gpmpc_create(C.byref(h), 0) == 0
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():
        rc = lib.gpmpc_prepare_sparse(h, X.data_ptr(), Y.data_ptr(), N, Z.data_ptr(), M, ls.data_ptr(), osc.data_ptr(), nz.data_ptr(),
                                      1e-6, D, D + A, st)
        assert rc == 0, rc
    out = {"shape": {"N": N, "D": D, "E": D + A, "M": M}, "library": label, "build_id": lib.gpmpc_build_id().decode(),
           "prepare_sparse": _clock(call, reps)}
    lib.gpmpc_destroy(h)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A,M")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--parent-lib", help="libgpmpc_hip.so built from the parent commit: adds measurement (d)")
    ap.add_argument("--rounds", type=int, default=3, help="(d): alternations of parent and this build per shape")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    ap.add_argument("--prepare-only", nargs=3, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.reps)
    if args.prepare_only:
        return prepare_only(args.prepare_only[0], args.reps, args.prepare_only[1], args.prepare_only[2])

    def child(extra):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps)] + extra, timeout=args.limit).returncode
        if rc != 0:
            sys.exit(f"time_sparse_append.py: {' '.join(extra)} ended with status {rc}; nothing more is started")

    this_lib = os.path.join(ROOT, "data-efficient-reinforcement-learning-with-probabilistic-model-predictive-control_amd",
                            "libgpmpc_hip.so")
    for spec in args.shape:
        child(["--one", spec])
        if args.parent_lib:
            for _ in range(args.rounds):
                child(["--prepare-only", spec, os.path.abspath(args.parent_lib), "parent"])
                child(["--prepare-only", spec, this_lib, "this"])


if __name__ == "__main__":
    main()
