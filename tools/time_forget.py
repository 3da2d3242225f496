#!/usr/bin/env python3
"""Time a sliding-window control step's model update: forget(oldest) + prepare(window + 1 appended point) -- a downdate and a
border update -- against the only alternative without gpmpc_forget, a full prepare of the same final window.  Both arms in one
process, alternating step by step on the same windows of one seeded workload, device events around each arm's calls (both end
in a stream synchronisation), after `warmup` steps; the median over `steps` steps.  One JSON line per shape:
  ms_forget, ms_border   the pair's two calls (their sum: ms_pair)
  ms_full                the full factorisation of the same memory (a second engine with "incremental" = 0)
  max_rel_iK             |iK(pair) - iK(full)| / max|iK(full)| after the last step (the result must not change)
Default shapes: N = 40, 200 and 1000 at D = 3, N = 4096 at D = 16.  Needs a GPU.
  python tools/time_forget.py [--shape N,D,A ...] [--steps 24] [--warmup 4]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_mpc_amd  # noqa: E402
from oracle import synth  # noqa: E402

DEFAULT = ["40,3,1", "200,3,1", "1000,3,1", "4096,16,4"]


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--steps", type=int, default=24)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_forget.py needs a GPU")
    for spec in args.shape:
        N, D, A = (int(v) for v in spec.split(","))
        total = args.warmup + args.steps
        w = synth.make_workload(N + total, D, A, 2, 1, seed=N)
        inc, full = gp_mpc_amd.HipEngine(0), gp_mpc_amd.HipEngine(0)
        inc.set_option("refresh_every", 10 ** 6)          # steady state: no refresh inside the timed window
        full.set_option("incremental", 0)
        dev = lambda a: torch.as_tensor(a, dtype=torch.float64, device=inc.device)   # noqa: E731
        X, Y, hyp = dev(w.X), dev(w.Y), (dev(w.lengthscales), dev(w.outputscales), dev(w.noises))
        inc.prepare(X[:N], Y[:N], *hyp)
        t_forget, t_border, t_full = [], [], []
        for s in range(total):
            Xs, Ys = X[s + 1:N + s + 1], Y[s + 1:N + s + 1]
            a = timed(lambda: inc.forget([0]))
            assert inc.last_prepare_mode == 3
            b = timed(lambda: inc.prepare(Xs, Ys, *hyp))
            assert inc.last_prepare_mode == 1
            c = timed(lambda: full.prepare(Xs, Ys, *hyp))
            assert full.last_prepare_mode == 0
            if s >= args.warmup:
                t_forget.append(a), t_border.append(b), t_full.append(c)
        iK, iKf = inc.factors()[0], full.factors()[0]
        err = float((iK - iKf).abs().max() / iKf.abs().max())
        med = statistics.median
        print(json.dumps({"N": N, "D": D, "E": D + A, "steps": args.steps, "ms_forget": round(med(t_forget), 4),
                          "ms_border": round(med(t_border), 4),
                          "ms_pair": round(med([p + q for p, q in zip(t_forget, t_border)]), 4),
                          "ms_full": round(med(t_full), 4), "ms_pair_min_max": [round(min(p + q for p, q in zip(t_forget, t_border)), 4),
                                                                               round(max(p + q for p, q in zip(t_forget, t_border)), 4)],
                          "ms_full_min_max": [round(min(t_full), 4), round(max(t_full), 4)],
                          "max_rel_iK": err, "build_id": inc.build_id}), flush=True)
        inc.close()
        full.close()


if __name__ == "__main__":
    main()
