#!/usr/bin/env python3
"""Time gpmpc_rollout_feedback_backward (HipEngine.rollout_feedback_backward, per-candidate gains, J_bar = 1, gains_bar written,
no initial-state outputs: what rollout_feedback_grad adds to its forward) beside gpmpc_rollout_feedback with the same gains
(objective only) and gpmpc_rollout_backward for the same candidates (J_bar = 1), on the same build and the same device in one
run, by the method of tools/time_train_device.py: the arms ALTERNATE inside every round, after one unmeasured round; each
measurement is a window of >= 0.5 s of back-to-back calls between two device events; the median over `--rounds` is reported, with
every round beside it.  One JSON line per shape:
  ms.feedback_backward   per gpmpc_rollout_feedback_backward call (the forward recomputed inside: per horizon step the four
                         launches of gpmpc_moments and one step launch, then per reverse step the launches of
                         gpmpc_moments_backward and one wavefront-per-candidate launch)
  ms.feedback            per gpmpc_rollout_feedback call
  ms.rollout_backward    per gpmpc_rollout_backward call (open loop; the fused gradient kernels at these shapes)
  ratio_forward / ratio_open_loop_backward   ms.feedback_backward over the other two
Default shapes: config 2 (N = 200, D = 3, A = 1, H = 25) with B = 16 and B = 256.  Needs a GPU.
  python tools/time_rollout_feedback_backward.py [--shape N,D,A,H,B ...] [--rounds 3] [--out profiles/rollout_feedback_backward_timing.jsonl]
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
from time_train_device import alternate, window  # noqa: E402

DEFAULT = ["200,3,1,25,16", "200,3,1,25,256"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=DEFAULT, help="N,D,A,H,B")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_rollout_feedback_backward.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    for spec in args.shape:
        N, D, A, H, B = (int(v) for v in spec.split(","))
        w = synth.make_workload(N, D, A, H, B, seed=5, dynamics="contracting")
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        acts = torch.as_tensor(w.actions, device=eng.device)
        gains = torch.as_tensor(0.1 * np.random.default_rng(6).standard_normal((B, H, A, D)), device=eng.device)
        ones = torch.ones(B, dtype=torch.float64, device=eng.device)
        out = {"J": torch.empty(B, dtype=torch.float64, device=eng.device)}
        last = {}

        def feedback_backward():
            last["fb"] = eng.rollout_feedback_backward(acts, gains, w.mu0, w.S0, J_bar=ones, want_initial=False)

        def feedback():
            eng.rollout_feedback(acts, gains, w.mu0, w.S0, out=out)

        def rollout_backward():
            last["ol"] = eng.rollout_backward(acts, w.mu0, w.S0, J_bar=ones, want_initial=False)
        med, every = alternate({"feedback_backward": feedback_backward, "feedback": feedback, "rollout_backward": rollout_backward},
                               args.rounds, window)
        torch.cuda.synchronize()
        finite = all(bool(torch.isfinite(t).all()) for t in (last["fb"]["actions_bar"], last["fb"]["gains_bar"], out["J"]))
        line = json.dumps({"N": N, "D": D, "A": A, "H": H, "B": B, "ms": med, "ms_rounds": every,
                           "ratio_forward": round(med["feedback_backward"] / med["feedback"], 2),
                           "ratio_open_loop_backward": round(med["feedback_backward"] / med["rollout_backward"], 2),
                           "rounds": args.rounds, "window_s": 0.5, "finite": finite, "build_id": eng.build_id})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
