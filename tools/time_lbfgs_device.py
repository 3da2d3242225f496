#!/usr/bin/env python3
"""Time one control step's candidate optimisation at the config-2 shape (N = 200, D = 3, A = 1, H = 25) through its three
gradient searches, on the same build and device, with the same starts (numpy seed 7, no warm start):
  scipy           candidate_optimizer = None: the sequential scipy L-BFGS-B restarts, one gpmpc_objective_grad_host per evaluation
  lbfgs           the same solver per restart in lockstep threads, one gpmpc_rollout_grad launch per round
  lbfgs_device    gpmpc_lbfgs_search: the loop on the device; `iterations` = the nfev scipy needed for the start -- with several
                  starts the LARGEST of their nfev: lockstep restarts all run the same number of iterations
with 1 start and with 16.  The arms ALTERNATE inside every round (after one unmeasured round), wall-clock around
_get_optimal_actions with a device synchronisation behind it; median over `--rounds`.  One JSON line per number of starts:
  ms_step         per control step's search, per arm (and every round's value)
  launches        objective + gradient LAUNCHES on the step's critical path (scipy: one per evaluation = the sum of nfev; lbfgs:
                  rounds, each serving every restart still running; lbfgs_device: iterations, each serving all restarts)
  ms_per_launch   ms_step / launches -- what one more evaluation on the critical path costs, host work included
  sequences       action sequences evaluated in all (scipy, lbfgs: the sum of nfev; lbfgs_device: starts x iterations, finished
                  restarts included), and ms_per_sequence = ms_step / sequences.  The arms do different amounts of work with 16
                  starts: compare ms_step, and the two per-unit figures only within their own meaning
  J               the final objective of each arm
`--trace-only` runs the lbfgs_device arm alone (`--rounds` times, 16 starts): the run to put under a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/time_lbfgs_device.py --trace-only) for lbfgs_step_kernel's time.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import gp_mpc_amd  # noqa: E402
from helpers import make_controller  # noqa: E402
from oracle import synth  # noqa: E402


def controller(w, eng, starts, optimizer, iterations=30):
    c = make_controller(w, optimize=True, restarts=starts, engine=eng, shard=False)
    cc = c.config.controller
    cc.candidate_optimizer, cc.init_from_previous_actions, cc.lbfgs_device_iterations = optimizer, False, iterations
    c._prepare()
    return c


def one_step(c, mu0, S0):
    np.random.seed(7)
    before = c.num_rollouts
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c._get_optimal_actions(mu0, S0)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    J, _ = c.compute_mean_lcb_trajectory(c.actions_mpc_previous_iter, mu0, S0)
    return ms, c.num_rollouts - before - 1, float(J)          # (compute_mean_lcb_trajectory counts one rollout itself)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", nargs="*", type=int, default=[1, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_lbfgs_device.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    w = synth.make_workload(200, 3, 1, 25, 2, seed=0)
    mu0, S0 = torch.as_tensor(w.mu0), torch.as_tensor(w.S0)
    if args.trace_only:
        c = controller(w, eng, 16, "lbfgs_device")
        for _ in range(args.rounds):
            one_step(c, mu0, S0)
        eng.close()
        return
    for starts in args.starts:
        seq = controller(w, eng, starts, None)
        one_step(seq, mu0, S0)                                    # unmeasured round
        np.random.seed(7)
        from scipy.optimize import minimize
        from gp_mpc_amd.control_objects.actions_mappers.action_init_functions import generate_mpc_action_init_random
        nfev = [minimize(fun=seq.compute_mean_lcb_trajectory, x0=generate_mpc_action_init_random(len_horizon=25, dim_action=1),
                         jac=True, args=(mu0, S0), method="L-BFGS-B", bounds=seq.actions_mapper.bounds,
                         options=seq.config.controller.actions_optimizer_params).nfev for _ in range(starts)]
        arms = {"scipy": seq, "lbfgs": controller(w, eng, starts, "lbfgs"),
                "lbfgs_device": controller(w, eng, starts, "lbfgs_device", iterations=max(nfev))}
        for c in arms.values():
            one_step(c, mu0, S0)
        ms = {k: [] for k in arms}
        launches, seqs, J = {}, {}, {}
        for _ in range(args.rounds):
            for k, c in arms.items():
                t, n_roll, J[k] = one_step(c, mu0, S0)
                ms[k].append(t)
                seqs[k] = n_roll - (0 if k == "scipy" else 1)      # (the batched arms evaluate their winner once more)
                launches[k] = n_roll if k == "scipy" else c.lbfgs_evaluations
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"N": 200, "D": 3, "A": 1, "H": 25, "starts": starts, "scipy_nfev": nfev,
                          "ms_step": {k: round(v, 3) for k, v in med.items()},
                          "ms_step_rounds": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                          "launches": launches, "ms_per_launch": {k: round(med[k] / max(launches[k], 1), 4) for k in med},
                          "sequences": seqs, "ms_per_sequence": {k: round(med[k] / max(seqs[k], 1), 4) for k in med},
                          "J": J, "build_id": eng.build_id}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
