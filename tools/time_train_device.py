#!/usr/bin/env python3
"""Time the device hyper-parameter search and the batched training loss under it, at N = 200 (config 2), 64 and 256 with D = 3,
E = 4, on one device, the arms ALTERNATING inside every round (after one unmeasured round), median over `--rounds`:
  (a) mll_batch      gpmpc_mll_batch of R = 1, 16, 64 hyper-parameter sets per GP (device events around windows >= 0.5 s of
                     back-to-back calls) against R successive gpmpc_mll calls -- of `--parent-lib`, the library built from the
                     parent commit, where given, else of this build (gpmpc_mll is synchronous: its window is the same events
                     around the R calls, repeated)
  (b) train_search   HipEngine.train_search_host with R = 16 starts and 30 iterations (wall clock, its one synchronisation
                     included) against GpStateTransitionModel.train's host loop at its default iter_train = 15, and the whole
                     train() call of both optimizers (wall clock, the engine each call creates included)
  (c) prepare        config-2 gpmpc_prepare (full factorisation: option "incremental" = 0) of this build against `--parent-lib`:
                     the A/B that decides whether prepare_small_kernel may be built from the functions of csrc/small_factor.h
One JSON line per measurement.  Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import queue
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gp_mpc_amd  # noqa: E402
from gp_mpc_amd import _lib as L  # noqa: E402
from gp_mpc_amd.control_objects.models.gp_model import GpHyperParameters, GpStateTransitionModel, SavedState  # noqa: E402
from oracle import synth  # noqa: E402

WINDOW_S = 0.5


class OtherBuildEngine(gp_mpc_amd.HipEngine):
    """An engine on another build of the library (no ABI check: only entry points both builds have are called)."""

    def __init__(self, path, device=0):
        lib = C.CDLL(path)
        for name, (res, args) in L.SIGNATURES.items():
            if hasattr(lib, name):
                getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
        self.lib = lib
        self.device = torch.device("cuda", int(device))
        h = C.c_void_p()
        if lib.gpmpc_create(C.byref(h), self.device.index) != L.GPMPC_OK:
            raise RuntimeError(f"gpmpc_create failed in {path}")
        self._h, self._ogh_plans, self._cost = h, {}, None
        self.N = self.D = self.E = 0


def window(fn):
    """ms per call of fn over a window of >= WINDOW_S of back-to-back calls between two device events."""
    fn()
    torch.cuda.synchronize()
    reps, total = 1, 0.0
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        total = e0.elapsed_time(e1)
        if total >= WINDOW_S * 1e3:
            return total / reps
        reps = max(reps + 1, int(reps * 1.2 * WINDOW_S * 1e3 / max(total, 1e-3)))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(arms, rounds, measure):
    for fn in arms.values():
        measure(fn)                                                  # unmeasured round
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(measure(fn))
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}, {k: [round(x, 4) for x in v] for k, v in ms.items()}


def rows_of(w, R, seed):
    rng = np.random.default_rng(seed)
    D, E = w.lengthscales.shape
    base = np.concatenate([w.lengthscales, w.outputscales[:, None], w.noises[:, None]], axis=1)
    f = np.concatenate([rng.uniform(0.8, 1.25, size=(R, D, E + 1)), rng.uniform(2.0, 4.0, size=(R, D, 1))], axis=2)
    return base[None] * f


def saved_state(w):
    D, E = w.lengthscales.shape
    cons = {"min_lengthscale": np.full((D, E), 4e-3), "max_lengthscale": np.full((D, E), 25.0),
            "min_outputscale": np.full(D, 1e-3), "max_outputscale": np.full(D, 0.95),
            "min_std_noise": np.full(D, 1e-3), "max_std_noise": np.full(D, 3e-1)}
    st = SavedState(w.X, w.Y, [GpHyperParameters(w.lengthscales[a], w.outputscales[a], w.noises[a]).state_dict() for a in range(D)],
                    cons)
    st.to_arrays()
    lo = np.concatenate([cons["min_lengthscale"], cons["min_outputscale"][:, None], cons["min_std_noise"][:, None] ** 2], axis=1)
    hi = np.concatenate([cons["max_lengthscale"], cons["max_outputscale"][:, None], cons["max_std_noise"][:, None] ** 2], axis=1)
    return st, lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libgpmpc_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", nargs="*", type=int, default=[200, 64, 256])
    ap.add_argument("--skip", nargs="*", default=[], choices=["mll_batch", "train_search", "prepare"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_train_device.py needs a GPU")
    eng = gp_mpc_amd.HipEngine(0)
    old = OtherBuildEngine(args.parent_lib) if args.parent_lib else eng
    tag = dict(build_id=eng.build_id, parent_build_id=old.build_id, parent_lib=bool(args.parent_lib))
    dev = eng.device
    for N in args.sizes:
        w = synth.make_workload(N, 3, 1, 3, 2, seed=N)
        D, E = w.lengthscales.shape
        X, Y = torch.as_tensor(w.X, device=dev), torch.as_tensor(w.Y, device=dev)
        if "mll_batch" not in args.skip:
            for R in (1, 16, 64):
                th = torch.as_tensor(rows_of(w, R, N), device=dev)
                out = eng.mll_batch(X, Y, th)
                ls, osc, nz = th[:, :, :E].contiguous(), th[:, :, E].contiguous(), th[:, :, E + 1].contiguous()

                def batch():
                    eng.mll_batch(X, Y, th, out=out)

                def sequential():
                    for r in range(R):
                        old.mll(X, Y, ls[r], osc[r], nz[r])
                med, every = alternate({"mll_batch": batch, "sequential_mll": sequential}, args.rounds, window)
                print(json.dumps({"what": "mll_batch", "N": N, "D": D, "E": E, "R": R, "ms": med, "ms_rounds": every,
                                  "speedup": round(med["sequential_mll"] / med["mll_batch"], 2), **tag}), flush=True)
        if "train_search" not in args.skip:
            st, lo, hi = saved_state(w)
            R, iters = 16, 30
            x0 = np.random.default_rng(N).uniform(size=(R, D, E + 2))
            res = {}

            def device_search():
                res["device"] = eng.train_search_host(X, Y, x0, lo, hi, iters, history=10)

            def train_with(optimizer):
                def run():
                    q = queue.Queue()
                    torch.manual_seed(N)
                    GpStateTransitionModel.train(q, st, 7e-3, 15, 1e-3, optimizer=optimizer, restarts=R, device_iterations=iters)
                    res[optimizer] = q.get_nowait()
                return run
            med, every = alternate({"train_search_host": device_search, "train_lbfgs": train_with("lbfgs"),
                                    "train_lbfgs_device": train_with("lbfgs_device")}, args.rounds, wall)
            print(json.dumps({"what": "train_search", "N": N, "D": D, "E": E, "R": R, "iterations": iters, "iter_train": 15,
                              "ms": med, "ms_rounds": every, "device_loss": [float(v) for v in res["device"]["loss"]],
                              "mll_calls_of_the_host_loop": GpStateTransitionModel.last_training_launches, **tag}), flush=True)
    if "prepare" not in args.skip and args.parent_lib:
        w = synth.make_workload(200, 3, 1, 25, 2, seed=0)
        tens = [torch.as_tensor(v, device=dev) for v in (w.X, w.Y, w.lengthscales, w.outputscales, w.noises)]
        for e in (eng, old):
            e.set_option("incremental", 0)
        med, every = alternate({"this_build": lambda: eng.prepare(*tens), "parent": lambda: old.prepare(*tens)}, max(args.rounds, 5),
                               window)
        print(json.dumps({"what": "prepare", "N": 200, "D": 3, "E": 4, "ms": med, "ms_rounds": every,
                          "ratio": round(med["this_build"] / med["parent"], 4), **tag}), flush=True)
    if old is not eng:
        old.close()
    eng.close()


if __name__ == "__main__":
    main()
