"""Batch-major pairwise pass (pair_tile_kernel.h) against the fused-horizon kernel and the CPU oracle, then timings.
  python tools/gpu_tiles_check.py [parity] [time] [name=value engine options ...]
parity: small shapes (ragged N, D = 1..4, time input, direct-exp path) -- tiled vs oracle and vs the fused kernel;
time:   config 4 (N = 1000, D = 4, H = 30, B = 2048) and config 3, HIP-event time per batch for both paths."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gp_mpc_amd
from oracle import synth, gpmpc_oracle as orc

args = sys.argv[1:]
opts = [a for a in args if "=" in a]
modes = [a for a in args if "=" not in a] or ["parity", "time"]
eng = gp_mpc_amd.HipEngine(0)
for kv in opts:
    eng.set_option(kv.split("=")[0], float(kv.split("=")[1]))


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def run(w, tiles, **o):
    eng.set_option("pair_tiles", tiles)
    for k, v in o.items():
        eng.set_option(k, v)
    out = eng.rollout(w.actions, w.mu0, w.S0, w.include_time, w.time0)
    path = eng.last_rollout_path
    for k in o:
        eng.set_option(k, 0)
    eng.set_option("pair_tiles", 0)
    return {k: v.cpu().numpy() for k, v in out.items()}, path


if "parity" in modes:
    bad = 0
    for (N, D, A, H, B, tm, s0, fp) in [(300, 4, 2, 4, 5, False, 1e-6, 0), (129, 4, 2, 3, 3, False, 1e-4, 0), (257, 3, 1, 4, 4, False, 1e-5, 0),
                                        (200, 2, 1, 5, 7, False, 1e-6, 0), (140, 1, 1, 4, 3, False, 1e-5, 0), (130, 3, 1, 3, 3, True, 1e-5, 0),
                                        (300, 4, 2, 3, 4, False, 3e-2, 0), (150, 4, 2, 3, 70, False, 1e-5, 0), (260, 4, 2, 3, 4, False, 1e-5, 1),
                                        (128, 2, 2, 3, 2, False, 1e-5, 0), (40, 3, 1, 3, 3, False, 1e-5, 0)]:
        w = synth.make_workload(N, D, A, H, B, include_time=tm, seed=N + D, s0=s0, time0=3.0 if tm else 0.0)
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        o = {"force_path": fp} if fp else {}
        t_out, p_t = run(w, 1, **o)
        f_out, p_f = run(w, 2, **o)
        f = orc.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        ref = orc.evaluate_candidates(f, w)
        e = dict(mu_o=rel(t_out["mu"], ref["mu"]), S_o=rel(t_out["Sig"], ref["Sig"]), J_o=rel(t_out["J"], ref["J"]),
                 mu_f=rel(t_out["mu"], f_out["mu"]), S_f=rel(t_out["Sig"], f_out["Sig"]), S_fo=rel(f_out["Sig"], ref["Sig"]))
        # covariances: two correct fp64 evaluations differ by the noise floor of the method (cond K); the tiled path has to be
        # as close to the oracle as the fused kernel is (factor 2) and close to the fused kernel itself
        ok = (p_t == 2 and p_f == 0 and e["mu_o"] < 1e-8 and e["S_o"] < max(2e-6, 2 * e["S_fo"]) and e["S_f"] < max(2e-6, e["S_fo"])
              and e["J_o"] < 1e-6)
        bad += not ok
        print(f"N={N} D={D} A={A} H={H} B={B} time={int(tm)} s0={s0:g} force_path={fp}: paths {p_t}/{p_f} "
              + " ".join(f"{k}={v:.1e}" for k, v in e.items()) + ("  OK" if ok else "  FAIL"), flush=True)
    # independence of the batch: candidates 3.. of a batch of 40 alone
    w = synth.make_workload(300, 4, 2, 3, 40, seed=5, s0=1e-5)
    eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    eng.set_cost(w.target, w.W, w.W_T, w.kappa)
    full, _ = run(w, 1)
    w2 = synth.make_workload(300, 4, 2, 3, 40, seed=5, s0=1e-5)
    w2.actions = w.actions[3:20].copy()
    sub, _ = run(w2, 1)
    same = np.array_equal(full["Sig"][3:20], sub["Sig"]) and np.array_equal(full["J"][3:20], sub["J"])
    again, _ = run(w, 1)
    rep = np.array_equal(full["Sig"], again["Sig"])
    print("bitwise: sub-batch", same, "repeat", rep, flush=True)
    bad += (not same) + (not rep)
    print("PARITY", "OK" if bad == 0 else f"FAILED ({bad})", flush=True)

if "time" in modes or "c4" in modes:
    for name, B in ([("c4", 2048)] if "c4" in modes else [("c4", 2048), ("c4", 512), ("c3", 1024), ("c2", 2048)]):
        w = synth.named(name, B=B)
        N, D, A, E, H, _ = w.dims
        eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        res = {}
        for tiles in (2, 1):
            eng.set_option("pair_tiles", tiles)
            eng.rollout_timed(w.actions, w.mu0, w.S0, 1)
            ms, J = eng.rollout_timed(w.actions, w.mu0, w.S0, 3 if name == "c4" else 10)
            res[tiles] = (ms, J.cpu().numpy(), eng.last_rollout_path)
        eng.set_option("pair_tiles", 0)
        dj = rel(res[1][1], res[2][1])
        print(f"{name} N={N} D={D} H={H} B={B}: fused {res[2][0]:.2f} ms (path {res[2][2]}), tiled {res[1][0]:.2f} ms (path {res[1][2]}) "
              f"= {B / res[1][0] * 1e3:.0f} rollouts/s; |dJ| {dj:.1e}", flush=True)
eng.close()
