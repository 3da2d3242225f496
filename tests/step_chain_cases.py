"""Runs of tests/test_gpu_step_chain_bits.py and of tools/gen_step_chain_golden.py (which pins their bits): the serial chain of a
horizon step of the fused-horizon kernel (csrc/rollout_kernel.h) -- the pair totals, M and V, the state update, the trajectory
store and the next step's small D x D algebra -- through every loop shape, state dimension, workgroup width and form of the
kernel.  One function, so that the fixture and the test can never disagree about the inputs.

A run = (N, D, H, candidates, force_path, threads, include_time, lds_limit_kb, cluster, rows_per_chunk, pair_tiles); A = 1; a run
of fewer candidates than B takes the leading ones of the shape's workload.  force_path 2 is Taylor without separable pairs (the
element-wise totals); lds_limit_kb > 0 leaves the row records of only some output pairs in LDS (several pair groups per step:
asserted); cluster > 1 is the cooperative form; pair_tiles 1 the batch-major path, whose per-candidate kernel runs one horizon
step per launch from the state stored in the trajectory (force_path 2: every candidate is handed to it)."""
from oracle import synth

B = 3


def _runs():
    runs = []
    # loop shape x state dimension: H = 1 (the first small algebra and the last tail only), 2 (one merged trip), 5 (several);
    # D = 1 (one pair, one mean problem), 2-4 (register solves), 6 (run-time D, elimination in LDS)
    for D in (1, 2, 3, 4, 6):
        for H in (1, 2, 5):
            runs.append((33, D, H, B, 0, 0, 0, 0, 1, 0, 0))
    # memory size: fewer points than a wavefront; more than one; both kinds of totals
    for N in (5, 70):
        for fp in (0, 2):
            runs.append((N, 3, 2, B, fp, 0, 0, 0, 1, 0, 0))
    runs.append((33, 4, 2, B, 2, 0, 0, 0, 1, 0, 0))
    runs.append((33, 6, 2, B, 2, 0, 0, 0, 1, 0, 0))
    # memories at which the separable form of an off-diagonal pair is the cheaper one (the kernel's own rule): the moment totals
    for D, fp in ((2, 0), (3, 0), (3, 2), (4, 0)):
        runs.append((130, D, 2, B, fp, 0, 0, 0, 1, 0, 0))
    # workgroup width
    for D in (3, 4):
        for nt in (256, 512, 1024):
            runs.append((33, D, 2, B, 0, nt, 0, 0, 1, 0, 0))
    # the time input: E = D + A + 1
    runs.append((33, 2, 2, B, 0, 0, 1, 0, 1, 0, 0))
    runs.append((33, 3, 5, B, 0, 0, 1, 0, 1, 0, 0))
    # several pair groups per step (the q0 loop): 24 / 32 KB hold 2-7 of the 10 (D = 4) and 2-6 of the 21 (D = 6) pairs
    for H in (1, 2, 5):
        runs.append((33, 4, H, B, 0, 0, 0, 24, 1, 0, 0))
    runs.append((33, 4, 2, B, 2, 0, 0, 24, 1, 0, 0))
    runs.append((33, 6, 2, B, 0, 0, 0, 32, 1, 0, 0))
    runs.append((33, 6, 5, B, 0, 0, 0, 32, 1, 0, 0))
    # the cooperative form at H = 1 and 2, and the plain kernel at its chunk length
    for H in (1, 2):
        runs.append((130, 3, H, B, 0, 0, 0, 0, 1, 16, 0))
        for cs in (2, 9):
            runs.append((130, 3, H, 1, 0, 0, 0, 0, cs, 16, 0))
    # the batch-major path: the per-candidate kernel takes one step at a time (a horizon slice of 1 < H) from the stored state
    runs.append((70, 3, 3, B, 2, 0, 0, 0, 1, 0, 1))
    runs.append((70, 4, 3, B, 2, 0, 0, 0, 1, 0, 1))
    return runs


RUNS = _runs()
MULTI_GROUP_RUNS = [r for r in RUNS if r[7] > 0]
COOP_PAIRS = [(r, (r[0], r[1], r[2], B, r[4], r[5], r[6], r[7], 1, r[9], r[10])) for r in RUNS if r[8] > 1]


def run_key(run):
    return "N%d_D%d_H%d_B%d_fp%d_nt%d_tm%d_lds%d_cl%d_rpc%d_pt%d" % run


def case_key(run):
    N, D, H, _, _, _, tm = run[:7]
    return (N, D, H, tm)


CASES = sorted({case_key(r) for r in RUNS})


def make_case(N, D, H, tm):
    return synth.make_workload(N=N, D=D, A=1, H=H, B=B, include_time=bool(tm), seed=9000 + 100 * N + 10 * D + H,
                               time0=3.0 if tm else 0.0)


OPTIONS = ("force_path", "threads", "lds_limit_kb", "cluster", "rows_per_chunk", "pair_tiles")


def reset_options(engine):
    for name in OPTIONS:
        engine.set_option(name, 0)


def run_all(engine):
    """Every run of RUNS on `engine`: {key: {"mu", "Sig", "J"} as numpy arrays and "groups", the pair groups per step}."""
    out = {}
    prepared = None
    try:
        for run in RUNS:
            N, D, H, nB, fp, nt, tm, lds, cs, rpc, pt = run
            if prepared != case_key(run):
                w = make_case(N, D, H, tm)
                engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
                engine.set_cost(w.target, w.W, w.W_T, w.kappa)
                prepared = case_key(run)
            for name, v in zip(OPTIONS, (fp, nt, lds, cs, rpc, pt)):
                engine.set_option(name, v)
            o = engine.rollout(w.actions[:nB], w.mu0, w.S0, w.include_time, w.time0)
            assert engine.last_rollout_path == (2 if pt == 1 else 0), (run, engine.last_rollout_path)
            assert engine.last_cluster == cs, (run, engine.last_cluster)
            res = {k: o[k].cpu().numpy().copy() for k in ("mu", "Sig", "J")}
            res["groups"] = engine.last_pair_groups
            out[run_key(run)] = res
    finally:
        reset_options(engine)
    return out
