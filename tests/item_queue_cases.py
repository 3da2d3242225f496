"""Runs of tests/test_gpu_item_queue_bits.py and of tools/gen_item_queue_golden.py (which pins their bits): the work queue of the
fused-horizon kernel's pairwise phase (the step's item list, the pull, an item's head and tail in csrc/rollout_kernel.h) where
few wavefronts meet many entries, where the list's length is 0, 1 and 2 modulo the number of wavefronts, where a step walks its
output pairs in several groups (the queue starts again per group), and in the cooperative form.  One function, so that the fixture
and the test can never disagree about the inputs.

A run = (N, D, candidates, force_path, threads, rows_per_chunk, cluster, lds_limit_kb, include_time, pair groups); H = 3, A = 1;
a run of fewer candidates than B takes the leading ones of the shape's workload, which is the one of tests/item_loop_cases.py
(with the time index as one more input dimension where include_time is set).  `pair groups` is what the launch has to report
(Engine.last_pair_groups): the run's LDS limit is there to reach it, and both neighbouring group sizes are 0.9 KiB or more away.

List lengths.  With force_path 1 and 2 nothing is separable, and a step of D = 3 in one group lists 3 wtri + 3 wpp + 3 entries
(wtri slots per diagonal pair, wpp per off-diagonal pair, three mean sums).  The planner's chunking (plan_rollout) gives
  N = 33,  256 threads:                       12-row chunks, wpp 1,  wtri 1:  9 entries  = 1 mod 4
  N = 130, 256 threads:                       44-row chunks, wpp 4,  wtri 3: 24 entries  = 0 mod 4
  N = 130, 256 threads, rows_per_chunk 32:    28-row chunks, wpp 6,  wtri 3: 30 entries  = 2 mod 4
  N = 130, rows_per_chunk 16 (any width):     16-row chunks, wpp 10, wtri 5: 48 entries  = 0 mod 4, 8 and 16
so four wavefronts take 2 to 12 entries each.  force_path 0 replaces off-diagonal pairs by their separable form where that is
the cheaper one (fewer entries, of another class); several groups split the list.
These lengths follow from plan_rollout's chunking as it is now and nothing here asserts them (the engine reports neither wpp nor
wtri): run_all asserts the kernel, the form and the pair groups only.  Whoever changes the chunking has to redo the table above,
or the 0 / 1 / 2 modulo corner goes quietly; the bits stay pinned either way."""
from oracle import synth

import item_loop_cases as loop_cases

H = loop_cases.H
B = loop_cases.B

SHAPES = [(33, 3), (130, 3)]


def _runs():
    runs = []
    # four wavefronts against many entries, every path: list lengths 1, 0 and 2 modulo 4
    for fp in (0, 1, 2):
        runs.append((33, 3, B, fp, 256, 0, 1, 0, 0, 1))
        runs.append((130, 3, B, fp, 256, 0, 1, 0, 0, 1))
        runs.append((130, 3, B, fp, 256, 32, 1, 0, 0, 1))
    # short chunks (many slots per pair) at every width
    for nt in (256, 512, 1024):
        for fp in (0, 1, 2):
            runs.append((130, 3, B, fp, nt, 16, 1, 0, 0, 1))
    # the step's pairs in several groups: at N = 130 48 KiB hold the records of 4 of the 6 pairs (44 KiB 2 beside the moments of
    # force_path 0), 32 KiB 2 (1) at 16-row chunks; N = 33: 16 KiB hold 1 pair beside the moments, 13 KiB 3 without them
    runs.append((130, 3, B, 0, 256, 0, 1, 44, 0, 3))
    runs.append((130, 3, B, 1, 256, 0, 1, 48, 0, 2))
    runs.append((130, 3, B, 2, 256, 0, 1, 48, 0, 2))
    runs.append((130, 3, B, 0, 1024, 16, 1, 32, 0, 6))
    runs.append((130, 3, B, 1, 1024, 16, 1, 32, 0, 3))
    runs.append((130, 3, B, 2, 1024, 16, 1, 32, 0, 3))
    runs.append((33, 3, B, 0, 256, 0, 1, 16, 0, 6))
    runs.append((33, 3, B, 2, 256, 0, 1, 13, 0, 2))
    # the time index as an input dimension
    for fp in (0, 2):
        runs.append((33, 3, B, fp, 256, 0, 1, 0, 1, 1))
        runs.append((130, 3, B, fp, 0, 16, 1, 0, 1, 1))
    # the cooperative form, one candidate (the plain run at its chunk length: 1024 threads, 16 rows, above)
    runs.append((130, 3, 1, 0, 0, 16, 2, 0, 0, 1))
    return runs


RUNS = _runs()
CASES = sorted({(r[0], r[1], r[8]) for r in RUNS})


def run_key(run):
    return "N%d_D%d_B%d_fp%d_nt%d_rpc%d_cl%d_lds%d_tm%d_g%d" % run


def make_case(N, D, tm):
    if not tm:
        return loop_cases.make_case(N, D)
    return synth.make_workload(N=N, D=D, A=1, H=H, B=B, include_time=True, seed=7000 + 10 * N + D, time0=3.0)


def apply_options(engine, fp, nt, rpc, cs, lds):
    loop_cases.apply_options(engine, fp, nt, rpc, cs)
    engine.set_option("lds_limit_kb", lds)


def reset_options(engine):
    loop_cases.reset_options(engine)
    engine.set_option("lds_limit_kb", 0)


def run_all(engine):
    """Every run of RUNS on `engine`: {key: {"mu", "Sig", "J"} as numpy arrays}; a case's model is prepared once, and every launch has to
    be the fused-horizon kernel's, in the form and with the number of pair groups the run names."""
    out = {}
    for case in CASES:
        N, D, tm = case
        w = make_case(N, D, tm)
        engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        engine.set_cost(w.target, w.W, w.W_T, w.kappa)
        try:
            for run in RUNS:
                if (run[0], run[1], run[8]) != case:
                    continue
                _, _, nB, fp, nt, rpc, cs, lds, _, groups = run
                apply_options(engine, fp, nt, rpc, cs, lds)
                o = engine.rollout(w.actions[:nB], w.mu0, w.S0, w.include_time, w.time0)
                assert engine.last_rollout_path == 0, (run, engine.last_rollout_path)         # the fused-horizon kernel
                assert engine.last_cluster == cs, (run, engine.last_cluster)
                assert engine.last_pair_groups == groups, (run, engine.last_pair_groups)
                out[run_key(run)] = {k: o[k].cpu().numpy().copy() for k in ("mu", "Sig", "J")}
        finally:
            reset_options(engine)
    return out
