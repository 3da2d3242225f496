"""Runs of tests/test_gpu_short_item_bits.py and of tools/gen_short_item_golden.py (which pins their bits): the SHORT items of the
fused-horizon kernel's pairwise work queue at three state dimensions -- the separable (side, band) items (sep3_item<3 ... 6> of
csrc/rollout_kernel.h) and the mean sums -- and the per-point pass that feeds them, with X^T read from LDS and from global memory.
One function, so that the fixture and the test can never disagree about the inputs.

A run = (N, candidates, threads, rows_per_chunk, cluster, lds_limit_kb, include_time, S0 index, pair groups); D = 3, H = 3, A = 1,
force_path 0 and force_separable 1 (every off-diagonal pair whose Taylor degree is 1 ... 6 takes the separable form, whatever the cost
model says: at these N it would rarely choose it).  A run of fewer candidates than B takes the leading ones of its workload.

Which sep3_item<KS> runs.  KS = max(3, Taylor degree), and the degree grows with the state covariance, so the workloads differ in the
initial covariance S0 = s0 I, s0 = S0_VALUES[index].  degrees_of() restates the kernel's degree selection on the numpy oracle's
trajectory (tests/hetero_cases.taylor_degrees, as tests/test_hetero_reference.py does); tests/test_short_item_cases.py asserts that
every KS = 3, 4, 5, 6 is met by an off-diagonal pair in some step of some run, and that no run is without a separable pair.

N: 33 one partial point trip of 64 lanes; 64 exactly one full trip; 65 a second trip with one lane; 130 three trips, the last with
two lanes.  256 threads: four wavefronts take several short items each (the claim of the next entry under an item's reduction);
1024: sixteen.

Where X^T lives.  The engine does not report RolloutPlan::x_in_lds, so the (shape, lds_limit_kb) of the runs were put through
plan_rollout by a stand-alone host program (tools/rollout_plan_probe.hip, which needs no GPU); PROBE_OUTPUT below is what it printed
(G = pairs per group of the 6, groups = ceil(6 / G)).  The planner prefers all pairs in one group over the X^T copy, so every run
of several groups reads X^T from global memory, every run without an LDS limit reads the LDS copy, and 90 KiB at N = 130 hold all
pairs in one group but not the copy beside them; run_all asserts what the engine can report (the pair groups)."""
from oracle import synth

H = 3
B = 8
D = 3
S0_VALUES = (1e-6, 1e-3, 4e-3)

PROBE_OUTPUT = """\
  N=33 E=4 B=8 threads=256 rows_per_chunk=0 cluster=1 lds_kb=0 -> rc=0 path=0 nt=256 G=6 groups=1 CH=12 x_in_lds=1 cluster=1 lds_bytes=44304
  N=33 E=4 B=8 threads=1024 rows_per_chunk=0 cluster=1 lds_kb=0 -> rc=0 path=0 nt=1024 G=6 groups=1 CH=12 x_in_lds=1 cluster=1 lds_bytes=44304
  N=33 E=4 B=8 threads=256 rows_per_chunk=0 cluster=1 lds_kb=16 -> rc=0 path=0 nt=256 G=1 groups=6 CH=12 x_in_lds=0 cluster=1 lds_bytes=12640
  N=64 E=4 B=8 threads=256 rows_per_chunk=0 cluster=1 lds_kb=0 -> rc=0 path=0 nt=256 G=6 groups=1 CH=16 x_in_lds=1 cluster=1 lds_bytes=58688
  N=64 E=4 B=8 threads=1024 rows_per_chunk=0 cluster=1 lds_kb=0 -> rc=0 path=0 nt=1024 G=6 groups=1 CH=16 x_in_lds=1 cluster=1 lds_bytes=58688
  N=65 E=4 B=8 threads=256 rows_per_chunk=0 cluster=1 lds_kb=0 -> rc=0 path=0 nt=256 G=6 groups=1 CH=16 x_in_lds=1 cluster=1 lds_bytes=59488
  N=65 E=4 B=8 threads=1024 rows_per_chunk=0 cluster=1 lds_kb=0 -> rc=0 path=0 nt=1024 G=6 groups=1 CH=16 x_in_lds=1 cluster=1 lds_bytes=59488
  N=65 E=4 B=8 threads=256 rows_per_chunk=0 cluster=1 lds_kb=28 -> rc=0 path=0 nt=256 G=2 groups=3 CH=16 x_in_lds=0 cluster=1 lds_bytes=24848
  N=130 E=4 B=8 threads=256 rows_per_chunk=0 cluster=1 lds_kb=0 -> rc=0 path=0 nt=256 G=6 groups=1 CH=44 x_in_lds=1 cluster=1 lds_bytes=94960
  N=130 E=4 B=8 threads=1024 rows_per_chunk=0 cluster=1 lds_kb=0 -> rc=0 path=0 nt=1024 G=6 groups=1 CH=16 x_in_lds=1 cluster=1 lds_bytes=89040
  N=130 E=4 B=8 threads=256 rows_per_chunk=0 cluster=1 lds_kb=44 -> rc=0 path=0 nt=256 G=2 groups=3 CH=20 x_in_lds=0 cluster=1 lds_bytes=37104
  N=130 E=4 B=8 threads=1024 rows_per_chunk=0 cluster=1 lds_kb=44 -> rc=0 path=0 nt=1024 G=2 groups=3 CH=16 x_in_lds=0 cluster=1 lds_bytes=37312
  N=130 E=4 B=8 threads=256 rows_per_chunk=0 cluster=1 lds_kb=90 -> rc=0 path=0 nt=256 G=6 groups=1 CH=44 x_in_lds=0 cluster=1 lds_bytes=90800
  N=33 E=5 B=8 threads=256 rows_per_chunk=0 cluster=1 lds_kb=0 -> rc=0 path=0 nt=256 G=6 groups=1 CH=12 x_in_lds=1 cluster=1 lds_bytes=44640
  N=130 E=5 B=8 threads=256 rows_per_chunk=0 cluster=1 lds_kb=0 -> rc=0 path=0 nt=256 G=6 groups=1 CH=44 x_in_lds=1 cluster=1 lds_bytes=96064
  N=130 E=4 B=8 threads=1024 rows_per_chunk=16 cluster=1 lds_kb=0 -> rc=0 path=0 nt=1024 G=6 groups=1 CH=16 x_in_lds=1 cluster=1 lds_bytes=89040
  N=130 E=4 B=1 threads=0 rows_per_chunk=16 cluster=2 lds_kb=0 -> rc=0 path=0 nt=1024 G=6 groups=1 CH=16 x_in_lds=1 cluster=2 lds_bytes=74016"""


def _runs():
    runs = []
    # every N at both widths and every S0 (KS = 3 ... 6), X^T in LDS
    for N in (33, 64, 65, 130):
        for s0 in range(len(S0_VALUES)):
            runs.append((N, B, 256, 0, 1, 0, 0, s0, 1))
        runs.append((N, B, 1024, 0, 1, 0, 0, 1, 1))
    # several pair groups (the queue starts again per group); X^T in global memory
    runs.append((33, B, 256, 0, 1, 16, 0, 1, 6))
    runs.append((65, B, 256, 0, 1, 28, 0, 2, 3))
    runs.append((130, B, 256, 0, 1, 44, 0, 1, 3))
    runs.append((130, B, 1024, 0, 1, 44, 0, 2, 3))
    # all pairs in one group, X^T in global memory
    runs.append((130, B, 256, 0, 1, 90, 0, 0, 1))
    # the time index as an input dimension (its degrees are higher: KS = 5, 6 at the small S0)
    runs.append((33, B, 256, 0, 1, 0, 1, 0, 1))
    runs.append((130, B, 256, 0, 1, 0, 1, 0, 1))
    # the cooperative form, one candidate, and the plain run at its chunk length (same bits for the first candidate)
    runs.append((130, B, 1024, 16, 1, 0, 0, 1, 1))
    runs.append((130, 1, 0, 16, 2, 0, 0, 1, 1))
    return runs


RUNS = _runs()
CASES = sorted({(r[0], r[6], r[7]) for r in RUNS})


def run_key(run):
    return "N%d_B%d_nt%d_rpc%d_cl%d_lds%d_tm%d_s%d_g%d" % run


def make_case(N, tm, s0):
    return synth.make_workload(N=N, D=D, A=1, H=H, B=B, include_time=bool(tm), seed=7000 + 10 * N + D, time0=3.0, s0=S0_VALUES[s0])


def apply_options(engine, nt, rpc, cs, lds):
    engine.set_option("force_path", 0)
    engine.set_option("force_separable", 1)
    engine.set_option("threads", nt)
    engine.set_option("rows_per_chunk", rpc)
    engine.set_option("cluster", cs)
    engine.set_option("lds_limit_kb", lds)


def reset_options(engine):
    for name in ("force_path", "force_separable", "threads", "rows_per_chunk", "cluster", "lds_limit_kb"):
        engine.set_option(name, 0)


def degrees_of(case, max_arg):
    """The Taylor degrees of the off-diagonal pairs of `case` = (N, tm, s0 index), per candidate and step, restated on the numpy
    oracle's trajectory: an int array (B, H, 3).  `max_arg` = kTaylorMaxArg of csrc/rollout_kernel.h."""
    import numpy as np
    import hetero_cases as hc
    from oracle import gpmpc_oracle as orc
    w = make_case(*case)
    o = orc.evaluate_candidates(orc.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises), w)
    out = []
    for c in range(B):
        deg, _, pairs = hc.taylor_degrees(w, o["mu"][c], o["Sig"][c], max_arg)
        off = [q for q, (a, b) in enumerate(pairs) if a != b]
        out.append(deg[:, off])
    return np.stack(out)


def run_all(engine):
    """Every run of RUNS on `engine`: {key: {"mu", "Sig", "J"} as numpy arrays}; a case's model is prepared once, and every launch has to
    be the fused-horizon kernel's, in the form and with the number of pair groups the run names."""
    out = {}
    for case in CASES:
        N, tm, s0 = case
        w = make_case(N, tm, s0)
        engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        engine.set_cost(w.target, w.W, w.W_T, w.kappa)
        try:
            for run in RUNS:
                if (run[0], run[6], run[7]) != case:
                    continue
                _, nB, nt, rpc, cs, lds, _, _, groups = run
                apply_options(engine, nt, rpc, cs, lds)
                o = engine.rollout(w.actions[:nB], w.mu0, w.S0, w.include_time, w.time0)
                assert engine.last_rollout_path == 0, (run, engine.last_rollout_path)         # the fused-horizon kernel
                assert engine.last_cluster == cs, (run, engine.last_cluster)
                assert engine.last_pair_groups == groups, (run, engine.last_pair_groups)
                out[run_key(run)] = {k: o[k].cpu().numpy().copy() for k in ("mu", "Sig", "J")}
        finally:
            reset_options(engine)
    return out
