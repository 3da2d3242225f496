"""Runs of tests/test_gpu_item_loop_bits.py and of tools/gen_item_loop_golden.py (which pins their bits): the element loops of
the fused-horizon kernel's pairwise items (item_taylor2 / item_exp2 of csrc/rollout_kernel.h) through every branch, workgroup
width and chunk length.  One function, so that the fixture and the test can never disagree about the inputs.

A run = (N, D, candidates, force_path, threads, rows_per_chunk, cluster); H = 3, A = 1; a run of fewer candidates than B takes
the leading ones of the shape's workload.  force_path 1 is the direct-exp loop, 2 Taylor
without separable pairs (the off-diagonal branch of the Taylor loop); cluster > 1 is the cooperative form."""
from oracle import synth

H = 3
B = 3

# (N, D): each the smallest that reaches its corner
SHAPES = [
    (33, 3),      # odd N: the masked second column, rows not 16-byte aligned, one column unit, a 1-row last chunk
    (130, 3),     # two column units, the triangle lane map, a 2-row last chunk, the prefetch running into the last output's pad rows
    (70, 2),
    (66, 4),      # four rows per trip
]


def _runs():
    runs = []
    for N, D in SHAPES:
        for fp in (0, 1, 2):
            for nt in (256, 512, 1024):
                runs.append((N, D, B, fp, nt, 0, 1))
    for fp in (0, 1, 2):
        runs.append((130, 3, B, fp, 0, 16, 1))            # short chunks: many slots per pair
    for cs in (2, 9):
        runs.append((130, 3, 1, 0, 0, 16, cs))            # the cooperative form: the plain run above at 16 rows, first candidate
    return runs


RUNS = _runs()


def run_key(run):
    return "N%d_D%d_B%d_fp%d_nt%d_rpc%d_cl%d" % run


def make_case(N, D):
    return synth.make_workload(N=N, D=D, A=1, H=H, B=B, seed=7000 + 10 * N + D)


def apply_options(engine, fp, nt, rpc, cs):
    engine.set_option("force_path", fp)
    engine.set_option("threads", nt)
    engine.set_option("rows_per_chunk", rpc)
    engine.set_option("cluster", cs)


def reset_options(engine):
    engine.set_option("force_path", 0)
    engine.set_option("threads", 0)
    engine.set_option("rows_per_chunk", 0)
    engine.set_option("cluster", 0)


def run_all(engine):
    """Every run of RUNS on `engine`: {key: {"mu", "Sig", "J"} as numpy arrays}; the model of a shape is prepared once."""
    out = {}
    prepared = None
    try:
        for run in RUNS:
            N, D, nB, fp, nt, rpc, cs = run
            w = make_case(N, D)
            if prepared != (N, D):
                engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
                engine.set_cost(w.target, w.W, w.W_T, w.kappa)
                prepared = (N, D)
            apply_options(engine, fp, nt, rpc, cs)
            o = engine.rollout(w.actions[:nB], w.mu0, w.S0)
            assert engine.last_rollout_path == 0, (run, engine.last_rollout_path)         # the fused-horizon kernel
            assert engine.last_cluster == cs, (run, engine.last_cluster)
            out[run_key(run)] = {k: o[k].cpu().numpy().copy() for k in ("mu", "Sig", "J")}
    finally:
        reset_options(engine)
    return out
