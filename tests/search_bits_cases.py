"""Runs of tests/test_gpu_search_bits.py and of tools/gen_search_bits_golden.py (which pins their bits): every device-resident
search -- gpmpc_cem_search, gpmpc_cem_local + gpmpc_cem_merge, gpmpc_lbfgs_search, gpmpc_train_search, gpmpc_ilqr_search -- on
the smallest cases that reach the corners of the code they share (csrc/action_mapper.h, the sort / key load / refit of
csrc/search.hip, finite_d / clip01 of csrc/device_common.h, the objective-only rollout setup).  One function, so that the fixture
and the test can never disagree about the inputs.

Model: synth.make_workload(N=24, D=2, A, H, B=2, seed=7), cost = distance to 0.5 with identity weights (as
tests/test_gpu_cem_search.py::setup).  Every result is a dict of numpy arrays, keyed "<group>/<case>"."""
import numpy as np
import torch

from oracle import synth

N, D = 24, 2
SEED = 11                              # the Philox path
MAX_CHANGE = {2: np.array([0.3, 0.6]), 5: np.array([0.3, 0.6, 0.45, 0.2, 0.8])}
ACTION_PREV = {2: np.array([0.2, 0.7]), 5: np.array([0.2, 0.7, 0.5, 0.9, 0.1])}

# (A, H) of every model the runs prepare, in the order they are prepared
MODELS = [(2, 3), (5, 13)]

# cem_search: A = 2, H = 3, 3 iterations.  B = 2 the minimum, 65 one past a wavefront, 2049 -> P2 = 4096: the sort loops stride
# more than once over the 1024 threads
CEM_A, CEM_H, CEM_ITERS = 2, 3, 3
CEM_RUNS = [(B, ne, deriv, first) for B in (2, 65, 2049) for ne in sorted({1, 9, B}) if ne <= B
            for deriv in (0, 1) for first in (0, 1)]
# cem_local + cem_merge: B_total = 130 in the slices [0, 65), [65, 130) and an empty one, n_elite = 9, 3 iterations
SHARD_B, SHARD_SLICES, SHARD_ELITE, SHARD_ITERS = 130, [(0, 65), (65, 65), (130, 0)], 9, 3
SHARD_RUNS = [(deriv,) for deriv in (0, 1)]
# lbfgs_search: B = 3, history 3, 6 iterations (the pair ring wraps); n = 6 and n = 65 (one past the lane stride)
LBFGS_B, LBFGS_HISTORY, LBFGS_ITERS = 3, 3, 6
LBFGS_RUNS = [(H, A, deriv, prop) for (H, A) in ((3, 2), (13, 5)) for deriv in (0, 1) for prop in ("moment", "linearized")]
# train_search: R = 2 restarts on the (X, Y) of the (A, H) = (2, 3) model, history 3, 4 iterations
TRAIN_R, TRAIN_HISTORY, TRAIN_ITERS = 2, 3, 4
# ilqr_search: B = 3, H = 3, A = 2, L = 4, 3 iterations
ILQR_B, ILQR_H, ILQR_A, ILQR_L, ILQR_ITERS = 3, 3, 2, 4, 3


def cem_key(run):
    return "cem_search/B%d_ne%d_deriv%d_first%d" % run


def shard_key(run):
    return "cem_shard/deriv%d" % run


def lbfgs_key(run):
    return "lbfgs_search/H%d_A%d_deriv%d_%s" % run


TRAIN_KEY = "train_search/R2"
ILQR_KEY = "ilqr_search/B3"
KEYS = [cem_key(r) for r in CEM_RUNS] + [shard_key(r) for r in SHARD_RUNS] + [lbfgs_key(r) for r in LBFGS_RUNS] + [TRAIN_KEY, ILQR_KEY]


def make_case(A, H):
    return synth.make_workload(N=N, D=D, A=A, H=H, B=2, seed=7)


def _load(engine, A, H):
    w = make_case(A, H)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    engine.set_cost(np.full(D + A, 0.5), np.eye(D + A), np.eye(D), w.kappa)
    return w


def _mapper(A, deriv):
    return dict(max_change=MAX_CHANGE[A], action_prev=ACTION_PREV[A]) if deriv else {}


def _np(t):
    return t.cpu().numpy().copy()


def _cem(engine, w, out):
    A, H, n = CEM_A, CEM_H, CEM_A * CEM_H
    first = np.random.default_rng(100).uniform(size=n)
    for run in CEM_RUNS:
        B, ne, deriv, use_first = run
        x, J = engine.cem_search(w.mu0, w.S0, B, H, A, CEM_ITERS, ne, seed=SEED, first_candidate=first if use_first else None,
                                 **_mapper(A, deriv))
        out[cem_key(run)] = {"best": x, "best_J": np.array([J])}
    for run in SHARD_RUNS:
        (deriv,) = run
        state = torch.zeros(3 * n + 1, dtype=torch.float64, device=engine.device)
        res = {}
        for it in range(SHARD_ITERS):
            recs = [engine.cem_local(w.mu0, w.S0, SHARD_B, b0, Bl, H, A, it, SHARD_ELITE, state, seed=SEED, first_candidate=first,
                                     **_mapper(A, deriv)) for (b0, Bl) in SHARD_SLICES]
            for s, rec in enumerate(recs):
                res[f"records_it{it}_slice{s}"] = _np(rec)
            engine.cem_merge(torch.cat(recs).contiguous(), SHARD_ELITE, n, it, state)
            res[f"state_it{it}"] = _np(state)
        out[shard_key(run)] = res


def _lbfgs(engine, w, run, out):
    H, A, deriv, prop = run
    n = H * A
    x0 = np.random.default_rng(200 + n).uniform(size=(LBFGS_B, n))
    st = engine.lbfgs_state(LBFGS_B, n, LBFGS_HISTORY)
    rec = engine.lbfgs_search(st, w.mu0, w.S0, H, A, LBFGS_ITERS, x0=x0, propagation=prop, **_mapper(A, deriv))
    out[lbfgs_key(run)] = {"state": _np(st["buffer"]), "winner": _np(rec)}


def _train(engine, w, out):
    base = np.concatenate([w.lengthscales, w.outputscales[:, None], w.noises[:, None]], axis=1)
    n = base.shape[1]
    x0 = np.random.default_rng(300).uniform(0.05, 0.95, size=(TRAIN_R, D, n))
    st = engine.lbfgs_state(TRAIN_R * D, n, TRAIN_HISTORY)
    rec = engine.train_search(st, w.X, w.Y, base / 8.0, base * 8.0, TRAIN_ITERS, x0=x0)
    out[TRAIN_KEY] = {"state": _np(st["buffer"]), "winner": _np(rec)}


def _ilqr(engine, w, out):
    x0 = np.random.default_rng(400).uniform(size=(ILQR_B, ILQR_H, ILQR_A))
    st = engine.ilqr_state(ILQR_B, ILQR_H, ILQR_A, ILQR_L)
    rec = engine.ilqr_search(st, w.mu0, w.S0, ILQR_ITERS, x0)
    out[ILQR_KEY] = {"state": _np(st["buffer"]), "winner": _np(rec)}


def run_all(engine):
    """Every run on `engine`: {key: {name: numpy array}}; each model is prepared once.  (train_search replaces nothing the other
    searches read: it runs last on its model.)"""
    out = {}
    for (A, H) in MODELS:
        w = _load(engine, A, H)
        if (A, H) == (CEM_A, CEM_H):
            _cem(engine, w, out)
        for run in LBFGS_RUNS:
            if (run[1], run[0]) == (A, H):
                _lbfgs(engine, w, run, out)
        if (A, H) == (ILQR_A, ILQR_H):
            _ilqr(engine, w, out)
            _train(engine, w, out)
    assert list(out) and set(out) == set(KEYS)
    return out
