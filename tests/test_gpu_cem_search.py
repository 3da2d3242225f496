"""Tier 2 (GPU): the kernels of csrc/search.hip (gpmpc_cem_search / gpmpc_cem_local / gpmpc_cem_merge) against the numpy
restatement of tests/cem_ref.py -- the Philox draws, both action mappers, the sort with its tie rule, the slice records, the
refit and the incumbent rule, at the sizes where the kernels change path.

How the kernels are observed: cem_local with ONE slice [0, B) and n_elite = B returns every candidate's record, so X and J of
the whole population are read back and reordered by the index column; cem_merge leaves mean | std | best | best J in `state`.

Tolerances: copies (X at iteration 0, record rows, best, best J, padding rows) are compared bit for bit.  Computed values (normal
draws, mean, std) by the rule of test_gpu_prepare_sparse.py,
    tolerance = 10 e64 + 64 eps scale            (e64: the float64 restatement's own error against the longdouble one on that case,
                                                  computed here, never taken from the GPU; eps = 2^-52)
with scale = 1 (the width of the box) for mean and std and scale = max |z| for the normal draws z; a sampled coordinate
mean + std z inherits std tol(z) plus 2 eps for its own multiply-add.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cem_ref as ref
from helpers import record
from oracle import synth

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LD = np.longdouble


def tol(e64, scale=1.0):
    return 10.0 * float(e64) + 64.0 * EPS * float(scale)


def err(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)))) if np.size(a) else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


_WORK = {}
_LOADED = {}


def setup(engine, A, H, time=False):
    """The model of (A, H, time): N = 24, D = 2; cost = distance to 0.5 with identity weights.  Prepared when it changes."""
    key = (A, H, time)
    if key not in _WORK:
        _WORK[key] = synth.make_workload(N=24, D=2, A=A, H=H, B=2, include_time=time, time0=3.0, seed=7)
    w = _WORK[key]
    if _LOADED.get(id(engine)) != key:
        engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        engine.set_cost(np.full(2 + A, 0.5), np.eye(2 + A), np.eye(2), w.kappa)
        _LOADED[id(engine)] = key
    return w


def zeros_state(engine, n):
    return torch.zeros(3 * n + 1, dtype=torch.float64, device=engine.device)


def records(engine, w, B_total, b0, Bl, H, A, it, n_elite, state=None, **kw):
    state = zeros_state(engine, H * A) if state is None else state
    rec = engine.cem_local(w.mu0, w.S0, B_total, b0, Bl, H, A, it, n_elite, state, include_time=w.include_time,
                           time0=w.time0, **kw)
    return rec.cpu().numpy()


def by_index(rec, b0=0):
    """X and J of the records in candidate order (the index column must be a permutation of the slice)."""
    idx = rec[:, 1].astype(np.int64) - b0
    assert np.array_equal(np.sort(idx), np.arange(rec.shape[0]))
    X, J = np.empty_like(rec[:, 2:]), np.empty(rec.shape[0])
    X[idx], J[idx] = rec[:, 2:], rec[:, 0]
    return X, J


def population(engine, w, B, H, A, it, state=None, **kw):
    rec = records(engine, w, B, 0, B, H, A, it, B, state, **kw)
    X, J = by_index(rec)
    return X, J, rec


def make_noise(rng, iters, B, n):
    return np.concatenate([rng.uniform(size=(1, B, n)), rng.standard_normal((iters - 1, B, n))])


def rollout_J(engine, w, actions):
    return engine.rollout(actions, w.mu0, w.S0, include_time=w.include_time, time0=w.time0, trajectories=False,
                          stage_costs=False)["J"].cpu().numpy()


# -- a. draws ---------------------------------------------------------------------------------------------------------------------
SEEDS = [0, 11, 2 ** 63 + 5]
A_DRAW, H_DRAW, B_DRAW, N_DRAW = 2, 3, 130, 6


@pytest.mark.parametrize("seed", SEEDS)
def test_uniform_draws_of_iteration_0_bit_for_bit(engine, seed):
    w = setup(engine, A_DRAW, H_DRAW)
    u = ref.draws(seed, 0, B_DRAW, N_DRAW)
    X, _, _ = population(engine, w, B_DRAW, H_DRAW, A_DRAW, 0, seed=seed)
    assert same_bits(X, u)                                       # without a warm start slot 0 is a draw like any other
    first = np.random.default_rng(1).uniform(size=N_DRAW)
    Xw, _, _ = population(engine, w, B_DRAW, H_DRAW, A_DRAW, 0, seed=seed, first_candidate=first)
    assert same_bits(Xw[0], first) and same_bits(Xw[1:], u[1:])


@pytest.mark.parametrize("it", [1, 3])
@pytest.mark.parametrize("seed", SEEDS)
def test_normal_draws_against_longdouble(engine, seed, it):
    w = setup(engine, A_DRAW, H_DRAW)
    n = N_DRAW
    z64, zld = ref.draws(seed, it, B_DRAW, n), ref.draws(seed, it, B_DRAW, n, LD)
    e64, zmax = err(z64, zld), float(np.max(np.abs(zld)))
    tol_z = tol(e64, zmax)
    assert zmax < 8.7
    best = np.random.default_rng(2).uniform(size=n)
    # std = 2^-6: nothing clips, and X - 0.5 is the draw scaled by a power of two
    std = 2.0 ** -6
    host = np.concatenate([np.full(n, 0.5), np.full(n, std), best, [1.25]])
    state = torch.as_tensor(host, device=engine.device)
    X, _, _ = population(engine, w, B_DRAW, H_DRAW, A_DRAW, it, state, seed=seed)
    want = ref.sample(it, 0, B_DRAW, B_DRAW, n, host, None, seed, LD)
    assert np.all((want[1:] > 0.0) & (want[1:] < 1.0))
    e_x = err(X[1:], want[1:])
    e_z = e_x / std
    print(f"seed {seed} it {it}: draws GPU {e_z:.3e} (tol {tol_z:.3e}, numpy {e64:.3e}, max |z| {zmax:.3f})")
    record(f"cem_draws[seed={seed},it={it}]", draws=e_z, numpy_draws=e64, tol_draws=tol_z)
    assert e_x <= std * tol_z + 2.0 * EPS
    assert same_bits(X[0], best)                                 # slot 0 is the incumbent
    assert same_bits(state.cpu().numpy(), host)                  # cem_local reads the state, never writes it
    # std = 1: most of the population reaches the faces of the box
    host1 = np.concatenate([np.full(n, 0.5), np.full(n, 1.0), best, [1.25]])
    X1, _, _ = population(engine, w, B_DRAW, H_DRAW, A_DRAW, it, torch.as_tensor(host1, device=engine.device), seed=seed)
    v = LD(0.5) + zld                                            # unclipped
    tol_v = tol_z + 2.0 * EPS
    assert np.all((X1 >= 0.0) & (X1 <= 1.0))
    lo, hi = v[1:] < -tol_v, v[1:] > 1.0 + tol_v
    assert lo.sum() > 50 and hi.sum() > 50 and (~lo & ~hi).sum() > 50
    assert np.all(X1[1:][lo] == 0.0) and np.all(X1[1:][hi] == 1.0)
    assert err(X1[1:], np.clip(v[1:], LD(0.0), LD(1.0))) <= tol_v
    assert same_bits(X1[0], best)


@pytest.mark.parametrize("it", [0, 1])
def test_slices_draw_the_rows_of_the_whole_population(engine, it):
    """Counters and the caller's noise are indexed by the GLOBAL candidate."""
    w = setup(engine, A_DRAW, H_DRAW)
    n = N_DRAW
    rng = np.random.default_rng(3)
    host = np.concatenate([np.full(n, 0.5), np.full(n, 0.25), rng.uniform(size=n), [1.25]])
    state = torch.as_tensor(host, device=engine.device)
    first = rng.uniform(size=n)
    for draws in (dict(seed=11), dict(noise=make_noise(rng, 2, B_DRAW, n))):
        whole, _, _ = population(engine, w, B_DRAW, H_DRAW, A_DRAW, it, state, first_candidate=first, **draws)
        src = draws.get("noise", 11)
        if it == 0:
            assert same_bits(whole, ref.sample(0, 0, B_DRAW, B_DRAW, n, None, first, src))
        for lo, hi in ((0, 50), (50, 50), (50, 130)):
            rec = records(engine, w, B_DRAW, lo, hi - lo, H_DRAW, A_DRAW, it, max(hi - lo, 1), state, first_candidate=first, **draws)
            if hi == lo:
                assert rec.shape == (1, n + 2) and rec[0, 0] == np.inf and rec[0, 1] == 2147483647.0 and np.all(rec[0, 2:] == 0.0)
                continue
            X, _ = by_index(rec, lo)
            assert same_bits(X, whole[lo:hi])


# -- b. mappers, through J --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time", [False, True])
@pytest.mark.parametrize("A,H", [(1, 1), (2, 3), (3, 4)])
def test_mappers_through_the_objective(engine, A, H, time):
    w = setup(engine, A, H, time)
    B, n = 65, H * A
    rng = np.random.default_rng(10 * A + H)
    noise = make_noise(rng, 1, B, n)
    # identity: the search's J is the rollout's J of the same (B, H, A) actions
    X, J, _ = population(engine, w, B, H, A, 0, noise=noise)
    assert same_bits(X, noise[0])
    J_roll = rollout_J(engine, w, ref.to_model(X, H, A))
    assert same_bits(J, J_roll)
    # derivative mapper: its own scale and start per action dimension, deltas large enough for both clamps
    mc = np.array([0.6, 0.9, 0.8])[:A]
    prev = np.array([0.3, 0.8, 0.5])[:A]
    acts = ref.to_model(X, H, A, mc, prev)
    for a in range(A if H > 1 else 0):
        assert np.any(acts[:, :, a] == 0.0) and np.any(acts[:, :, a] == 1.0) and np.any((acts[:, :, a] > 0) & (acts[:, :, a] < 1))
    assert np.any(acts == 0.0) and np.any((acts > 0.0) & (acts < 1.0))
    Xd, Jd, _ = population(engine, w, B, H, A, 0, noise=noise, max_change=mc, action_prev=prev)
    assert same_bits(Xd, noise[0])
    Jd_roll = rollout_J(engine, w, acts)
    e = float(np.max(np.abs(Jd - Jd_roll) / np.abs(Jd_roll)))
    record(f"cem_mapper[A={A},H={H},time={int(time)}]", derivative_J_rel=e)
    assert e <= 1e-9                                             # the mapper's multiply-subtract may be contracted
    if A > 1:                                                    # the objective tells the action dimensions apart
        other = rollout_J(engine, w, ref.to_model(X, H, A, np.full(A, mc[0]), prev))
        assert np.max(np.abs(Jd - other) / np.abs(other)) > 1e-6


# -- c. sort and records of a slice -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 3, 64, 65, 1024, 1025, 2048, 2049, 4096])
def test_records_are_the_population_ordered_by_objective_then_index(engine, B):
    A, H, n = 2, 3, 6
    w = setup(engine, A, H)
    noise = make_noise(np.random.default_rng(B), 1, B, n)
    X, J, rec = population(engine, w, B, H, A, 0, noise=noise)
    assert same_bits(X, noise[0])
    assert same_bits(rec, ref.elite_records(J, X, 0, B))
    assert np.all(np.diff(rec[:, 0]) >= 0.0)
    for n_elite in sorted({1, 9, B - 1}):
        if 1 <= n_elite <= B:
            part = records(engine, w, B, 0, B, H, A, 0, n_elite, noise=noise)
            assert same_bits(part, rec[:n_elite])


def test_ties_between_different_vectors_come_out_by_index(engine):
    """Derivative mapper with action_prev = 0: every candidate whose coordinates are all below 0.5 has negative deltas only, a
    negative running sum and so all-zero actions -- one objective for 40 different vectors."""
    A, H, n, B = 2, 3, 6, 65
    w = setup(engine, A, H)
    rng = np.random.default_rng(65)
    noise = make_noise(rng, 1, B, n)
    tied = np.sort(rng.permutation(B)[:40])
    noise[0, tied] = rng.uniform(0.0, 0.5, size=(40, n))
    assert np.unique(noise[0, tied], axis=0).shape[0] == 40
    kw = dict(max_change=np.array([0.3, 0.6]), action_prev=np.zeros(A))
    assert np.all(ref.to_model(noise[0, tied], H, A, kw["max_change"], kw["action_prev"]) == 0.0)
    X, J, rec = population(engine, w, B, H, A, 0, noise=noise, **kw)
    assert same_bits(X, noise[0])
    assert np.unique(J[tied].view(np.uint64)).size == 1          # precondition: one J, bit for bit
    rows = np.flatnonzero(rec[:, 0] == J[tied[0]])
    assert rows.size >= 40 and np.array_equal(rows, np.arange(rows[0], rows[0] + rows.size))     # one contiguous group
    assert np.all(np.diff(rec[rows, 1]) > 0) and set(tied) <= set(rec[rows, 1].astype(int))
    assert same_bits(rec, ref.elite_records(J, X, 0, B))
    part = records(engine, w, B, 0, B, H, A, 0, 9, noise=noise, **kw)
    assert same_bits(part, rec[:9])


def test_short_and_empty_slices_pad_their_records(engine):
    A, H, n, B = 2, 3, 6, 65
    w = setup(engine, A, H)
    noise = make_noise(np.random.default_rng(66), 1, B, n)
    X, J, _ = population(engine, w, B, H, A, 0, noise=noise)
    rec = records(engine, w, B, 60, 5, H, A, 0, 9, noise=noise)
    assert same_bits(rec[:5, 2:], X[rec[:5, 1].astype(int)])
    assert same_bits(rec, ref.elite_records(J[60:], X[60:], 60, 9))
    assert np.all(rec[5:, 0] == np.inf) and np.all(rec[5:, 1] == 2147483647.0) and same_bits(rec[5:, 2:], np.zeros((4, n)))
    empty = records(engine, w, B, 60, 0, H, A, 0, 9, noise=noise)
    assert same_bits(empty, ref.elite_records(np.empty(0), np.empty((0, n)), 60, 9))
    assert np.all(empty[:, 0] == np.inf) and np.all(empty[:, 1] == 2147483647.0) and same_bits(empty[:, 2:], np.zeros((9, n)))


# -- d. cem_merge alone, on hand-made records -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bare_engine():
    """An engine that never prepared a model: gpmpc_cem_merge needs none."""
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


KEYS = np.array([-3.5, -1.0, 0.0, 0.125, 0.25, 2.0, 1e300, np.inf])


def hand_made_records(lists, n_elite, n, seed):
    """Keys from eight values (ties everywhere, +inf among them), global indices a shuffled permutation (slot order is not index
    order), vectors uniform in [0, 1]; with more than one list, the last one is part padding."""
    rng = np.random.default_rng(seed)
    R = lists * n_elite
    rec = np.empty((R, n + 2))
    rec[:, 0] = rng.choice(KEYS, size=R)
    rec[:, 1] = rng.permutation(R) + 5
    rec[:, 2:] = rng.uniform(size=(R, n))
    if lists > 1 and n_elite > 1:
        pad = max(1, n_elite // 3)
        rec[R - pad:, 0], rec[R - pad:, 1], rec[R - pad:, 2:] = np.inf, 2147483647.0, 0.0
    return rec


MERGE_CASES = [(1, 1, 1), (1, 1, 1500), (1, 2, 7), (3, 5, 7), (3, 5, 1025), (8, 8, 1), (8, 8, 1024), (5, 13, 7), (5, 13, 1024),
               (5, 13, 1025), (5, 13, 1500), (4, 256, 7), (5, 205, 7), (8, 256, 7), (1, 2049, 7), (8, 512, 7), (1, 4096, 7)]


def run_merge(eng, rec, n_elite, n, it, state_host):
    state = torch.as_tensor(np.asarray(state_host, dtype=np.float64), device=eng.device)
    eng.cem_merge(torch.as_tensor(rec, device=eng.device), n_elite, n, it, state)
    return state.cpu().numpy()


def check_state(name, got, rec, n_elite, n, state_in, first):
    """`got` against refit: best | best J bit for bit, mean and std by the rule.  Returns the float64 restatement."""
    s64, sld = ref.refit(rec, n_elite, state_in, first), ref.refit(rec, n_elite, state_in, first, LD)
    e64_m, e64_s = err(s64[:n], sld[:n]), err(s64[n:2 * n], sld[n:2 * n])
    e_m, e_s = err(got[:n], sld[:n]), err(got[n:2 * n], sld[n:2 * n])
    bit_equal = same_bits(got[:n], s64[:n])
    print(f"{name}: mean GPU {e_m:.3e} (tol {tol(e64_m):.3e}, numpy {e64_m:.3e}, bit-equal to numpy: {bit_equal})  "
          f"std GPU {e_s:.3e} (tol {tol(e64_s):.3e}, numpy {e64_s:.3e})")
    record(name, mean=e_m, std=e_s, numpy_mean=e64_m, numpy_std=e64_s, tol_mean=tol(e64_m), tol_std=tol(e64_s),
           mean_bit_equal_to_numpy=float(bit_equal))
    assert same_bits(got[2 * n:], s64[2 * n:])
    assert e_m <= tol(e64_m) and e_s <= tol(e64_s)
    return s64


@pytest.mark.parametrize("lists,n_elite,n", MERGE_CASES)
def test_merge_against_the_refit_of_hand_made_records(bare_engine, lists, n_elite, n):
    rec = hand_made_records(lists, n_elite, n, 1000 * lists + n_elite + n)
    sentinel = np.full(3 * n + 1, -7.0)
    got = run_merge(bare_engine, rec, n_elite, n, 0, sentinel)
    s64 = check_state(f"cem_merge[{lists}x{n_elite},n={n}]", got, rec, n_elite, n, sentinel, True)
    order = np.lexsort((rec[:, 1], rec[:, 0]))
    assert same_bits(got[2 * n:3 * n], rec[order[0], 2:]) and got[3 * n] == rec[order[0], 0]
    if n_elite == 1:
        assert same_bits(got[:n], rec[order[0], 2:]) and same_bits(got[n:2 * n], np.full(n, 1e-3))
    # later iterations: an incumbent as good as the new leader stays (strict improvement); a better leader replaces it
    lead_J = rec[order[0], 0]
    inc = np.concatenate([np.zeros(2 * n), np.full(n, 0.375), [lead_J]])
    kept = run_merge(bare_engine, rec, n_elite, n, 2, inc)
    assert same_bits(kept[2 * n:], inc[2 * n:]) and same_bits(kept[:2 * n], got[:2 * n])
    assert same_bits(kept[2 * n:], ref.refit(rec, n_elite, inc, False)[2 * n:])
    if np.isfinite(lead_J):                                      # (a single record may carry the +inf key)
        inc[3 * n] = np.nextafter(lead_J, np.inf)
        took = run_merge(bare_engine, rec, n_elite, n, 2, inc)
        assert same_bits(took[2 * n:], s64[2 * n:]) and same_bits(took[:2 * n], got[:2 * n])


@pytest.mark.parametrize("lists,n_elite,n", [(3, 5, 7), (1, 2049, 7)])
def test_merge_first_iteration_with_every_key_infinite(bare_engine, lists, n_elite, n):
    rec = hand_made_records(lists, n_elite, n, 77)
    rec[:, 0] = np.inf
    sentinel = np.full(3 * n + 1, -7.0)
    got = run_merge(bare_engine, rec, n_elite, n, 0, sentinel)
    check_state(f"cem_merge_all_inf[{lists}x{n_elite},n={n}]", got, rec, n_elite, n, sentinel, True)
    leader = int(np.argmin(rec[:, 1]))                           # the leader by index
    assert same_bits(got[2 * n:3 * n], rec[leader, 2:]) and got[3 * n] == np.inf
    # afterwards nothing is a strict improvement on +inf
    kept = run_merge(bare_engine, rec, n_elite, n, 1, got)
    assert same_bits(kept, got)


# -- e. one step at a time, then the whole search ---------------------------------------------------------------------------------
CHAIN = [(B, ne) for B in (2, 65, 1025, 4096) for ne in sorted({1, 9, B}) if ne <= B]


@pytest.mark.parametrize("draws", ["noise", "seed"])
@pytest.mark.parametrize("deriv", [False, True])
@pytest.mark.parametrize("B,n_elite", CHAIN)
def test_every_step_of_the_search_then_the_whole_search(engine, B, n_elite, deriv, draws):
    A, H, n, iters = 2, 3, 6, 3
    w = setup(engine, A, H)
    rng = np.random.default_rng(B + n_elite)
    first = rng.uniform(size=n)
    kw = dict(max_change=np.array([0.3, 0.6]), action_prev=np.array([0.2, 0.7])) if deriv else {}
    src = make_noise(rng, iters, B, n) if draws == "noise" else 11
    dr = dict(noise=src) if draws == "noise" else dict(seed=src)
    name = f"cem_chain[B={B},n_elite={n_elite},deriv={int(deriv)},{draws}]"
    state = zeros_state(engine, n)
    worst = dict(x=0.0, tol_x=0.0)
    for it in range(iters):
        before = state.cpu().numpy()
        rec_dev = engine.cem_local(w.mu0, w.S0, B, 0, B, H, A, it, B, state, first_candidate=first, **dr, **kw)
        rec = rec_dev.cpu().numpy()
        X, J = by_index(rec)
        # the draws of this iteration, around the DEVICE's own state
        if it == 0:
            assert same_bits(X, ref.sample(0, 0, B, B, n, None, first, src))
        else:
            tol_x = 2.0 * EPS
            if draws == "seed":
                z64, zld = ref.draws(src, it, B, n), ref.draws(src, it, B, n, LD)
                tol_x += float(np.max(before[n:2 * n])) * tol(err(z64, zld), np.max(np.abs(zld)))
            e_x = err(X, ref.sample(it, 0, B, B, n, before, first, src, LD))
            worst = dict(x=max(worst["x"], e_x), tol_x=max(worst["tol_x"], tol_x))
            assert e_x <= tol_x
            assert same_bits(X[0], before[2 * n:3 * n])
            assert np.all((X >= 0.0) & (X <= 1.0))
        # the objective is the rollout's; the records are the population ordered by the device's own J
        acts = ref.to_model(X, H, A, kw.get("max_change"), kw.get("action_prev"))
        J_roll = rollout_J(engine, w, acts)
        assert np.max(np.abs(J - J_roll) / np.abs(J_roll)) <= 1e-9
        assert same_bits(rec, ref.elite_records(J, X, 0, B))
        # the refit on the n_elite leaders
        engine.cem_merge(rec_dev[:n_elite].contiguous(), n_elite, n, it, state)
        check_state(f"{name}[it={it}]", state.cpu().numpy(), rec[:n_elite], n_elite, n, before, it == 0)
    record(name, **worst)
    host = state.cpu().numpy()
    x, Jb = engine.cem_search(w.mu0, w.S0, B, H, A, iters, n_elite, first_candidate=first, include_time=w.include_time,
                              time0=w.time0, **dr, **kw)
    assert same_bits(x, host[2 * n:3 * n]) and same_bits(np.array([Jb]), host[3 * n:])


# -- f. errors --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_touch_nothing(engine, bare_engine):
    from gp_mpc_amd import _lib as L
    A, H, n, B = 2, 3, 6, 65
    w = setup(engine, A, H)
    noise = make_noise(np.random.default_rng(4), 1, B, n)
    good = records(engine, w, B, 0, B, H, A, 0, 9, noise=noise)
    mc = np.array([0.3, 0.6])

    def local(B_total, b0, Bl, n_elite, rows, **kw):
        out = torch.full((rows, n + 2), -7.0, dtype=torch.float64, device=engine.device)
        state = torch.full((3 * n + 1,), -7.0, dtype=torch.float64, device=engine.device)
        with pytest.raises((L.GpmpcError, ValueError)):
            engine.cem_local(w.mu0, w.S0, B_total, b0, Bl, H, A, 0, n_elite, state, out=out, **kw)
        torch.cuda.synchronize()
        assert np.all(out.cpu().numpy() == -7.0) and np.all(state.cpu().numpy() == -7.0)
        assert same_bits(records(engine, w, B, 0, B, H, A, 0, 9, noise=noise), good)       # the engine still works

    local(1, 0, 1, 1, 1)                                         # B = 1
    local(4097, 0, 4097, 9, 9)                                   # B = 4097
    local(B, 0, B, 0, 1)                                         # n_elite = 0
    local(B, 0, B, B + 1, B + 1)                                 # n_elite = B + 1
    local(B, 60, 6, 9, 9)                                        # a slice reaching past B_total
    local(B, 0, B, 9, 9, max_change=mc)                          # the derivative mapper without action_prev
    for bad in (dict(B=1, n_elite=1), dict(B=4097, n_elite=9), dict(B=B, n_elite=0), dict(B=B, n_elite=B + 1),
                dict(B=B, n_elite=9, max_change=mc)):
        with pytest.raises((L.GpmpcError, ValueError)):
            engine.cem_search(w.mu0, w.S0, bad.pop("B"), H, A, 2, bad.pop("n_elite"), **bad)
    # ... and at the C entry point, where the engine's own argument handling is not in the way
    mu0, S0 = np.ascontiguousarray(w.mu0), np.ascontiguousarray(w.S0)
    out = torch.full((9, n + 2), -7.0, dtype=torch.float64, device=engine.device)
    state = torch.full((3 * n + 1,), -7.0, dtype=torch.float64, device=engine.device)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = engine.lib.gpmpc_cem_local(engine._h, ptr(mu0), ptr(S0), B, 0, B, H, A, 0, 0.0, 0, 9, 11, None, 1, ptr(mc), None, None,
                                    state.data_ptr(), out.data_ptr(), engine._stream())
    assert rc == L.GPMPC_ERR_ARG and b"derivative mapper" in engine.lib.gpmpc_last_error(engine._h)
    best = torch.full((n + 1,), -7.0, dtype=torch.float64, device=engine.device)
    rc = engine.lib.gpmpc_cem_search(engine._h, ptr(mu0), ptr(S0), B, H, A, 0, 0.0, 2, 9, 11, None, 1, ptr(mc), None, None,
                                     best.data_ptr(), engine._stream())
    assert rc == L.GPMPC_ERR_ARG
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7.0) and np.all(state.cpu().numpy() == -7.0) and np.all(best.cpu().numpy() == -7.0)
    assert same_bits(records(engine, w, B, 0, B, H, A, 0, 9, noise=noise), good)
    # lists x n_elite = 4097 records
    rec = torch.zeros((4097, n + 2), dtype=torch.float64, device=bare_engine.device)
    state = torch.full((3 * n + 1,), -7.0, dtype=torch.float64, device=bare_engine.device)
    with pytest.raises(L.GpmpcError):
        bare_engine.cem_merge(rec, 1, n, 0, state)
    with pytest.raises(L.GpmpcError):
        bare_engine.cem_merge(rec, 4097, n, 0, state)
    torch.cuda.synchronize()
    assert np.all(state.cpu().numpy() == -7.0)
    small = hand_made_records(3, 5, n, 5)
    got = run_merge(bare_engine, small, 5, n, 0, np.full(3 * n + 1, -7.0))
    assert same_bits(got[2 * n:], ref.refit(small, 5, None, True)[2 * n:])
