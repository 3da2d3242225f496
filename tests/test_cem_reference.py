"""Tier 1 (CPU): the numpy restatement of the device search (tests/cem_ref.py) against things outside it -- Philox's published
known answers and a textbook integer form of its rounds, the end points and the statistics of the draws, numpy's stable
argsort / mean / std, and the package's own action mappers.  tests/test_gpu_cem_search.py then holds the kernels to it."""
import numpy as np
import pytest
import torch

import cem_ref as ref


def _philox_textbook(counter, key):
    """Philox4x32-10 on Python integers, as published (Salmon et al., SC'11): mulhilo, xor, key bump between rounds."""
    c, k = list(counter), list(key)
    for r in range(10):
        if r > 0:
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
    return c


KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
          (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    assert tuple(_philox_textbook(counter, key)) == want
    got = ref.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], [np.array([k], dtype=np.uint64) for k in key])
    assert tuple(int(g[0]) for g in got) == want


def test_philox_array_form_matches_the_textbook_rounds_on_the_samplers_counters():
    seed = 2 ** 63 + 5
    idx = np.array([0, 1, 77, 2 ** 31 + 3, 2 ** 32 - 1], dtype=np.uint64)
    for it in (0, 3):
        got = ref.philox4x32_10((idx, np.full(5, it, np.uint64), np.full(5, 0x243F6A88, np.uint64), np.full(5, 0x9E3779B9, np.uint64)),
                                (np.full(5, seed & 0xFFFFFFFF, np.uint64), np.full(5, seed >> 32, np.uint64)))
        for j, i in enumerate(idx):
            want = _philox_textbook((int(i), it, 0x243F6A88, 0x9E3779B9), (seed & 0xFFFFFFFF, seed >> 32))
            assert [int(g[j]) for g in got] == want
            u0, u1 = ref.uniform2(seed, idx[j:j + 1], it)
            x0, x1 = (want[0] << 21) ^ (want[1] >> 11), (want[2] << 21) ^ (want[3] >> 11)
            assert x0 < 2 ** 53 and x1 < 2 ** 53
            assert u0[0] == (float(x0) + 0.5) * 2.0 ** -53 and u1[0] == (float(x1) + 0.5) * 2.0 ** -53


def test_uniform_end_points():
    u = ref.unit_from_53_bits(np.array([0, 2 ** 53 - 1, 2 ** 52], dtype=np.uint64))
    assert u[0] == 2.0 ** -54 and u[1] == 1.0 and u[2] == 0.5 + 2.0 ** -54
    assert np.isfinite(np.log(u[0]))
    u0, u1 = ref.uniform2(11, np.arange(4096 * 12, dtype=np.uint64), 1)
    for v in (u0, u1, ref.draws(11, 0, 4096, 12)):
        assert np.all(v > 0.0) and np.all(v <= 1.0)


def test_draw_statistics():
    B, n, seed = 4096, 12, 11
    u = ref.draws(seed, 0, B, n)
    z1, z2 = ref.draws(seed, 1, B, n), ref.draws(seed, 2, B, n)
    assert u.shape == z1.shape == (B, n)
    assert np.unique(u).size == B * n and np.unique(z1).size == B * n
    corr = lambda a, b: float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    figures = (u.mean(), 12.0 * u.var(), z1.mean(), z1.var(), corr(z1, z2), corr(z1[:, :-1], z1[:, 1:]))
    print("uniform mean %.4f 12 var %.4f normal mean %.4f var %.4f corr(it 1, it 2) %.4f corr(neighbours) %.4f" % figures)
    assert abs(figures[0] - 0.5) < 0.01 and abs(figures[1] - 1.0) < 0.02
    assert abs(figures[2]) < 0.02 and abs(figures[3] - 1.0) < 0.02
    assert abs(figures[4]) < 0.02 and abs(figures[5]) < 0.02
    # the longdouble form starts from the same uniforms: it differs from the float64 one by rounding only
    z1_ld = ref.draws(seed, 1, B, n, np.longdouble)
    assert z1_ld.dtype == np.longdouble and float(np.max(np.abs(z1_ld - z1))) < 1e-13
    assert np.array_equal(ref.draws(seed, 0, B, n, np.longdouble).astype(np.float64), u)


def test_sample_slots_and_global_indexing():
    rng = np.random.default_rng(0)
    B, n = 13, 4
    noise = np.concatenate([rng.uniform(size=(1, B, n)), rng.standard_normal((2, B, n))])
    first = rng.uniform(size=n)
    state = np.concatenate([np.full(n, 0.5), np.full(n, 0.25), rng.uniform(size=n), [1.5]])
    for src in (noise, 7):
        d0 = noise[0] if src is noise else ref.draws(7, 0, B, n)
        d1 = noise[1] if src is noise else ref.draws(7, 1, B, n)
        X0 = ref.sample(0, 0, B, B, n, None, None, src)
        assert np.array_equal(X0, d0)
        X0w = ref.sample(0, 0, B, B, n, None, first, src)
        assert np.array_equal(X0w[0], first) and np.array_equal(X0w[1:], d0[1:])
        X1 = ref.sample(1, 0, B, B, n, state, first, src)
        assert np.array_equal(X1[0], state[2 * n:3 * n])
        assert np.array_equal(X1[1:], np.clip(0.5 + 0.25 * d1[1:], 0.0, 1.0))
        # slices are rows of the whole population; the warm start / incumbent belongs to global slot 0 only
        for it, whole in ((0, X0w), (1, X1)):
            parts = [ref.sample(it, lo, hi - lo, B, n, state, first, src) for lo, hi in ((0, 5), (5, 5), (5, 13))]
            assert parts[1].shape == (0, n) and np.array_equal(np.concatenate(parts), whole)


def _keys_with_ties(rng, size):
    J = rng.choice(np.array([0.25, 0.5, 0.5, 1.0, np.inf, np.nan, -1.0, 0.25]), size=size)
    return J


@pytest.mark.parametrize("B,n_elite", [(2, 1), (2, 2), (17, 5), (17, 17), (64, 9), (65, 65), (5, 9)])
def test_elite_records_against_stable_argsort(B, n_elite):
    rng = np.random.default_rng(B * 100 + n_elite)
    n, b0 = 3, 40
    J, X = _keys_with_ties(rng, B), rng.uniform(size=(B, n))
    rec = ref.elite_records(J, X, b0, n_elite)
    assert rec.shape == (n_elite, n + 2)
    Jc = np.where(np.isnan(J), np.inf, J)
    order = np.argsort(Jc, kind="stable")[:n_elite]
    real = min(B, n_elite)
    assert np.array_equal(rec[:real, 0], Jc[order]) and np.array_equal(rec[:real, 1], order + b0)
    assert np.array_equal(rec[:real, 2:], X[order])
    assert np.all(rec[real:, 0] == np.inf) and np.all(rec[real:, 1] == 2147483647.0) and np.all(rec[real:, 2:] == 0.0)
    for v in np.unique(rec[:real, 0]):                           # the rows of a tied group come out by index
        assert np.all(np.diff(rec[:real, 1][rec[:real, 0] == v]) > 0)


def test_elite_records_of_an_empty_slice_are_padding():
    rec = ref.elite_records(np.empty(0), np.empty((0, 4)), 7, 3)
    assert rec.shape == (3, 6) and np.all(rec[:, 0] == np.inf) and np.all(rec[:, 1] == 2147483647.0) and np.all(rec[:, 2:] == 0.0)


@pytest.mark.parametrize("lists,n_elite", [(1, 1), (1, 2), (3, 5), (8, 8), (5, 13)])
def test_refit_against_numpy_mean_and_std(lists, n_elite):
    rng = np.random.default_rng(lists * 100 + n_elite)
    R, n = lists * n_elite, 7
    rec = np.empty((R, n + 2))
    rec[:, 0] = rng.choice(np.array([0.25, 0.5, 1.0, np.inf, -1.0]), size=R)
    rec[:, 1] = rng.permutation(R) + 3                            # slot order differs from index order
    rec[:, 2:] = rng.uniform(size=(R, n))
    if R > 4:                                                     # a list that is part padding
        rec[-2:, 0], rec[-2:, 1], rec[-2:, 2:] = np.inf, 2147483647.0, 0.0
    by_index = np.argsort(rec[:, 1], kind="stable")
    order = by_index[np.argsort(rec[by_index, 0], kind="stable")]
    lead = rec[order[:n_elite]]
    old = np.concatenate([np.zeros(2 * n), rng.uniform(size=n), [lead[0, 0]]])    # an incumbent as good as the leader
    for dtype in (np.float64, np.longdouble):
        st = ref.refit(rec, n_elite, np.zeros(3 * n + 1), True, dtype)
        assert st.dtype == dtype and st.shape == (3 * n + 1,)
        assert np.allclose(st[:n].astype(np.float64), lead[:, 2:].mean(axis=0), rtol=0, atol=1e-15)
        assert np.allclose(st[n:2 * n].astype(np.float64), lead[:, 2:].std(axis=0) + 1e-3, rtol=0, atol=1e-15)
        assert np.array_equal(st[2 * n:3 * n].astype(np.float64), lead[0, 2:]) and float(st[3 * n]) == lead[0, 0]
        kept = ref.refit(rec, n_elite, old, False, dtype)        # strict improvement only
        assert np.array_equal(kept[2 * n:].astype(np.float64), old[2 * n:]) and np.array_equal(kept[:2 * n], st[:2 * n])
        worse = old.copy()
        worse[3 * n] = np.nextafter(lead[0, 0], np.inf) if np.isfinite(lead[0, 0]) else np.inf
        took = ref.refit(rec, n_elite, worse, False, dtype)
        if np.isfinite(lead[0, 0]):
            assert np.array_equal(took[2 * n:], st[2 * n:])
    if n_elite == 1:
        st = ref.refit(rec, 1, np.zeros(3 * n + 1), True)
        assert np.array_equal(st[:n], lead[0, 2:]) and np.all(st[n:2 * n] == 1e-3)


def test_refit_adopts_the_leader_by_index_when_every_key_is_infinite():
    n = 3
    rec = np.zeros((6, n + 2))
    rec[:, 0] = np.inf
    rec[:, 1] = [4, 2, 5, 1, 3, 0]
    rec[:, 2:] = np.arange(18).reshape(6, 3) / 18.0
    st = ref.refit(rec, 2, np.full(3 * n + 1, -7.0), True)
    assert np.array_equal(st[2 * n:3 * n], rec[5, 2:]) and st[3 * n] == np.inf
    assert np.allclose(st[:n], (rec[5, 2:] + rec[3, 2:]) / 2.0, rtol=0, atol=1e-16)


@pytest.mark.parametrize("A", [1, 3])
def test_to_model_matches_the_package_mappers(A):
    from gp_mpc_amd.control_objects.actions_mappers.mappers import DerivativeActionMapper, NormalizationActionMapper
    from gp_mpc_amd.config_classes import ActionsConfig
    H, B = 5, 33
    rng = np.random.default_rng(A)
    X = rng.uniform(size=(B, H * A))
    mc = np.array([0.6, 0.7, 0.15])[:A]
    prev = np.array([0.1, 0.9, 0.5])[:A]
    ident = NormalizationActionMapper(np.zeros(A), np.ones(A), H, ActionsConfig())
    assert np.array_equal(ref.to_model(X, H, A), ident.mpc_to_model_batch(X))
    der = DerivativeActionMapper(np.zeros(A), np.ones(A), H, ActionsConfig(True, list(mc)))
    der.action_model_previous_iter = torch.as_tensor(prev)
    got, want = ref.to_model(X, H, A, mc, prev), der.mpc_to_model_batch(X)
    assert got.shape == want.shape == (B, H, A)
    assert np.array_equal(got, want)
    assert np.any(got == 0.0) and np.any(got == 1.0) and np.any((got > 0.0) & (got < 1.0))       # both clamps act
    if A == 3:                                                   # each action dimension has its own scale and start
        assert not np.array_equal(got, ref.to_model(X, H, A, np.full(A, mc[0]), prev))
        assert not np.array_equal(got, ref.to_model(X, H, A, mc, np.full(A, prev[0])))
